"""The per-unit build of libsmhip.so and of the smhip_shard driver: every source file belongs to a unit or to the driver, and an edit
recompiles exactly what the compiler-written dependency files say reads the edited file (no GPU needed: hipcc cross-compiles for gfx950)."""
import os

from staticmapping_amd import build

DRIVER = "shard_driver.cc"


def _compiled_at():
    return {u: os.path.getmtime(build.dep_path(u)) for u in build.UNITS}


def test_no_orphan_sources():
    build.build()
    named = {p for u in build.UNITS + [DRIVER] for p in build.unit_deps(u)}
    units = {os.path.join(build.CSRC, u) for u in build.UNITS}
    assert units <= named                                        # a unit's dependency file names the unit itself
    assert os.path.join(build.CSRC, DRIVER) in build.unit_deps(DRIVER)   # and so does the driver's
    orphans = [f for f in sorted(os.listdir(build.CSRC)) if os.path.join(build.CSRC, f) not in named]
    assert orphans == []


def test_second_build_compiles_nothing():
    build.build()
    before = _compiled_at()
    lib = os.path.getmtime(build.LIB_PATH)
    build.build()
    assert _compiled_at() == before
    assert os.path.getmtime(build.LIB_PATH) == lib


def test_touched_header_recompiles_its_units_only():
    # (a tree copied without its objects has a current library, but any link has to make the missing objects first)
    build.build(force=not all(os.path.exists(build.obj_path(u)) for u in build.UNITS))
    header = os.path.join(build.CSRC, "prep_normals.h")
    users = {u for u in build.UNITS if header in build.unit_deps(u)}
    assert {"prep_normals.hip", "smhip_api.hip"} <= users < set(build.UNITS)
    before = _compiled_at()
    st = os.stat(header)
    try:
        os.utime(header)                                         # now: later than every dependency file
        build.build()
    finally:
        os.utime(header, ns=(st.st_atime_ns, st.st_mtime_ns))    # the content never changed: what was just built stays current
    after = _compiled_at()
    assert {u for u in build.UNITS if after[u] > before[u]} == users
    assert os.path.getmtime(build.LIB_PATH) >= max(after.values())


def test_touched_header_relinks_the_driver_and_no_library_unit():
    build.build()
    exe = build.build_shard_driver()
    header = os.path.join(build.ROOT, "include", "smhip", "m2dp.h")     # the driver reads it through other headers only
    assert header in build.unit_deps(DRIVER)
    before, linked = _compiled_at(), os.stat(exe).st_mtime_ns
    build.build_shard_driver()
    assert os.stat(exe).st_mtime_ns == linked                    # nothing is newer than the program: no second link
    st = os.stat(header)
    try:
        os.utime(header)                                         # now: later than the program
        build.build_shard_driver()
    finally:
        os.utime(header, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert os.stat(exe).st_mtime_ns > linked
    assert _compiled_at() == before and os.path.getmtime(build.LIB_PATH) <= os.path.getmtime(exe)
