"""The per-unit build of libsmhip.so: every source file belongs to a unit, and an edit recompiles exactly the units whose
compiler-written dependency files name the edited file (no GPU needed: hipcc cross-compiles for gfx950)."""
import os

from staticmapping_amd import build


def _compiled_at():
    return {u: os.path.getmtime(build.dep_path(u)) for u in build.UNITS}


def test_no_orphan_sources():
    build.build()
    named = {p for u in build.UNITS for p in build.unit_deps(u)}
    units = {os.path.join(build.CSRC, u) for u in build.UNITS}
    assert units <= named                                        # a unit's dependency file names the unit itself
    orphans = [f for f in sorted(os.listdir(build.CSRC)) if f != "shard_driver.cc" and os.path.join(build.CSRC, f) not in named]
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
