"""In-tree build of libsmhip.so (gfx950 only).  `python -m staticmapping_amd.build [--force]`.

One object per translation unit under lib/obj/, compiled concurrently, then one link.  A unit is compiled again when a file
its compiler-written dependency file (-MD) names is newer than that dependency file, or when the flags change."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libsmhip.so")
SHARD_EXE = os.path.join(LIB_DIR, "smhip_shard")          # C++ sharded sequence driver (RCCL gather), csrc/shard_driver.cc
OBJ_DIR = os.path.join(LIB_DIR, "obj")
FLAGS_STAMP = os.path.join(OBJ_DIR, "flags.txt")          # the compile flags the objects and dependency files were made with

# translation units, slowest first (each #includes its kernel files and fragments: its dependency file lists them)
UNITS = ["smhip_api.hip", "smhip_mrvm.hip", "cloud_filters.hip", "prep_normals.hip", "smhip_ndt_gicp.hip", "smhip_filter_api.hip", "smhip_m2dp.hip",
         "smhip_submap.hip", "smhip_pose_graph.hip", "smhip_icp_information.hip", "guess_search.hip", "host_cloud.cc", "map_package.cc"]


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: libsmhip.so can only be built with the ROCm toolchain")


def _jobs() -> int:
    return max(1, min(16, int(os.environ.get("MAX_JOBS") or os.cpu_count() or 1)))


def obj_path(unit: str) -> str:
    return os.path.join(OBJ_DIR, os.path.splitext(unit)[0] + ".o")


def dep_path(unit: str) -> str:
    return os.path.join(OBJ_DIR, os.path.splitext(unit)[0] + ".d")


def unit_deps(unit: str) -> list[str]:
    """The files the unit's last compilation read (its own source included), from the dependency file; [] if there is none."""
    try:
        with open(dep_path(unit)) as fh:
            rule = fh.read().replace("\\\n", " ")
    except OSError:
        return []
    return [os.path.normpath(os.path.join(ROOT, p)) for p in rule.partition(": ")[2].split()]


def _stale(unit: str) -> bool:
    deps = unit_deps(unit)
    if not deps:
        return True
    t = os.path.getmtime(dep_path(unit))
    return any(not os.path.exists(p) or os.path.getmtime(p) > t for p in deps)


def build_shard_driver(force: bool = False, verbose: bool = False) -> str:
    """The C++ host program of BASELINE config #4: links libsmhip.so + librccl.so (no device code of its own).  One command compiles and
    links it; it runs again when a file its dependency file names, or the library, is newer than the program."""
    unit = "shard_driver.cc"
    deps = unit_deps(unit)
    if not force and deps and os.path.exists(SHARD_EXE):
        t = os.path.getmtime(SHARD_EXE)
        if all(os.path.exists(p) and os.path.getmtime(p) <= t for p in deps + [LIB_PATH]):
            return SHARD_EXE
    os.makedirs(OBJ_DIR, exist_ok=True)
    cmd = [_hipcc(), "-O2", "-std=c++17", "-I", "include", os.path.relpath(os.path.join(CSRC, unit), ROOT), "-o", SHARD_EXE, "-MD", "-MF", dep_path(unit),
           "-L", LIB_DIR, "-lsmhip", "-L", "/opt/rocm/lib", "-lrccl", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    try:
        subprocess.check_call(cmd, cwd=ROOT)
    except BaseException:
        if os.path.exists(dep_path(unit)):          # no dependency file without the program it describes
            os.remove(dep_path(unit))
        raise
    return SHARD_EXE


def _compile(unit: str, flags: list[str], verbose: bool) -> None:
    # run from the repository root on paths relative to it, so that a copy of the tree elsewhere is not stale
    cmd = [_hipcc()] + flags + ["-c", os.path.relpath(os.path.join(CSRC, unit), ROOT), "-o", obj_path(unit), "-MD", "-MF", dep_path(unit)]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    try:
        subprocess.check_call(cmd, cwd=ROOT)
    except BaseException:
        if os.path.exists(dep_path(unit)):          # no dependency file without the object it describes
            os.remove(dep_path(unit))
        raise


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the stale HIP translation units for gfx950 and link staticmapping_amd/lib/libsmhip.so (+ the smhip_shard driver)."""
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", "include"]
    flags += os.environ.get("SMHIP_EXTRA_HIPCC_FLAGS", "").split()
    os.makedirs(OBJ_DIR, exist_ok=True)
    stamp = open(FLAGS_STAMP).read() if os.path.exists(FLAGS_STAMP) else None
    if force or stamp != " ".join(flags):           # nothing made with other flags counts: every unit is stale
        for u in UNITS:
            if os.path.exists(dep_path(u)):
                os.remove(dep_path(u))
        with open(FLAGS_STAMP, "w") as fh:
            fh.write(" ".join(flags))
    stale = [u for u in UNITS if _stale(u)]
    if not stale and os.path.exists(LIB_PATH) and all(os.path.getmtime(dep_path(u)) <= os.path.getmtime(LIB_PATH) for u in UNITS):
        build_shard_driver(False, verbose)
        return LIB_PATH
    # the link needs every object; one that is gone (objects do not travel with a copied tree) is compiled again
    stale = [u for u in UNITS if u in stale or not os.path.exists(obj_path(u))]
    with ThreadPoolExecutor(_jobs()) as pool:
        for done in [pool.submit(_compile, u, flags, verbose) for u in stale]:
            done.result()
    cmd = [_hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared", "-o", LIB_PATH] + [obj_path(u) for u in UNITS]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    build_shard_driver(True, verbose)
    return LIB_PATH


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
