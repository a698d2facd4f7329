"""include/smhip/submap.h without a GPU: tests/cpp/test_submap.cc compiles, and its `host` mode checks the bookkeeping of
static_map::Submap -- local poses, full after frame_count frames, the refused insert after that, the voxel size's six-decimal trip
through the filter text, and the (source, target, guess) order of the consecutive pairs ConnectSubmaps matches
(map_builder.cc:399-429)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_submap.cc")


def _build_exe():
    from staticmapping_amd import build
    lib = build.build()
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_submap")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    hdrs = [os.path.join(ROOT, "include", "smhip", h) for h in ("submap.h", "back_end.h", "registrator.h", "filters.h")] + [os.path.join(ROOT, "include", "smhip.h")]
    if (not os.path.exists(exe)) or max([os.path.getmtime(SRC), os.path.getmtime(lib)] + [os.path.getmtime(h) for h in hdrs]) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                               "-L", os.path.dirname(lib), "-lsmhip", "-Wl,-rpath," + os.path.dirname(lib),
                               "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_submap_header_compiles_without_a_gpu():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), SRC])


def test_submap_bookkeeping_on_the_host():
    out = subprocess.run([_build_exe(), "host"], text=True, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout


def test_driver_knows_the_submap_flags():
    from staticmapping_amd import build
    build.build()
    out = subprocess.run([build.build_shard_driver(), "--scans", "/nonexistent", "--submap-frames", "0"], text=True, capture_output=True, timeout=60)
    assert out.returncode == 2 and "--submap-frames >= 1" in out.stderr
    out = subprocess.run([build.build_shard_driver(), "--no-such-flag"], text=True, capture_output=True, timeout=60)
    assert "--submap-edges" in out.stderr and "--submap-min-score" in out.stderr
