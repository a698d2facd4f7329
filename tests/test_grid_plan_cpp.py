"""Which form builds the ICP search grid of a launch (plan::sorted_grid_build in staticmapping_amd/csrc/icp_plan.h) is a pure host
function: compiled with g++ alone and checked at its limits on the CPU box (tests/cpp/test_grid_plan.cc)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_include() -> str:
    for cand in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if cand and os.path.exists(os.path.join(cand, "include", "hip", "hip_runtime.h")):
            return os.path.join(cand, "include")
    raise RuntimeError("HIP headers not found (smhip_device.h includes hip/hip_runtime.h for the vector types)")


def test_grid_build_choice_at_its_limits():
    build = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "test_grid_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_grid_plan.cc")
    csrc = os.path.join(ROOT, "staticmapping_amd", "csrc")
    deps = [src, os.path.join(csrc, "icp_plan.h"), os.path.join(csrc, "smhip_device.h"), os.path.join(ROOT, "include", "smhip.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I", _hip_include(), "-I", csrc,
                               "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    out = subprocess.run([exe], text=True, capture_output=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
