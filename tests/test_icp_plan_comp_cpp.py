"""The inner-compensation plan of the IcpFast dispatch (staticmapping_amd/csrc/icp_plan.h, Inputs::compensation) on the CPU box:
tests/cpp/test_icp_plan_comp.cc, compiled with g++ alone -- no one_launch, no certificate or fused kernel, comp_apply first, and
with the flag off the plans the header made before it knew the flag."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_include() -> str:
    for cand in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if cand and os.path.exists(os.path.join(cand, "include", "hip", "hip_runtime.h")):
            return os.path.join(cand, "include")
    raise RuntimeError("HIP headers not found (smhip_device.h includes hip/hip_runtime.h for the vector types)")


def test_inner_compensation_program_compiles_without_a_gpu():
    """tests/cpp/test_inner_compensation.cc (run by tests/test_icp_compensation_gpu.py) against registrator.h, on the CPU box."""
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_inner_compensation.cc")])


def test_icp_plan_with_inner_compensation():
    build = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "test_icp_plan_comp")
    src = os.path.join(ROOT, "tests", "cpp", "test_icp_plan_comp.cc")
    csrc = os.path.join(ROOT, "staticmapping_amd", "csrc")
    deps = [src, os.path.join(csrc, "icp_plan.h"), os.path.join(csrc, "smhip_device.h"), os.path.join(ROOT, "include", "smhip.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I", _hip_include(), "-I", csrc,
                               "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    out = subprocess.run([exe], text=True, capture_output=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
