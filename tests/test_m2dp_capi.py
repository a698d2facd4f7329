"""The host-only entries of the M2DP C ABI (no GPU): smhip_m2dp_default_options, smhip_m2dp_length with its refusals, and
smhip_m2dp_match against the restated matchTwoM2dpDescriptors; the ctypes mirror of smhip_m2dp_options against the header."""
import ctypes
import os
import subprocess

import numpy as np

import m2dp_ref as mr
from staticmapping_amd import _capi
from staticmapping_amd import m2dp as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_defaults_and_length():
    o = dm.make_options()
    assert (o.r, o.max_distance, o.t, o.p, o.q) == (0.1, 100.0, 16, 4, 16)                   # m2dp.h:48-49
    assert dm.length(o) == mr.length(mr.options()) == 64 + 32 * 16
    nd = dict(t=8, p=2, q=4, r=0.5, max_distance=50.0)
    assert dm.length(dm.make_options(**nd)) == mr.length(mr.options(**nd)) == 8 + 10 * 8
    assert dm.length(dm.make_options(r=1e-6, max_distance=1e-6, t=1, p=1, q=1)) == 2        # r = 1e-6 is not "too small" (:64)
    assert dm.length(dm.make_options(p=4, q=16, t=512, r=1.0, max_distance=256.0)) == 64 + 8192   # exactly the device limits
    lib = _capi.load_library()
    assert lib.smhip_m2dp_length(None) == -1
    for kw in (dict(r=0.999e-6), dict(r=float("nan")), dict(r=float("inf")), dict(max_distance=float("nan")), dict(max_distance=float("inf")),
               dict(max_distance=0.0), dict(max_distance=-1.0), dict(t=0), dict(p=0), dict(q=0), dict(t=-3), dict(p=5, q=13),
               dict(t=513, r=1.0, max_distance=256.0), dict(r=1e-6, max_distance=1e30), dict(p=1 << 16, q=1 << 16)):
        assert dm.length(dm.make_options(**kw)) == -1, kw


def test_match_equals_the_restatement():
    rng = np.random.default_rng(2)
    P, Q = rng.uniform(0, 1, 576).astype(np.float32), rng.uniform(0, 1, 576).astype(np.float32)
    # the two sum 576 products in different orders: each sum is good to 576 eps of ~2e2, the numerator N P.Q - sum P sum Q
    # cancels from ~8e4 to ~3e2 over a denominator of ~3e4, so the scores agree to a few 1e-13 at worst
    assert abs(dm.match(P, Q) - mr.match(P, Q)) <= 1e-12
    assert abs(dm.match(P, P) - 1.0) <= 1e-12
    assert dm.match(-P, Q) == dm.match(P, Q) == dm.match(Q, P)
    assert dm.match(P, Q[:-1]) == -1.0 and dm.match(P[:9], Q[:9]) == -1.0 and dm.match(P[:10], Q[:10]) >= 0.0
    lib = _capi.load_library()
    assert lib.smhip_m2dp_match(None, Q.ctypes.data_as(_capi.c_float_p), 576) == -1.0


def test_ctypes_mirror_has_the_headers_layout(tmp_path):
    fields = [f for f, _ in _capi.M2dpOptions._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smhip.h"\nint main(void) {\n  printf("%zu\\n", sizeof(smhip_m2dp_options));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(smhip_m2dp_options, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert ctypes.sizeof(_capi.M2dpOptions) == out[0]
    assert [getattr(_capi.M2dpOptions, f).offset for f in fields] == out[1:]


def test_probe_reads_a_kernel_stats_file(tmp_path):
    """tools/m2dp_probe.py --kernel-stats on a file in the layout of profiles/submap_probe_kernel_stats.csv (rocprofv3
    --kernel-trace --stats, demangled names) and with a mangled name"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("m2dp_probe", os.path.join(ROOT, "tools", "m2dp_probe.py"))
    probe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    f = tmp_path / "kernel_stats.csv"
    f.write_text('"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"\n'
                 '"(anonymous namespace)::m2dp_hist(HIP_vector_type<float, 4u> const*, int, float const*, int, int, int, int, int, double, double, int*)",22,2200000,100000.0,50.0,1,2,0.1\n'
                 '"_ZN12_GLOBAL__N_115m2dp_descriptorEPKiiiPdPfPi",22,1100000,50000.0,25.0,1,2,0.1\n'
                 '"void rocprim::detail::radix_sort_block_sort<unsigned long long*>(unsigned int)",10,999,99.9,1.0,1,2,0.1\n')
    assert probe.kernel_times(str(f)) == {"m2dp_hist": {"calls": 22, "mean_us": 100.0}, "m2dp_descriptor": {"calls": 22, "mean_us": 50.0}}
