"""The serial end of Ndt ON THE DEVICE: the Newton solve (ndt_solve6 with its fallback) and the More-Thuente loop with the state
machine that drives it (ndt_ctl_step, arithmetic in csrc/ndt_ctl_math.h), at options for which the loop runs -- with the wrapper's
settings it is dead code, and no other suite sets step_size.  Every case runs in a process of its own under a timeout
(tests/ndt_ctl_gpu_cases.py): a control bug can stall the round loop, and it must end the case, not the session.

The clouds: a 3 000-point scan against 12 000 points merged from 3 scans (ndt_case of test_ndt_gpu.py, smaller), resolution 1.0.
The reference of every Align is the C oracle's (oracle/cref.py) with the same options as floats: iterations and derivative calls
equal, the pose, the fitness score and the transformation probability inside the bounds test_ndt_align_parity already asserts
(1e-4 rad, 1e-3 m, 1e-3 and 1e-4 relative).

solve6_device  smhip_ndt_debug_solve6 on the 110 systems of tests/ndt_ctl_cases.py: |x - x_exact| <= max(8 x the oracle's own error,
               64 eps cond_kept |x_exact|), x_exact the 60-digit pseudo-inverse under JacobiSVD's rule.  The `hidden` family is
               the one the host test found the defect with: elimination pivots within ten decades while a singular value is
               below the threshold -- solved by elimination they came out 3e14 off; ndt_solve6 now switches on a bound of the
               condition number, and this case holds the device's contracted arithmetic to the same rule.
mt_loop        (step_size, transformation_epsilon) = (0.05, 0.1), (0.1, 0.2), (0.1, 0.5), guesses 0.3 m and 0.8 m + 2 degrees off;
               the oracle's trace must show a loop of at least 2 trials and the closing Hessian-only evaluation in every run
exits          no overlap (the source 200 m away: the guess comes back exactly, 0 iterations, 1 derivative call, 0 pairs, a finite
               fitness score), max_iterations 1 and 2 at epsilon 0.01 (the oracle's uncapped run is longer), default options with
               the 0.8 m guess (the oracle's first step is clamped to step_size)
mixed_batch    five guesses in one smhip_ndt_align_batch at (0.1, 0.2): the oracle's loop lengths differ, so Hessian and no-Hessian
               requests share launches and the jobs end in different rounds; every slot equals its single call bit for bit
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(name, timeout=120):
    p = subprocess.run([sys.executable, os.path.join(HERE, "ndt_ctl_gpu_cases.py"), name], capture_output=True, text=True, timeout=timeout)
    print(p.stdout)
    print(p.stderr[-4000:], file=sys.stderr)
    assert p.returncode == 0, (name, p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.strip().splitlines()[-1] == "ok " + name


def test_solve6_on_the_device():
    run_case("solve6_device")


def test_more_thuente_loop_runs_and_matches_the_oracle():
    run_case("mt_loop")


def test_exits():
    run_case("exits")


def test_mixed_batch_equals_single_calls_and_the_oracle():
    run_case("mixed_batch")
