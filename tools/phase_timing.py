"""Diagnostic (needs a library built with -DSMHIP_PHASE_TIMING=1): per-phase cycle shares of nn_ball_lds and the search rounds per path
(points staged / row tables only / global lookups) with their cycles (SMHIP_DEBUG_FLAGS=16), 64 pairs, 8 iterations, one stream.
finalize prints one line per iteration.  The batch is aligned twice: the counters' memory is not cleared when the handle is made, so
the first Align's line for iteration 0 may hold leftovers; read the second Align's lines."""
import os, sys
os.environ["SMHIP_DEBUG_FLAGS"] = "16"
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import staticmapping_amd as sm
from staticmapping_amd import synth
a, b, T = synth.scan_pair("cfg2", n_points=120000)
q, n = sm.calculate_normals(a[:, :3].astype(np.float64))
B = 64
guess = synth.make_pose(t=(0.6, 0, 0))
m = sm.IcpFastHip(pair_slots=B, max_source_points=len(b), max_target_points=len(q), max_iteration=8, early_exit=0, no_overlap=1)
m.set_input_source(b); m.set_input_target(q, n)
for s in range(1, B): m.copy_slot(0, s)
for k in range(2):
    print(f"--- Align {k + 1}", flush=True)
    m.align_batch(B, [guess] * B)
    m.synchronize()
m.close()
