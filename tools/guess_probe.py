"""smhip_shard --guess ctrv against --guess constant on the `end_to_end` drive of bench.py --full.

  guess_probe.py [--scans 1025] [--runs 5] [--out FILE]
      generates the drive as bench.end_to_end does (seed 5, 8 m/s, 10 Hz, yaw rate +-0.2 rad/s, 120 000 points a scan), then runs the
      driver 1 + RUNS times per setting -- constant guess with 20 fixed iterations (the bench's), ctrv with --early-exit 1, and ctrv
      with 20 fixed iterations -- and prints the medians of pairs_per_s and mean_iterations after the first run."""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sources_sha256():
    h = hashlib.sha256()
    for f in ("icp_one.hip", "icp_kernels.hip", "grid_sort_build.hip", "smhip_device.h", "shard_driver.cc"):
        h.update(open(os.path.join(ROOT, "staticmapping_amd", "csrc", f), "rb").read())
    return h.hexdigest()


def throughput(args):
    import torch  # noqa: F401  (before the package: one HIP runtime per process)
    import numpy as np
    from staticmapping_amd import build, kitti, synth
    exe = build.SHARD_EXE
    root = tempfile.mkdtemp(prefix="smhip_guess_probe_", dir="/tmp")
    try:
        drive = os.path.join(root, "drive")
        os.makedirs(drive)
        poses = synth.drive_poses(args.scans, seed=5, speed=8.0, hz=10.0, yaw_rate_max=0.2)
        scene = synth.make_drive_scene(poses, seed=5)
        for k, P in enumerate(poses):
            kitti.write_bin(kitti.scan_path(drive, k), synth.velodyne_scan(synth.scene_near(scene, P[:3, 3]), P, seed=1000 + k, n_points=120_000, device="cuda:0"))
        truth = [np.linalg.inv(poses[0]) @ P for P in poses]
        settings = {"constant_fixed20": ["--guess", "constant", "--iterations", "20", "--early-exit", "0"],
                    "ctrv_early_exit": ["--guess", "ctrv", "--iterations", "100", "--early-exit", "1"],
                    "ctrv_fixed20": ["--guess", "ctrv", "--iterations", "20", "--early-exit", "0"]}
        out = {"workload": f"{args.scans}-scan drive of bench.py's end_to_end leg through smhip_shard, --guess-tx 0.8, default batch; medians of {args.runs} runs after one",
               "kernel_sources_sha256": sources_sha256()}
        pose_file = os.path.join(root, "kitti_pose.txt")
        for name, flags in settings.items():
            rows = []
            for rep in range(1 + args.runs):
                r = subprocess.run([exe, "--scans", drive, "--gpus", "1", "--guess-tx", "0.8", "--out", pose_file] + flags, text=True, capture_output=True, timeout=600)
                if r.returncode != 0:
                    print(json.dumps({"error": name, "status": r.returncode, "stderr": r.stderr[-400:]}))
                    return 1                      # nothing more is started after a failed run
                rows.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
            est = kitti.read_poses(pose_file)
            rows = rows[1:]
            out[name] = {"pairs_per_s": statistics.median(r["pairs_per_s"] for r in rows), "pairs_per_s_runs": [r["pairs_per_s"] for r in rows],
                         "steady_state_pairs_per_s": statistics.median(r["steady_state_pairs_per_s_rank0"] for r in rows),
                         "mean_iterations": statistics.median(r["mean_iterations"] for r in rows), "unfinished_pairs": rows[-1]["unfinished_pairs"],
                         "pairs": rows[-1]["pairs"], "batch": rows[-1]["batch"],
                         "worst_distance_to_truth_m": float(max(np.linalg.norm(est[k][:3, 3] - truth[k][:3, 3]) for k in range(len(truth))))}
        text = json.dumps(out, indent=1)
        print(text)
        if args.out:
            open(args.out, "w").write(text + "\n")
        return 0
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1025)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out")
    sys.exit(throughput(ap.parse_args()))
