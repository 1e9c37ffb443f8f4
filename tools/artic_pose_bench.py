"""Cost of pose coordinates in the articulated step (include/moby_hip_artic.h, MH_ARTIC_BASE_POSE): the hinged pair of
tests/scenes/floating_hinged_pair.xml in free flight (its spheres and the stabiliser off: the four-waves kernel k_artic_step_w4 against
k_artic_step_w4_pose), B perturbed copies x 200 steps of 1e-3 -- short enough that angle coordinates stay clear of the middle hinge's quarter
turn -- angle and pose batches launched alternately, timed by device events after a warm-up of each.  Prints one JSON line: per variant the
median and the spread (min, max) in ms, the ratio of the medians, and how far the two runs' base link poses end apart.
usage: python tools/artic_pose_bench.py [--reps 10] [--B 8192] [--steps 200]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from moby_amd import artic as A, scene as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    m, _, _, q0, qd0, _ = A.load_xml(os.path.join(ROOT, "tests", "scenes", "floating_hinged_pair.xml"))
    m.nspheres = 0; m.cstab_max_iterations = 0
    B, nj, n, dt = a.B, m.nj, a.steps, 1e-3
    rng = np.random.default_rng(1)
    q = np.tile(q0, (B, 1)); qd = np.tile(qd0, (B, 1))
    q[:, 3:6] += rng.uniform(-0.3, 0.3, (B, 3)); q[:, 6] = rng.uniform(-0.5, 0.3, B); qd += rng.uniform(-0.5, 0.5, (B, nj))
    dev = torch.device("cuda", 0)
    batches = {"angles": A.ArticBatch(m, q, qd), "pose": A.ArticBatch(m, np.zeros_like(q), np.zeros_like(qd), base_coords="pose")}
    P0 = batches["pose"].base_pose()
    stream = torch.cuda.current_stream(dev).cuda_stream
    times = {k: [] for k in batches}
    out = {}
    for rep in range(a.reps + 1):                 # rep 0: warm-up of both (and their outcome)
        for k, ab in batches.items():
            ab.upload(q, qd, S.new_aux(B))
            if k == "pose":
                ab.set_base_pose(P0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ab.step(dt, n, stream=stream)
            e1.record(); e1.synchronize()
            if rep:
                times[k].append(e0.elapsed_time(e1))
            else:
                aux = ab.download()[2]
                out[k] = dict(finished=int((aux["steps"] == n).sum()), base=ab.link_poses()[:, 5])
    for ab in batches.values():
        ab.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"bench": "artic_pose", "B": B, "steps": n, "dt": dt, "reps": a.reps,
           "ms": {k: {"median": med[k], "min": float(min(v)), "max": float(max(v))} for k, v in times.items()},
           "ratio_pose_to_angles": med["pose"] / med["angles"],
           "ratio_spread": [min(times["pose"]) / max(times["angles"]), max(times["pose"]) / min(times["angles"])],
           "worlds_finished": {k: v["finished"] for k, v in out.items()},
           "base_pose_max_diff": float(np.abs(out["pose"]["base"] - out["angles"]["base"]).max())}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
