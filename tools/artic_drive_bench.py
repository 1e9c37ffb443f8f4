"""Cost of a drive in the articulated step (include/moby_hip_artic.h, mh_artic_batch_step_driven): BASELINE config 5 (ur10 x 8192, 200 steps of
5e-4 from ur10_states) undriven, and driven with one held row (rows = 1) and with a row per step (rows = 200) -- an all-zero drive (the
undriven trajectory: the cost of the drive itself) and a servo + force (the same trajectory for both row counts) -- launches alternating, timed
by device events after a warm-up of each; the drive's arrays are device tensors (zero-copy).  Prints one JSON line: per variant the median and
the spread (min, max) in ms, the ratios of the medians to the undriven one, the LCP solves, and whether the trajectory is the undriven one.
usage: python tools/artic_drive_bench.py [--reps 10] [--B 8192] [--steps 200]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from moby_amd import artic as A, scene as S  # noqa: E402
from tests.test_artic_gpu import ur10_states  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    m, _, _ = A.load_sdf(os.path.join(ROOT, "tests", "scenes", "ten_joint_arm.sdf"))
    B, nj, n, dt = a.B, m.nj, a.steps, 5e-4
    q0, qd0 = ur10_states(m, B)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    Z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device=dev)
    on = np.ones(nj); on[[0, 7]] = 0.0                # the two near-fixed joints stay undriven, as in example/ur10/controller.cpp
    kp, kv, ff = T(rng.uniform(0.0, 5.0, (B, nj)) * on), T(rng.uniform(0.0, 0.05, (B, nj)) * on), T(rng.uniform(-1, 1, (B, nj)) * on)
    qdes = T(q0)
    # zero_*: every term present, all zero -- the undriven trajectory, so the difference is what the drive itself costs;
    # pd_*: a servo to the start pose plus a constant force, the schedule repeating the held row -- the same trajectory for both row counts
    variants = {"undriven": None,
                "zero_rows1": A.Drive(kp=Z(B, nj), kv=Z(B, nj), q_des=Z(B, nj), qd_des=Z(B, nj), tau_ff=Z(B, nj)),
                "zero_rows%d" % n: A.Drive(kp=Z(B, nj), kv=Z(B, nj), q_des=Z(n, B, nj), qd_des=Z(n, B, nj), tau_ff=Z(n, B, nj)),
                "pd_rows1": A.Drive(kp=kp, kv=kv, q_des=qdes, qd_des=Z(B, nj), tau_ff=ff),
                "pd_rows%d" % n: A.Drive(kp=kp, kv=kv, q_des=qdes.expand(n, B, nj).contiguous(), qd_des=Z(n, B, nj), tau_ff=ff.expand(n, B, nj).contiguous())}
    ab = A.ArticBatch(m, q0, qd0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    times = {k: [] for k in variants}
    finished, solves, same_as_undriven = {}, {}, {}
    for rep in range(a.reps + 1):                 # rep 0: warm-up of every variant (and its outcome)
        for k, d in variants.items():
            ab.upload(q0, qd0, S.new_aux(B))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ab.step(dt, n, stream=stream, drive=d)
            e1.record(); e1.synchronize()
            if rep:
                times[k].append(e0.elapsed_time(e1))
            else:
                q, qd, aux = ab.download()
                finished[k] = int(((aux["steps"] == n) & np.isfinite(q).all(axis=1)).sum())   # worlds that ran every step
                solves[k] = int(aux["lcp_solves"].sum())
                if k == "undriven":
                    ref = (q, qd)
                same_as_undriven[k] = bool(np.array_equal(q, ref[0]) and np.array_equal(qd, ref[1]))
    ab.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = {"bench": "artic_drive", "B": B, "steps": n, "dt": dt, "reps": a.reps,
           "ms": {k: {"median": med[k], "min": float(min(v)), "max": float(max(v))} for k, v in times.items()},
           "ratio": {k: med[k] / med["undriven"] for k in times if k != "undriven"}, "worlds_finished": finished,
           "lcp_solves": solves, "bit_equal_to_undriven": same_as_undriven}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
