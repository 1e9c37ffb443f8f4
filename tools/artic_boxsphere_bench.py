"""What the box-sphere kernels cost a model that has no box-sphere pair (include/moby_hip_artic.h, mh_artic_model.pair_kind; mh_artic_bsp.hip):
the four-sphere-foot slab of tools/artic_pair_bench.py (a floating slab with a sphere of radius 0.01 per foot dropped onto the plane under the
no-slip model, stabiliser off), B perturbed copies x `steps` steps of 1e-3, stepped alternately (a) by the pair kernels (mh_debug_set(13, 1)) and
(b) by the box-sphere kernels (mh_debug_set(14, 1)); the two give the same results bit for bit.  Batches launched alternately in one process,
timed by device events after a warm-up of each.  Prints one JSON line: per variant the median and the spread (min, max) in ms and
world-steps/s, and the ratio of the medians.  Models without a box-sphere pair or a static box never take these kernels: a record, not a gate.
usage: python tools/artic_boxsphere_bench.py [--reps 5] [--B 8192] [--steps 200]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from moby_amd import _lib, artic as A, scene as S  # noqa: E402

FEET = ((-0.4, -0.4), (0.4, -0.4), (-0.4, 0.4), (0.4, 0.4))


def slab(kind):
    m = A.model_from_links([], gravity=(0.0, -9.81, 0.0), floating_base=dict(R0=np.eye(3), x0=(0.0, 0.06, 0.0), mass=5.0, inertia=np.eye(3)))
    A.add_spheres(m, [(5, (x, -0.05, z), 0.01) for x, z in FEET], plane_normal=(0.0, 1.0, 0.0), epsilon=0.2, mu_coulomb=100.0)
    m.cstab_max_iterations = 0
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    B, n, dt = a.B, a.steps, 1e-3
    rng = np.random.default_rng(1)
    q = np.zeros((B, 6)); qd = np.zeros((B, 6))
    q[:, 1] = rng.uniform(0.0, 0.02, B); qd[:, 1] = -rng.uniform(0.0, 0.5, B); qd[:, 0] = rng.uniform(-0.2, 0.2, B)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    batches = {}
    for k, key in (("pair_kernels", 13), ("bsp_kernels", 14)):                 # the switch applies to batches created after it
        if key: _lib.check(lib.mh_debug_set(key, 1))
        try:
            batches[k] = A.ArticBatch(slab("spheres"), q, qd)
        finally:
            if key: _lib.check(lib.mh_debug_set(key, 0))
    stream = torch.cuda.current_stream(dev).cuda_stream
    times = {k: [] for k in batches}
    out = {}
    for rep in range(a.reps + 1):                 # rep 0: warm-up of both (and their outcome)
        for k, ab in batches.items():
            ab.upload(q, qd, S.new_aux(B))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ab.step(dt, n, stream=stream)
            e1.record(); e1.synchronize()
            if rep:
                times[k].append(e0.elapsed_time(e1))
            else:
                aux = ab.download()[2]
                ws = float(aux["steps"].sum())
                out[k] = dict(finished=int((aux["steps"] == n).sum()), unsupported=int(((aux["status"] & S.MH_WORLD_UNSUPPORTED) != 0).sum()),
                              solves_per_world_step=float(aux["lcp_solves"].sum()) / ws, rows_per_solve=float(aux["lcp_rows"].sum()) / max(1.0, float(aux["lcp_solves"].sum())),
                              mini_steps_per_step=float(aux["mini_steps"].sum()) / ws)
    for ab in batches.values():
        ab.close()
    res = {"bench": "artic_boxsphere", "B": B, "steps": n, "dt": dt, "reps": a.reps, "variants": {}}
    for k, v in times.items():
        med = float(np.median(v))
        res["variants"][k] = dict(ms=dict(median=med, min=float(min(v)), max=float(max(v))), world_steps_per_s=B * n / (med * 1e-3), **out[k])
    res["ratio_bsp_to_pair_kernels"] = res["variants"]["bsp_kernels"]["ms"]["median"] / res["variants"]["pair_kernels"]["ms"]["median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
