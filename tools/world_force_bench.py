"""Cost of forces in the world step (include/moby_hip.h, mh_world_batch_set_forces / mh_world_batch_step_wrench) on the headline workload, by the
headline's method: sphere-stack x 4096 from t = 0, 5 warm-up steps (one launch), then a timed window of 20 steps (one launch), the device
synchronised before the clock stops.  Variants, alternating within one call, each repetition from the same uploaded state:
  plain          the plain kernel, no forces (compare with bench.py's headline of the same visit)
  drag           the forced kernel with Stokes drag and damping stored
  drag_wrench    ... and a wrench schedule with one row per step (forces +-2 N, torques +-0.4 N m)
  drag_push      ... the same schedule without its torques (spheres that spin in contact cost conservative advancement sub-steps: physics, not the kernel path)
Prints one JSON line: per variant the median and the spread (min, max) of the window in ms, the ratios of the medians to `plain`, the work done
(LCP rows, mini-steps) and the runtime's occupancy query for the plain and the forced kernel.
usage: python tools/world_force_bench.py [--reps 7] [--B 4096] [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from moby_amd import _lib, scene as S  # noqa: E402
from moby_amd.world import WorldBatchDevice  # noqa: E402

DT = 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert a.reps >= 5, "at least five repetitions"
    lib = _lib.load()
    B, n, wu = a.B, a.steps, a.warmup
    sc = S.sphere_stack_scene()
    st0 = S.sphere_stack_state_range(0, B)
    aux0 = S.new_aux(B)
    forces = S.make_forces(sc.nb, stokes=(0.3, 0.05), damping=(0.2, 0.02, 0.1, 0.01))
    rng = np.random.default_rng(1)
    w = np.concatenate([rng.uniform(-2.0, 2.0, (wu + n, B, sc.nb, 3)), rng.uniform(-0.4, 0.4, (wu + n, B, sc.nb, 3))], axis=3)
    w_dev = torch.from_numpy(w).cuda()
    push = w.copy(); push[..., 3:] = 0.0
    push_dev = torch.from_numpy(push).cuda()
    variants = {"plain": (None, None), "drag": (forces, None), "drag_wrench": (forces, w_dev), "drag_push": (forces, push_dev)}
    stream = torch.cuda.current_stream().cuda_stream
    wb = WorldBatchDevice(sc, st0)
    occupancy = {}
    times = {k: [] for k in variants}
    work = {}
    for rep in range(a.reps + 1):                 # rep 0: every variant once untimed (code objects loaded, outcome recorded)
        for k, (f, wr) in variants.items():
            wb.set_forces(f)
            occupancy["plain" if f is None else "forced"] = wb.occupancy()
            _lib.check(lib.mh_world_batch_upload(wb.handle, st0.ctypes.data, aux0.ctypes.data))
            if wu > 0:
                wb.step(DT, wu, stream, wrench=None if wr is None else wr[:wu].contiguous())
            torch.cuda.synchronize()
            wt = None if wr is None else wr[wu:].contiguous()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            wb.step(DT, n, stream, wrench=wt)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if rep:
                times[k].append(ms)
            else:
                _, aux = wb.download()
                work[k] = {"lcp_rows": int(aux["lcp_rows"].astype(np.int64).sum()), "mini_steps": int(aux["mini_steps"].astype(np.int64).sum()),
                           "worlds_with_errors": int(((aux["status"] & ~S.MH_WORLD_IMPACT_TOL) != 0).sum())}
    wb.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({"bench": "world_forces", "B": B, "steps": n, "warmup": wu, "dt": DT, "reps": a.reps,
                      "ms": {k: {"median": med[k], "min": float(min(v)), "max": float(max(v))} for k, v in times.items()},
                      "world_steps_per_sec": {k: B * n / (med[k] * 1e-3) for k in times},
                      "ratio_to_plain": {k: med[k] / med["plain"] for k in times if k != "plain"},
                      "work_after_warmup_and_window": work, "workgroups_per_cu": occupancy}))


if __name__ == "__main__":
    main()
