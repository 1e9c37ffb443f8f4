"""Box-sphere contacts between free bodies in the world step (include/moby_hip.h, "Box-sphere pairs"; mh_world_large_bsp*.hip), by the headline's
method: B worlds from t = 0, warm-up steps in one launch, then a timed window in one launch, the device synchronised before the clock stops, every
repetition from the same uploaded state.  Two measurements:
  full           the full image of tests/world_boxsphere_ref.py (4 boxes + 4 spheres + plane, all 16 box-sphere pairs enabled) x B: world-steps/s
  ab             a mixed scene with the box-sphere pairs DISABLED (two spheres + a box + plane), the same batch through the plain large kernel and,
                 under mh_debug_set(15, 1), through the box-sphere build; alternating, warm, median of the repetitions.  Default routing never
                 sends such a scene through the new objects: the ratio only describes the cost of the extra branches.
Prints one JSON line: medians and spreads in ms, world-steps/s, the ratio bsp / plain, the work done and the runtime's occupancy query.
usage: python tools/world_boxsphere_bench.py [--reps 5] [--B 4096] [--steps 20] [--warmup 5]"""
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
from tests.world_boxsphere_ref import disabled_mixed_batch, full_batch  # noqa: E402

DT = 1e-3


def window(lib, wb, st0, aux0, wu, n, stream):
    _lib.check(lib.mh_world_batch_upload(wb.handle, st0.ctypes.data, aux0.ctypes.data))
    if wu > 0:
        wb.step(DT, wu, stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    wb.step(DT, n, stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def work_of(wb):
    _, aux = wb.download()
    return {"lcp_rows": int(aux["lcp_rows"].astype(np.int64).sum()), "mini_steps": int(aux["mini_steps"].astype(np.int64).sum()),
            "worlds_with_errors": int(((aux["status"] & ~S.MH_WORLD_IMPACT_TOL) != 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert a.reps >= 5, "at least five repetitions"
    lib = _lib.load()
    B, n, wu = a.B, a.steps, a.warmup
    stream = torch.cuda.current_stream().cuda_stream
    aux0 = S.new_aux(B)
    out = {"bench": "world_boxsphere", "B": B, "steps": n, "warmup": wu, "dt": DT, "reps": a.reps}

    sc, st0 = full_batch(B)
    wb = WorldBatchDevice(sc, st0)
    try:
        t = [window(lib, wb, st0, aux0, wu, n, stream) for _ in range(a.reps + 1)][1:]      # the first pass loads the code object
        out["full"] = {"ms": {"median": float(np.median(t)), "min": min(t), "max": max(t)}, "world_steps_per_sec": B * n / (float(np.median(t)) * 1e-3),
                       "work_after_warmup_and_window": work_of(wb), "workgroups_per_cu": wb.occupancy()}
    finally:
        wb.close()

    sc, st0 = disabled_mixed_batch(B)
    wbs = {}
    try:
        for name, key in (("plain", 0), ("bsp", 1)):
            _lib.check(lib.mh_debug_set(15, key))
            wbs[name] = WorldBatchDevice(sc, st0)
    finally:
        _lib.check(lib.mh_debug_set(15, 0))
    try:
        times = {k: [] for k in wbs}
        for rep in range(a.reps + 1):
            for k, wb in wbs.items():
                ms = window(lib, wb, st0, aux0, wu, n, stream)
                if rep:
                    times[k].append(ms)
        med = {k: float(np.median(v)) for k, v in times.items()}
        out["ab"] = {"ms": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
                     "world_steps_per_sec": {k: B * n / (med[k] * 1e-3) for k in times}, "ratio_bsp_to_plain": med["bsp"] / med["plain"],
                     "work_after_warmup_and_window": {k: work_of(wb) for k, wb in wbs.items()}, "workgroups_per_cu": {k: wb.occupancy() for k, wb in wbs.items()}}
    finally:
        for wb in wbs.values():
            wb.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
