"""Static bodies among the free ones in the world step (include/moby_hip.h, "Static bodies"; mh_world_large_st*.hip), by the headline's method: B worlds
from t = 0, warm-up steps in one launch, then a timed window in one launch, the device synchronised before the clock stops, every repetition from
the same uploaded state.  Two measurements:
  ab             a ground-only mixed scene (a crate, a ball, the plane; tests/world_boxsphere_ref.py face_batch), the same batch through the box-sphere
                 build -- the object it launches by default -- and, under mh_debug_set(16, 1), through the statics build; alternating, warm, median
                 of the repetitions with min and max.  Default routing never sends such a scene through the new objects: the figures only describe
                 the cost of reading the plane from the statics table.
  corner9        six balls, a floor, a wall and a table box (tests/world_statics_ref.py corner9_batch: nine objects, all 36 pair slots) x B:
                 world-steps/s
Prints one JSON line: medians and spreads in ms, world-steps/s, the ratio st / bsp, whether the two spreads overlap, the work done and the runtime's
occupancy query.
usage: python tools/world_statics_bench.py [--reps 5] [--B 4096] [--steps 20] [--warmup 5]"""
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
from tests.world_boxsphere_ref import face_batch  # noqa: E402
from tests.world_statics_ref import corner9_batch  # noqa: E402

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
    out = {"bench": "world_statics", "B": B, "steps": n, "warmup": wu, "dt": DT, "reps": a.reps}

    sc, st0 = face_batch(B)
    wbs = {}
    try:
        for name, key in (("bsp", 0), ("st", 1)):
            _lib.check(lib.mh_debug_set(16, key))
            wbs[name] = WorldBatchDevice(sc, st0)
    finally:
        _lib.check(lib.mh_debug_set(16, 0))
    try:
        times = {k: [] for k in wbs}
        for rep in range(a.reps + 1):                              # the first pass loads the code objects
            for k, wb in wbs.items():
                ms = window(lib, wb, st0, aux0, wu, n, stream)
                if rep:
                    times[k].append(ms)
        med = {k: float(np.median(v)) for k, v in times.items()}
        out["ab"] = {"ms": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
                     "world_steps_per_sec": {k: B * n / (med[k] * 1e-3) for k in times}, "ratio_st_to_bsp": med["st"] / med["bsp"],
                     "spreads_overlap": bool(min(times["st"]) <= max(times["bsp"]) and min(times["bsp"]) <= max(times["st"])),
                     "work_after_warmup_and_window": {k: work_of(wb) for k, wb in wbs.items()}, "workgroups_per_cu": {k: wb.occupancy() for k, wb in wbs.items()}}
    finally:
        for wb in wbs.values():
            wb.close()

    sc, stt, st0 = corner9_batch(B)
    wb = WorldBatchDevice(sc, st0, statics=stt)
    try:
        t = [window(lib, wb, st0, aux0, wu, n, stream) for _ in range(a.reps + 1)][1:]
        out["corner9"] = {"ms": {"median": float(np.median(t)), "min": min(t), "max": max(t)}, "world_steps_per_sec": B * n / (float(np.median(t)) * 1e-3),
                          "work_after_warmup_and_window": work_of(wb), "workgroups_per_cu": wb.occupancy()}
    finally:
        wb.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
