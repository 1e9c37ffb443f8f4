"""Per-world parameters in the world step (include/moby_hip.h, "Per-world parameters"; mh_world_large_pw*.hip), by the headline's method: B worlds from
t = 0, warm-up steps in one launch, then a timed window, the device synchronised before the clock stops, every repetition from the same uploaded state.
The scene is corner9 (tests/world_statics_ref.py corner9_batch: six balls, a floor, a wall and a table box -- nine objects, all 36 pair slots), three legs:
  st        the statics build, the object such a batch launches by default
  pw_same   the per-world-parameters build under mh_debug_set(17, 1): every record equal to the scene, the same work -- the cost of the launch's read
  pw_varied the per-world-parameters build with friction and wall position of its own in every world (other work: reported, not compared)
st and pw_same alternate, warm; each leg runs twice: `long` = the window is ONE launch of --steps steps, `short` = the window is --steps launches of one
step each, where the read of the records at every launch shows most.  Medians with min and max of the repetitions, the ratio pw_same / st and whether
the two spreads overlap.
Prints one JSON line.
usage: python tools/world_params_bench.py [--reps 5] [--B 4096] [--steps 20] [--warmup 5]"""
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
from tests.world_statics_ref import corner9_batch  # noqa: E402

DT = 1e-3


def window(lib, wb, st0, aux0, wu, n, stream, short):
    _lib.check(lib.mh_world_batch_upload(wb.handle, st0.ctypes.data, aux0.ctypes.data))
    if wu > 0:
        wb.step(DT, wu, stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if short:
        for _ in range(n):
            wb.step(DT, 1, stream)
    else:
        wb.step(DT, n, stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def work_of(wb):
    _, aux = wb.download()
    return {"lcp_rows": int(aux["lcp_rows"].astype(np.int64).sum()), "mini_steps": int(aux["mini_steps"].astype(np.int64).sum()),
            "worlds_with_errors": int(((aux["status"] & ~S.MH_WORLD_IMPACT_TOL) != 0).sum())}


def varied(sc, stt, B):
    """friction of every pair slot x U(0.5, 1.5) and the wall 0-5 mm back along its normal, per world (world 0 keeps the scene)"""
    p = S.make_params(sc, stt, B)
    r = np.random.RandomState(17)
    p["cp_mu_coulomb"][1:, :] *= r.uniform(0.5, 1.5, (B - 1, S.MH_MAX_PAIRS))
    p["st_o"][1:, 1] -= p["st_R"][1:, 1].reshape(B - 1, 3, 3)[:, :, 1] * r.uniform(0.0, 5e-3, (B - 1, 1))
    return p


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
    out = {"bench": "world_params", "scene": "corner9", "B": B, "steps": n, "warmup": wu, "dt": DT, "reps": a.reps}
    sc, stt, st0 = corner9_batch(B)
    wbs = {}
    try:
        wbs["st"] = WorldBatchDevice(sc, st0, statics=stt)
        try:
            _lib.check(lib.mh_debug_set(17, 1))
            wbs["pw_same"] = WorldBatchDevice(sc, st0, statics=stt)
        finally:
            _lib.check(lib.mh_debug_set(17, 0))
        wbs["pw_varied"] = WorldBatchDevice(sc, st0, statics=stt, params=varied(sc, stt, B))
        out["workgroups_per_cu"] = {k: wb.occupancy() for k, wb in wbs.items()}
        for mode, short in (("long", False), ("short", True)):
            times = {k: [] for k in wbs}
            for rep in range(a.reps + 1):                              # the first pass loads the code objects
                for k, wb in wbs.items():
                    ms = window(lib, wb, st0, aux0, wu, n, stream, short)
                    if rep:
                        times[k].append(ms)
            med = {k: float(np.median(v)) for k, v in times.items()}
            out[mode] = {"launches_per_window": n if short else 1,
                         "ms": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
                         "world_steps_per_sec": {k: B * n / (med[k] * 1e-3) for k in times}, "ratio_pw_same_to_st": med["pw_same"] / med["st"],
                         "spreads_overlap": bool(min(times["pw_same"]) <= max(times["st"]) and min(times["st"]) <= max(times["pw_same"])),
                         "work_after_warmup_and_window": {k: work_of(wb) for k, wb in wbs.items()}}
    finally:
        for wb in wbs.values():
            wb.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
