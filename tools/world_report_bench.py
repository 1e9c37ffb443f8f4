"""The contact report in the world step (include/moby_hip.h, "Contact report"; mh_world_large_rp*.hip), by the method of tools/world_params_bench.py: B
worlds from t = 0, warm-up steps in one launch, then a timed window of ONE launch of --steps steps, the device synchronised before the clock stops, every
repetition from the same uploaded state.  The scene is corner9 (tests/world_statics_ref.py corner9_batch: nine objects, all 36 pair slots), every record
equal to the scene, three legs that alternate, warm:
  pw       the per-world-parameters build (mh_debug_set(17, 1)): the baseline
  rp_null  the report build with a NULL report (mh_debug_set(18, 1) on top): what the accumulators and the fold's test cost a caller who asks for nothing
  rp       the report build writing the report (B x steps x 36 x 8 doubles, the same device array in every repetition)
Medians with min and max of the repetitions, the ratios to pw and whether the spreads overlap.  Prints one JSON line.
usage: python tools/world_report_bench.py [--reps 5] [--B 4096] [--steps 20] [--warmup 5]"""
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
from moby_amd.world import WorldBatchDevice, body_impulses  # noqa: E402
from tests.world_statics_ref import corner9_batch  # noqa: E402

DT = 1e-3


def window(lib, wb, st0, aux0, wu, n, stream, report):
    _lib.check(lib.mh_world_batch_upload(wb.handle, st0.ctypes.data, aux0.ctypes.data))
    if wu > 0:
        wb.step(DT, wu, stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    wb.step(DT, n, stream, report=report)
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
    out = {"bench": "world_report", "scene": "corner9", "B": B, "steps": n, "warmup": wu, "dt": DT, "reps": a.reps}
    sc, stt, st0 = corner9_batch(B)
    wbs = {}
    try:
        try:
            _lib.check(lib.mh_debug_set(17, 1))
            wbs["pw"] = WorldBatchDevice(sc, st0, statics=stt)
            _lib.check(lib.mh_debug_set(18, 1))
            wbs["rp_null"] = WorldBatchDevice(sc, st0, statics=stt)
        finally:
            _lib.check(lib.mh_debug_set(18, 0))
            _lib.check(lib.mh_debug_set(17, 0))
        wbs["rp"] = WorldBatchDevice(sc, st0, statics=stt, report=True)
        rows = torch.zeros((B, n, wbs["rp"].npt, 8), dtype=torch.float64, device="cuda")
        reports = {"pw": None, "rp_null": None, "rp": rows}
        out["workgroups_per_cu"] = {k: wb.occupancy() for k, wb in wbs.items()}
        out["report_bytes_per_world_step"] = wbs["rp"].npt * 8 * 8
        times = {k: [] for k in wbs}
        for rep in range(a.reps + 1):                              # the first pass loads the code objects
            for k, wb in wbs.items():
                ms = window(lib, wb, st0, aux0, wu, n, stream, reports[k])
                if rep:
                    times[k].append(ms)
        med = {k: float(np.median(v)) for k, v in times.items()}
        over = lambda x, y: bool(min(times[x]) <= max(times[y]) and min(times[y]) <= max(times[x]))
        out["ms"] = {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()}
        out["world_steps_per_sec"] = {k: B * n / (med[k] * 1e-3) for k in times}
        out["ratio_to_pw"] = {k: med[k] / med["pw"] for k in ("rp_null", "rp")}
        out["spreads_overlap_pw"] = {k: over(k, "pw") for k in ("rp_null", "rp")}
        out["work_after_warmup_and_window"] = {k: work_of(wb) for k, wb in wbs.items()}
        ntot = sc.nb + sc.has_ground + stt.n
        out["contacts_in_window"] = float(rows[..., 0].sum().item())
        out["mean_body_impulse_up"] = float(body_impulses(rows, sc.nb, ntot)[..., 1].mean().item())
    finally:
        for wb in wbs.values():
            wb.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
