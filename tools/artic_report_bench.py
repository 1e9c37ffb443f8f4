"""The contact report in the articulated step (include/moby_hip_artic.h, "Contact report"; mh_artic_rp.hip), by the method of
tools/world_report_bench.py: B worlds, every repetition from the same uploaded state, warm-up steps in one launch, then a timed window of ONE launch
of --steps steps, the device synchronised before the clock stops.  The scene is mixed_all (tests/artic_boxsphere_ref.py: a floating box with an arm,
a pendulum on a second root, a static box; a sphere pair, two box-sphere pairs and the plane contacts of a sphere and a box in one list), its B states
aimed with the box-sphere reference as the tests aim theirs.  Three legs that alternate, warm:
  bsp      the box-sphere kernels (mh_artic_bsp.hip): what such a batch runs without the report -- the baseline
  rp_null  the report kernels with a NULL report (mh_debug_set(19, 1)): what the accumulators, the slot table and the fold's test cost a caller who
           asks for nothing
  rp       the report kernels writing the report (B x steps x 7 x 8 doubles, the same device array in every repetition)
Medians with min and max of the repetitions, the ratios to bsp and whether the spreads overlap.  Prints one JSON line.
usage: python tools/artic_report_bench.py [--reps 5] [--B 4096] [--steps 100] [--warmup 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from moby_amd import _lib, artic as A, scene as S  # noqa: E402
from tests import artic_boxsphere_ref as BS  # noqa: E402


def window(ab, q0, qd0, aux0, dt, wu, n, stream, report):
    ab.upload(q0, qd0, aux0)
    if wu > 0:
        ab.step(dt, wu, stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ab.step(dt, n, stream, report=report)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def work_of(ab):
    _, _, aux = ab.download()
    return {"lcp_rows": int(aux["lcp_rows"].astype(np.int64).sum()), "mini_steps": int(aux["mini_steps"].astype(np.int64).sum()),
            "worlds_with_errors": int(((aux["status"] & ~S.MH_WORLD_IMPACT_TOL) != 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert a.reps >= 5, "at least five repetitions"
    lib = _lib.load()
    B, n, wu = a.B, a.steps, a.warmup
    stream = torch.cuda.current_stream().cuda_stream
    m, sampler, dt = BS.mixed_all()
    q0, qd0 = BS.aim(BS.build_boxsphere_ref(), m, sampler, B, len("mixed_all"))
    aux0 = S.new_aux(B)
    out = {"bench": "artic_report", "scene": "mixed_all", "B": B, "steps": n, "warmup": wu, "dt": dt, "reps": a.reps}
    abs_ = {}
    try:
        abs_["bsp"] = A.ArticBatch(m, q0, qd0, aux0)
        try:
            _lib.check(lib.mh_debug_set(19, 1))
            abs_["rp_null"] = A.ArticBatch(m, q0, qd0, aux0)
        finally:
            _lib.check(lib.mh_debug_set(19, 0))
        abs_["rp"] = A.ArticBatch(m, q0, qd0, aux0, report=True)
        rows = torch.zeros((B, n, abs_["rp"].report_slots, A.REPORT_PAIR), dtype=torch.float64, device="cuda")
        reports = {"bsp": None, "rp_null": None, "rp": rows}
        out["report_bytes_per_world_step"] = abs_["rp"].report_slots * A.REPORT_PAIR * 8
        times = {k: [] for k in abs_}
        for rep in range(a.reps + 1):                              # the first pass loads the code objects
            for k, ab in abs_.items():
                ms = window(ab, q0, qd0, aux0, dt, wu, n, stream, reports[k])
                if rep:
                    times[k].append(ms)
        med = {k: float(np.median(v)) for k, v in times.items()}
        over = lambda x, y: bool(min(times[x]) <= max(times[y]) and min(times[y]) <= max(times[x]))
        out["ms"] = {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()}
        out["world_steps_per_sec"] = {k: B * n / (med[k] * 1e-3) for k in times}
        out["ratio_to_bsp"] = {k: med[k] / med["bsp"] for k in ("rp_null", "rp")}
        out["spreads_overlap_bsp"] = {k: over(k, "bsp") for k in ("rp_null", "rp")}
        out["work_after_warmup_and_window"] = {k: work_of(ab) for k, ab in abs_.items()}
        out["contacts_in_window"] = float(rows[..., 0].sum().item())
        out["mean_link_impulse_up"] = float(A.link_impulses(rows, m)[..., 1].mean().item())
    finally:
        for ab in abs_.values():
            ab.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
