"""Link wrenches in the articulated step (include/moby_hip_artic.h, "Link wrenches"; mh_artic_wr.hip), by the method of tools/artic_params_bench.py:
B worlds, every repetition from the same uploaded state, warm-up steps in one launch, then a timed window of ONE launch of --steps steps, the device
synchronised before the clock stops; the legs alternate, warm.  mixed_all x --B (tests/artic_boxsphere_ref.py; states aimed with the box-sphere
reference), batches with B images equal to the model and a NULL report:
    pw         the per-world-parameters kernels (mh_artic_pw.hip) -- the baseline, the path such a batch took before link wrenches existed
    wr_null    the link-wrench kernels under mh_debug_set(21, 1) with a NULL wrench -- what carrying the switch costs
    wr_sched   a wrench batch with a schedule of one row per step on every link (rows = --steps), model axes
    wr_damp    a wrench batch with damping on every link
Medians with min and max of the repetitions, the ratios to pw and whether the spreads overlap.  Prints one JSON line.
usage: python tools/artic_wrench_bench.py [--reps 5] [--B 4096] [--steps 100] [--warmup 10]"""
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


def window(ab, wr, q0, qd0, aux0, dt, wu, n, stream):
    ab.upload(q0, qd0, aux0)
    if wu > 0:
        ab.step(dt, wu, stream, wrench=wr)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ab.step(dt, n, stream, wrench=wr)
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
    n, wu, B = a.steps, a.warmup, a.B
    assert wu <= n, "the schedule has one row per step of the window"
    stream = torch.cuda.current_stream().cuda_stream
    m, sampler, dt = BS.mixed_all()
    q0, qd0 = BS.aim(BS.build_boxsphere_ref(), m, sampler, B, len("mixed_all"))
    aux0 = S.new_aux(B)
    rng = np.random.default_rng(7)
    dev = torch.device("cuda")
    T = lambda x: torch.from_numpy(x).to(dev)
    body = np.zeros(m.nj); body[5:] = 1.0                               # the base link and the links it carries; the virtual links take nothing
    sched = A.LinkWrench(w=T(rng.uniform(-1.0, 1.0, (n, B, m.nj, 6)) * body[:, None]))
    damp = A.LinkWrench(kl=T(rng.uniform(0.0, 0.5, (B, m.nj)) * body), ka=T(rng.uniform(0.0, 0.05, (B, m.nj)) * body),
                        klsq=T(rng.uniform(0.0, 0.2, (B, m.nj)) * body), kasq=T(rng.uniform(0.0, 0.02, (B, m.nj)) * body))
    batches = {}
    try:
        batches["pw"] = (A.ArticBatch(m, q0, qd0, aux0, report=True, params=True), None)
        try:
            _lib.check(lib.mh_debug_set(21, 1))
            batches["wr_null"] = (A.ArticBatch(m, q0, qd0, aux0, report=True, params=True), None)
        finally:
            _lib.check(lib.mh_debug_set(21, 0))
        batches["wr_sched"] = (A.ArticBatch(m, q0, qd0, aux0, report=True, wrench=True), sched)
        batches["wr_damp"] = (A.ArticBatch(m, q0, qd0, aux0, report=True, wrench=True), damp)
        times = {k: [] for k in batches}
        for rep in range(a.reps + 1):                                # the first pass loads the code objects
            for k, (ab, wr) in batches.items():
                ms = window(ab, wr, q0, qd0, aux0, dt, wu, n, stream)
                if rep:
                    times[k].append(ms)
        med = {k: float(np.median(v)) for k, v in times.items()}
        over = lambda x, y: bool(min(times[x]) <= max(times[y]) and min(times[y]) <= max(times[x]))
        others = [k for k in batches if k != "pw"]
        out = {"bench": "artic_wrench", "steps": n, "warmup": wu, "reps": a.reps, "B": B, "dt": dt,
               "ms": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
               "world_steps_per_sec": {k: B * n / (med[k] * 1e-3) for k in times},
               "ratio_to_pw": {k: med[k] / med["pw"] for k in others}, "spreads_overlap_pw": {k: over(k, "pw") for k in others},
               "work_after_warmup_and_window": {k: work_of(ab) for k, (ab, _) in batches.items()}}
    finally:
        for ab, _ in batches.values():
            ab.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
