"""Per-world parameters in the articulated step (include/moby_hip_artic.h, "Per-world parameters"; mh_artic_pw.hip), by the method of
tools/artic_report_bench.py: B worlds, every repetition from the same uploaded state, warm-up steps in one launch, then a timed window of ONE launch
of --steps steps, the device synchronised before the clock stops; the legs of a scene alternate, warm.  Two scenes:
  mixed_all x --B (tests/artic_boxsphere_ref.py; states aimed with the box-sphere reference), report batches with a NULL report:
    rp         the report kernels (mh_artic_rp.hip) over the one shared image -- the baseline
    pw_equal   the per-world-parameters kernels under mh_debug_set(20, 1): B images, all the model's -- what reading the world's own image costs
    pw_varied  a params batch whose records vary (tests/artic_params_ref.vary, mu >= 100 everywhere): other work per world, so no A/B of the kernel
  ur10 x --B-arm (tests/scenes/ten_joint_arm.sdf, the states of bench.py's config-5 leg), no geometry:
    plain      the plain kernels (mh_artic.hip, k_artic_step_w4) -- the baseline
    pw_equal   a params batch with equal records: the contact family's LDS image and empty contact lists against the plain kernels' occupancy
Medians with min and max of the repetitions, the ratios to the scene's baseline and whether the spreads overlap.  Prints one JSON line.
usage: python tools/artic_params_bench.py [--reps 5] [--B 4096] [--B-arm 8192] [--steps 100] [--warmup 10]"""
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
from tests import artic_params_ref as P  # noqa: E402
from tests.test_artic_gpu import ur10_states  # noqa: E402


def window(ab, q0, qd0, aux0, dt, wu, n, stream):
    ab.upload(q0, qd0, aux0)
    if wu > 0:
        ab.step(dt, wu, stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ab.step(dt, n, stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def work_of(ab):
    _, _, aux = ab.download()
    return {"lcp_rows": int(aux["lcp_rows"].astype(np.int64).sum()), "mini_steps": int(aux["mini_steps"].astype(np.int64).sum()),
            "worlds_with_errors": int(((aux["status"] & ~S.MH_WORLD_IMPACT_TOL) != 0).sum())}


def legs(batches, base, q0, qd0, aux0, dt, wu, n, reps, stream):
    """the alternating, warm repetitions of one scene's batches -> its part of the result"""
    times = {k: [] for k in batches}
    for rep in range(reps + 1):                                  # the first pass loads the code objects
        for k, ab in batches.items():
            ms = window(ab, q0, qd0, aux0, dt, wu, n, stream)
            if rep:
                times[k].append(ms)
    med = {k: float(np.median(v)) for k, v in times.items()}
    over = lambda x, y: bool(min(times[x]) <= max(times[y]) and min(times[y]) <= max(times[x]))
    others = [k for k in batches if k != base]
    return {"ms": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
            "world_steps_per_sec": {k: q0.shape[0] * n / (med[k] * 1e-3) for k in times},
            "ratio_to_" + base: {k: med[k] / med[base] for k in others}, "spreads_overlap_" + base: {k: over(k, base) for k in others},
            "work_after_warmup_and_window": {k: work_of(ab) for k, ab in batches.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--B-arm", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert a.reps >= 5, "at least five repetitions"
    lib = _lib.load()
    n, wu = a.steps, a.warmup
    stream = torch.cuda.current_stream().cuda_stream
    out = {"bench": "artic_params", "steps": n, "warmup": wu, "reps": a.reps}
    # ---- mixed_all
    B = a.B
    m, sampler, dt = BS.mixed_all()
    q0, qd0 = BS.aim(BS.build_boxsphere_ref(), m, sampler, B, len("mixed_all"))
    aux0 = S.new_aux(B)
    batches = {}
    try:
        batches["rp"] = A.ArticBatch(m, q0, qd0, aux0, report=True)
        try:
            _lib.check(lib.mh_debug_set(20, 1))
            batches["pw_equal"] = A.ArticBatch(m, q0, qd0, aux0, report=True)
        finally:
            _lib.check(lib.mh_debug_set(20, 0))
        batches["pw_varied"] = A.ArticBatch(m, q0, qd0, aux0, report=True, params=P.vary(m, B, 1, [100.0] * B))
        out["mixed_all"] = dict(B=B, dt=dt, **legs(batches, "rp", q0, qd0, aux0, dt, wu, n, a.reps, stream))
    finally:
        for ab in batches.values():
            ab.close()
    # ---- the arm of the config-5 leg (bench.py: the same model and states)
    B = a.B_arm
    m, _, _ = A.load_sdf(os.path.join(ROOT, "tests", "scenes", "ten_joint_arm.sdf"))
    q0, qd0 = ur10_states(m, B)
    aux0 = S.new_aux(B)
    batches = {}
    try:
        batches["plain"] = A.ArticBatch(m, q0, qd0, aux0)
        batches["pw_equal"] = A.ArticBatch(m, q0, qd0, aux0, params=True)
        out["ur10"] = dict(B=B, dt=5e-4, **legs(batches, "plain", q0, qd0, aux0, 5e-4, wu, n, a.reps, stream))
    finally:
        for ab in batches.values():
            ab.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
