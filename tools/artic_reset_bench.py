"""Episodes on the device (include/moby_hip_artic.h, "Episodes on the device"; mh_artic_reset.hip) in a control loop, by the method of
tools/artic_params_bench.py: B worlds, every repetition from the same uploaded state, the device synchronised before the clock stops; the legs of a
scene alternate, warm.  The timed window is a WHOLE loop of --control control steps, each one launch of --steps steps, after each of which 1/16 of the
worlds (a fixed pseudo-random sixteenth per control step, the same for every leg) start a new episode from their start state:
  bare       the launches alone, no world restarts -- what the loop cannot go below
  host       the only route before mh_artic_batch_reset_dev: download, the edit on the host, upload of the whole batch
  reset_dev  ArticBatch.reset on the stepping stream, the mask and the start states resident on the device; one synchronisation at the loop's end
and, per call, link_poses() (synchronise, allocate, launch, copy to the host, free) against link_poses_into (one launch into a resident tensor; the
calls are timed in runs of --pose-calls with one synchronisation at the end).  Two scenes: mixed_all x --B (tests/artic_boxsphere_ref.py, the
box-sphere kernels) and ur10 x --B-arm (tests/scenes/ten_joint_arm.sdf, the plain kernels).  Medians with min and max of the repetitions.
--root DIR imports moby_amd and tests from another tree -- an older build of the library, to measure `bare` and `host` on it with this same tool;
the legs that need entry points the library lacks are left out and named under "missing".  Prints one JSON line; every loop's time goes to stderr
as it ends (worlds of mixed_all that have come to rest step far slower than falling ones, and a launch lasts as long as its slowest world: one
mixed_all loop takes 44-50 s on an MI355X, an invocation with it a quarter of an hour; --scenes ur10 leaves it out).  The project's summary is the
median (min-max) of each invocation's line; two invocations are appended to profiles/artic_reset_bench.jsonl and both are quoted.
usage: python tools/artic_reset_bench.py [--root DIR] [--scenes ur10,mixed_all] [--reps 5] [--B 4096] [--B-arm 8192] [--control 50] [--steps 10] [--pose-calls 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--B", type=int, default=4096)
ap.add_argument("--B-arm", type=int, default=8192)
ap.add_argument("--control", type=int, default=50)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--pose-calls", type=int, default=20)
ap.add_argument("--scenes", default="ur10,mixed_all", help="which scenes to run, in this order: a mixed_all invocation takes a quarter of an hour (see above)")
ARGS = ap.parse_args()
ROOT = os.path.abspath(ARGS.root)
sys.path.insert(0, ROOT)
from moby_amd import _lib, artic as A, scene as S  # noqa: E402
from tests import artic_boxsphere_ref as BS  # noqa: E402
from tests.test_artic_gpu import ur10_states  # noqa: E402


def loop(ab, leg, q0, qd0, aux0, dt, n, masks, dev, stream):
    """one timed loop of len(masks) control steps -> ms"""
    fresh = S.new_aux(1)[0]
    ab.upload(q0, qd0, aux0)
    ab.step(dt, n, stream)                                        # warm: this shape's launch, before the clock
    ab.upload(q0, qd0, aux0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(len(masks)):
        ab.step(dt, n, stream)
        if leg == "host":
            q, qd, aux = ab.download()
            w = masks[k] != 0
            q[w] = q0[w]; qd[w] = qd0[w]; aux[w] = fresh
            ab.upload(q, qd, aux)
        elif leg == "reset_dev":
            ab.reset(mask=dev["masks"][k], q=dev["q0"], qd=dev["qd0"], stream=stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def poses(ab, into, calls, t, stream):
    """`calls` link-pose calls -> ms per call"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        if into:
            ab.link_poses_into(t, stream=stream)
        else:
            ab.link_poses()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def stats(times):
    return {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()}


def scene(name, m, q0, qd0, dt, has_new, a, stream):
    B = q0.shape[0]
    aux0 = S.new_aux(B)
    rng = np.random.default_rng(16)
    masks = np.zeros((a.control, B), dtype=np.int32)
    for k in range(a.control):
        masks[k, rng.choice(B, B // 16, replace=False)] = 1
    ab = A.ArticBatch(m, q0, qd0, aux0)
    try:
        d = ab._device()
        dev = {"masks": torch.from_numpy(masks).to(d), "q0": torch.from_numpy(q0).to(d), "qd0": torch.from_numpy(qd0).to(d)}
        legs = ["bare", "host"] + (["reset_dev"] if has_new else [])
        times = {k: [] for k in legs}
        for rep in range(a.reps + 1):                             # the first pass loads the code objects
            for leg in legs:
                ms = loop(ab, leg, q0, qd0, aux0, dt, a.steps, masks, dev, stream)
                print("%s B=%d pass %d %s: %.1f ms" % (name, B, rep, leg, ms), file=sys.stderr, flush=True)    # (a loop of old worlds is slow: say where the time goes)
                if rep:
                    times[leg].append(ms)
        _, _, aux = ab.download()                                  # (after a reset_dev loop when the library has it, else after a host loop)
        out = {"B": B, "dt": dt, "loop_ms": stats(times), "resets_per_control_step": B // 16,
               "after_last_loop": {"steps_min": int(aux["steps"].min()), "steps_max": int(aux["steps"].max()),
                                   "worlds_with_errors": int(((aux["status"] & ~S.MH_WORLD_IMPACT_TOL) != 0).sum())}}
        med = {k: float(np.median(v)) for k, v in times.items()}
        out["ratio_to_bare"] = {k: med[k] / med["bare"] for k in legs if k != "bare"}
        kinds = ["link_poses"] + (["link_poses_into"] if has_new else [])
        t = torch.empty((B, m.nj, 12), dtype=torch.float64, device=d)
        pt = {k: [] for k in kinds}
        for rep in range(a.reps + 1):
            for k in kinds:
                ms = poses(ab, k == "link_poses_into", a.pose_calls, t, stream)
                if rep:
                    pt[k].append(ms)
        out["pose_ms_per_call"] = stats(pt)
        return out
    finally:
        ab.close()


def main():
    a = ARGS
    assert torch.cuda.is_available(), "needs the GPU"
    assert a.reps >= 5, "at least five repetitions"
    lib = _lib.load()
    has_new = all(hasattr(lib, s) for s in ("mh_artic_batch_reset_dev", "mh_artic_batch_link_poses_dev")) and hasattr(A.ArticBatch, "reset")
    stream = torch.cuda.current_stream().cuda_stream
    out = {"bench": "artic_reset", "root": os.path.relpath(ROOT, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "control_steps": a.control,
           "steps_per_launch": a.steps, "reps": a.reps, "pose_calls": a.pose_calls, "missing": [] if has_new else ["reset_dev", "link_poses_into"]}
    scenes = a.scenes.split(",")
    assert set(scenes) <= {"ur10", "mixed_all"}, scenes
    if "ur10" in scenes:
        m, _, _ = A.load_sdf(os.path.join(ROOT, "tests", "scenes", "ten_joint_arm.sdf"))
        q0, qd0 = ur10_states(m, a.B_arm)
        out["ur10"] = scene("ur10", m, q0, qd0, 5e-4, has_new, a, stream)
        print("ur10: " + json.dumps(out["ur10"]), file=sys.stderr, flush=True)
    if "mixed_all" in scenes:
        m, sampler, dt = BS.mixed_all()
        q0, qd0 = BS.aim(BS.build_boxsphere_ref(), m, sampler, a.B, len("mixed_all"))
        out["mixed_all"] = scene("mixed_all", m, q0, qd0, dt, has_new, a, stream)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
