"""Fuzz of the box kernels (include/moby_hip_artic.h, mh_artic_model.nboxes; mh_artic_box.hip, mh_artic_box_pose.hip) against the box reference
(tests/native/artic_box_ref.cpp): random floating bodies (tests/test_artic_pose.py random_floating: a base of random pose and inertia, 0-3 revolute /
prismatic links, some with limits and restitution) or random fixed-base chains, 1-4 boxes of random size, pose and link, sometimes a sphere too,
against a floor under the no-slip or the Drumwright-Shell model; the stabiliser on or off, CRB or FSAB, angle or pose coordinates (floating
bases), random states and random drives changed every launch of 10 steps; q, qd, the poses, the rand() stream, the warm starts and the counters
bit for bit.     python tests/tools/fuzz_artic_box.py [seed0] [cases]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from moby_amd import artic as A, scene as S  # noqa: E402
from tests.artic_box_ref import build_box_ref  # noqa: E402
from tests.test_artic_drive import FIELDS    # noqa: E402
from tests.test_artic_pose import rand_rot, random_floating  # noqa: E402


def make_case(seed):
    rng = np.random.default_rng(seed)
    floating = rng.random() < 0.7
    if floating:
        m = random_floating(rng)
        first = 5
    else:
        m = A.chain_model(int(rng.integers(1, 4)), gravity=(0.0, -9.81, 0.0))
        first = 0
    nj = m.nj
    for j in range(6 if floating else 0, nj):
        if rng.random() < 0.5:
            m.lolimit[j] = -rng.uniform(0.05, 0.6); m.hilimit[j] = rng.uniform(0.05, 0.6); m.limit_restitution[j] = rng.choice([0.0, 0.4])
    eps = float(rng.choice([0.0, 0.3])); mu = float(rng.choice([100.0, 0.5, 0.05]))
    floor = (0.0, float(rng.uniform(-0.6, -0.2)) if floating else float(rng.uniform(-0.7, -0.3)), 0.0)
    if rng.random() < 0.3:
        A.add_spheres(m, [(int(rng.integers(first, nj)), rng.uniform(-0.2, 0.2, 3), float(rng.uniform(0.05, 0.2)))], plane_normal=(0.0, 1.0, 0.0),
                      plane_point=floor, epsilon=eps, mu_coulomb=mu)
    boxes = [(int(rng.integers(first, nj)), rng.uniform(-0.2, 0.2, 3), rand_rot(rng) if rng.random() < 0.7 else np.eye(3), rng.uniform(0.05, 0.6, 3))
             for _ in range(int(rng.integers(1, 5)))]
    A.add_boxes(m, boxes, plane_normal=(0.0, 1.0, 0.0), plane_point=floor, epsilon=eps, mu_coulomb=mu)
    m.cstab_max_iterations = int(rng.choice([0, 10]))
    m.algorithm = int(rng.integers(0, 2))
    B = int(rng.integers(1, 5))
    q = np.zeros((B, nj)); qd = np.zeros((B, nj))
    if floating:
        q[:, :3] = rng.uniform(-0.1, 0.1, (B, 3)); q[:, 3:6] = rng.uniform(-1.0, 1.0, (B, 3))
        qd[:, :3] = rng.uniform(-1.0, 1.0, (B, 3)); qd[:, 3:6] = rng.uniform(-5.0, 5.0, (B, 3))
        qd[:, 6:] = rng.uniform(-2.0, 2.0, (B, nj - 6))
    else:
        q[:] = rng.uniform(-0.5, 0.5, (B, nj)); qd[:] = rng.uniform(-2.0, 2.0, (B, nj))
    pose = floating and rng.random() < 0.5
    launches = []
    for _ in range(int(rng.integers(2, 6))):
        if rng.random() < 0.3:
            launches.append(None)
            continue
        rows = 10 if rng.random() < 0.5 else 1
        sh = (rows, B, nj) if rows > 1 else (B, nj)
        launches.append(A.Drive(kp=rng.uniform(0.0, 10.0, (B, nj)), kv=rng.uniform(0.0, 0.5, (B, nj)), q_des=rng.uniform(-0.5, 0.5, sh),
                                qd_des=rng.uniform(-1.0, 1.0, sh), tau_ff=rng.uniform(-2.0, 2.0, sh)))
    return m, q, qd, pose, launches


if __name__ == "__main__":
    seed0 = int(sys.argv[1]) if len(sys.argv) > 1 else 6100
    cases = int(sys.argv[2]) if len(sys.argv) > 2 else 300
    ref = build_box_ref()
    SKIP_AFTER = 5.0
    bad = skipped = solves = failed = unsup = rows16 = 0
    for case in range(cases):
        m, q0, qd0, pose, launches = make_case(seed0 + case)
        B, nj = q0.shape
        ab = A.ArticBatch(m, np.zeros_like(q0), np.zeros_like(qd0), base_coords="pose" if pose else "angles")
        P0 = ab.base_pose() if pose else None
        # the reference first: a world that keeps hitting the mini-step cap costs minutes on either side -- skip such a case
        q_r, qd_r, aux_r = q0.copy(), qd0.copy(), S.new_aux(B)
        P_r = None if P0 is None else P0.copy()
        t0 = time.time(); done = 0
        for d in launches:
            if time.time() - t0 > SKIP_AFTER:
                break
            ref.step(m, q_r, qd_r, aux_r, 1e-3, 10, pose=P_r, drive=d); done += 1
        if done < len(launches):
            ab.close(); skipped += 1; print("seed %d skipped: the reference needed more than %g s" % (seed0 + case, SKIP_AFTER), flush=True); continue
        ab.upload(q0, qd0, S.new_aux(B))
        for d in launches:
            ab.step(1e-3, 10, drive=d)
        q_g, qd_g, aux_g = ab.download()
        P_g = ab.base_pose() if pose else None
        ab.close()
        same = (np.array_equal(q_g, q_r, equal_nan=True) and np.array_equal(qd_g, qd_r, equal_nan=True)
                and (not pose or np.array_equal(P_g, P_r, equal_nan=True)) and all(np.array_equal(aux_g[f], aux_r[f]) for f in FIELDS))
        for w in range(B):
            k = int(aux_r["vns_size"][w]); same = same and np.array_equal(aux_g["vns"][w, :k], aux_r["vns"][w, :k])
            k = int(aux_r["zlast_size"][w]); same = same and np.array_equal(aux_g["zlast"][w, :k], aux_r["zlast"][w, :k])
        solves += int(aux_r["lcp_solves"].sum()); failed += int(((aux_r["status"] & S.MH_WORLD_LCP_FAILED) != 0).sum())
        unsup += int(((aux_r["status"] & S.MH_WORLD_UNSUPPORTED) != 0).sum())
        if not same:
            bad += 1
            print("MISMATCH seed %d: nj %d boxes %d spheres %d alg %d stab %d pose %d; max |dq| %.3e; %s" % (
                seed0 + case, nj, m.nboxes, m.nspheres, m.algorithm, m.cstab_max_iterations, pose, np.nanmax(np.abs(q_g - q_r)),
                [f for f in FIELDS if not np.array_equal(aux_g[f], aux_r[f])]), flush=True)
    print("fuzz_artic_box: %d cases from seed %d (%d skipped as too slow for the reference), %d mismatches; %d LCP solves, %d worlds ended by an "
          "exception, %d over capacity" % (cases, seed0, skipped, bad, solves, failed, unsup))
    sys.exit(1 if bad else 0)
