"""Fuzz of the articulated step in POSE coordinates (include/moby_hip_artic.h, MH_ARTIC_BASE_POSE) against the pose-coordinate reference
(tests/native/artic_pose_ref.cpp): random floating bodies from model_from_links(floating_base=...) (tests/test_artic_pose.py random_floating: a
base of random pose and inertia, 0-3 revolute / prismatic links, some with limits and restitution), optionally spheres on the base and the links
against a floor under the no-slip or the Drumwright-Shell model, the stabiliser on or off, CRB or FSAB, random spins fast enough to pass the
middle hinge's quarter turn, and random drives (tau_ff on every column, PD on the body's joints) changed every launch of 10 steps; q, qd, the
poses, the rand() stream, the warm starts and the counters bit for bit.     python tests/tools/fuzz_artic_pose.py [seed0] [cases]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from moby_amd import artic as A, scene as S  # noqa: E402
from tests import native_build               # noqa: E402
from tests.test_artic_drive import FIELDS    # noqa: E402
from tests.test_artic_pose import PoseRef, random_floating  # noqa: E402


def make_case(seed):
    rng = np.random.default_rng(seed)
    m = random_floating(rng)
    nj = m.nj
    for j in range(6, nj):
        if rng.random() < 0.5:
            m.lolimit[j] = -rng.uniform(0.05, 0.6); m.hilimit[j] = rng.uniform(0.05, 0.6); m.limit_restitution[j] = rng.choice([0.0, 0.4])
    if rng.random() < 0.5:
        spheres = [(5, rng.uniform(-0.1, 0.1, 3), float(rng.uniform(0.1, 0.3)))]
        for j in range(6, min(nj, 8)):
            spheres.append((j, rng.uniform(-0.2, 0.2, 3), float(rng.uniform(0.05, 0.15))))
        A.add_spheres(m, spheres, plane_normal=(0.0, 1.0, 0.0), plane_point=(0.0, -1.6, 0.0), epsilon=float(rng.choice([0.0, 0.5])),
                      mu_coulomb=float(rng.choice([100.0, 0.5])))
    m.cstab_max_iterations = int(rng.choice([0, 10]))
    m.algorithm = int(rng.integers(0, 2))
    B = int(rng.integers(1, 5))
    q = np.zeros((B, nj)); qd = np.zeros((B, nj))
    q[:, :3] = rng.uniform(-0.1, 0.1, (B, 3)); q[:, 3:6] = rng.uniform(-1.0, 1.0, (B, 3))
    qd[:, :3] = rng.uniform(-1.0, 1.0, (B, 3)); qd[:, 3:6] = rng.uniform(-8.0, 8.0, (B, 3)); qd[:, 4] += rng.choice([-1.0, 1.0], B) * 10.0
    qd[:, 6:] = rng.uniform(-2.0, 2.0, (B, nj - 6))
    launches = []
    for _ in range(int(rng.integers(2, 6))):
        if rng.random() < 0.3:
            launches.append(None)
            continue
        rows = 10 if rng.random() < 0.5 else 1
        sh = (rows, B, nj) if rows > 1 else (B, nj)
        on = np.zeros(nj); on[6:] = 1.0
        launches.append(A.Drive(kp=rng.uniform(0.0, 10.0, (B, nj)) * on, kv=rng.uniform(0.0, 0.5, (B, nj)) * on, q_des=rng.uniform(-0.5, 0.5, sh),
                                qd_des=rng.uniform(-1.0, 1.0, sh), tau_ff=rng.uniform(-2.0, 2.0, sh)))
    return m, q, qd, launches


if __name__ == "__main__":
    seed0 = int(sys.argv[1]) if len(sys.argv) > 1 else 4100
    cases = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    ref = PoseRef(native_build.build(("artic_pose_ref.cpp", "artic_drive_ref.cpp"), "artic_pose_ref"))
    SKIP_AFTER = 5.0
    bad = skipped = solves = failed = 0
    for case in range(cases):
        m, q0, qd0, launches = make_case(seed0 + case)
        B, nj = q0.shape
        ab = A.ArticBatch(m, np.zeros_like(q0), np.zeros_like(qd0), base_coords="pose")
        P0 = ab.base_pose()
        # the reference first: a world that keeps hitting the mini-step cap costs minutes on either side -- skip such a case
        q_r, qd_r, P_r, aux_r = q0.copy(), qd0.copy(), P0.copy(), S.new_aux(B)
        t0 = time.time(); done = 0
        for d in launches:
            if time.time() - t0 > SKIP_AFTER:
                break
            ref.step(m, q_r, qd_r, aux_r, P_r, 1e-3, 10, d); done += 1
        if done < len(launches):
            ab.close(); skipped += 1; print("seed %d skipped: the reference needed more than %g s" % (seed0 + case, SKIP_AFTER), flush=True); continue
        ab.upload(q0, qd0, S.new_aux(B))
        for d in launches:
            ab.step(1e-3, 10, drive=d)
        q_g, qd_g, aux_g = ab.download(); P_g = ab.base_pose(); ab.close()
        same = (np.array_equal(q_g, q_r, equal_nan=True) and np.array_equal(qd_g, qd_r, equal_nan=True) and np.array_equal(P_g, P_r, equal_nan=True)
                and all(np.array_equal(aux_g[f], aux_r[f]) for f in FIELDS))
        for w in range(B):
            k = int(aux_r["vns_size"][w]); same = same and np.array_equal(aux_g["vns"][w, :k], aux_r["vns"][w, :k])
            k = int(aux_r["zlast_size"][w]); same = same and np.array_equal(aux_g["zlast"][w, :k], aux_r["zlast"][w, :k])
        solves += int(aux_r["lcp_solves"].sum()); failed += int(((aux_r["status"] & S.MH_WORLD_LCP_FAILED) != 0).sum())
        if not same:
            bad += 1
            print("MISMATCH seed %d: nj %d spheres %d alg %d stab %d; max |dq| %.3e |dP| %.3e; %s" % (
                seed0 + case, nj, m.nspheres, m.algorithm, m.cstab_max_iterations, np.nanmax(np.abs(q_g - q_r)), np.nanmax(np.abs(P_g - P_r)),
                [f for f in FIELDS if not np.array_equal(aux_g[f], aux_r[f])]), flush=True)
    print("fuzz_artic_pose: %d cases from seed %d (%d skipped as too slow for the reference), %d mismatches; %d LCP solves, %d worlds ended by an exception"
          % (cases, seed0, skipped, bad, solves, failed))
    sys.exit(1 if bad else 0)
