"""Fuzz of the box-sphere kernels (include/moby_hip_artic.h, mh_artic_model.pair_kind, box_link = -1; mh_artic_bsp.hip, mh_artic_bsp_pose.hip)
against the box-sphere reference (tests/native/artic_boxsphere_ref.cpp): the random trees of tests/tools/fuzz_artic_pair.py with one or two
roots, 1-4 spheres, 1-3 boxes of which some are static (placed beside the spheres, clear of them at the start), random pairs of both kinds
(every static box in at least one), against a floor under the no-slip or the Drumwright-Shell model; the stabiliser on or off, CRB or FSAB,
angle or pose coordinates (floating bases), random states and random drives changed every launch of 10 steps; q, qd, the poses, the rand()
stream, the warm starts and the counters bit for bit.  A case in which the reference reports a sphere's centre inside a box (the NaN normal
of find_contacts_box_sphere) is skipped and counted; at most 5 % of the cases may be (the tool fails beyond that): the generator keeps radii
well above a step's travel and starts every box-sphere pair apart.
python tests/tools/fuzz_artic_boxsphere.py [seed0] [cases] [list: no GPU, the reference alone]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from moby_amd import _lib, artic as A, scene as S  # noqa: E402
from tests.artic_boxsphere_ref import INSIDE, build_boxsphere_ref  # noqa: E402
from tests.test_artic_drive import FIELDS    # noqa: E402
from tests.test_artic_pose import rand_rot, random_floating  # noqa: E402


def add_root(m, rng):
    """a second chain of 1-2 hinges about z hanging from the world beside the first tree (joints appended, parent -1)"""
    n0 = m.nj
    x = np.array([rng.uniform(0.2, 0.5), rng.uniform(-0.1, 0.3), rng.uniform(-0.1, 0.1)])
    for k in range(int(rng.integers(1, 3))):
        j = m.nj
        if j >= A.MH_ARTIC_MAX_JOINTS: break
        m.parent[j] = -1 if k == 0 else j - 1; m.jtype[j] = A.MH_JOINT_REVOLUTE
        for c in range(9): m.Rrel[j][c] = float(c % 4 == 0); m.inertia[j][c] = 0.01 * float(c % 4 == 0)
        for c in range(3):
            m.trel[j][c] = x[c] if k == 0 else (0.0, -0.3, 0.0)[c]; m.axis[j][c] = float(c == 2); m.com[j][c] = (0.0, -0.15, 0.0)[c]
        m.mass[j] = float(rng.uniform(0.2, 1.0)); m.lolimit[j] = -np.finfo(float).max; m.hilimit[j] = np.finfo(float).max; m.limit_restitution[j] = 0.0
        m.nj = j + 1
    return n0


REF = None          # the reference, once built: make_case places the states with it


def make_case(seed):
    rng = np.random.default_rng(seed)
    floating = rng.random() < 0.6
    if floating:
        m = random_floating(rng)
        first = 5
    else:
        m = A.chain_model(int(rng.integers(2, 4)), gravity=(0.0, -9.81, 0.0))
        first = 0
    root2 = add_root(m, rng) if rng.random() < 0.5 else None
    nj = m.nj
    for j in range(6 if floating else 0, nj):
        if rng.random() < 0.5:
            m.lolimit[j] = -rng.uniform(0.05, 0.6); m.hilimit[j] = rng.uniform(0.05, 0.6); m.limit_restitution[j] = rng.choice([0.0, 0.4])
    eps = float(rng.choice([0.0, 0.3])); mu = float(rng.choice([100.0, 0.5, 0.05]))
    floor = (0.0, float(rng.uniform(-0.6, -0.2)), 0.0)
    links = list(range(first, nj))
    ns = int(rng.integers(1, 5))
    sl = [int(rng.choice(links)) for _ in range(ns)]
    if root2 is not None: sl[-1] = int(rng.integers(root2, nj))          # one sphere on the second root
    if ns > 1 and len(set(sl)) == 1 and len(links) > 1: sl[0] = [l for l in links if l != sl[0]][0]
    A.add_spheres(m, [(l, rng.uniform(-0.15, 0.15, 3), float(rng.uniform(0.08, 0.2))) for l in sl], plane_normal=(0.0, 1.0, 0.0),
                  plane_point=floor, epsilon=eps, mu_coulomb=mu)
    nb = int(rng.integers(1, 4))
    boxes = []
    for _ in range(nb):
        if rng.random() < 0.5:                                             # a static box under / beside the body, its pose in the model frame
            boxes.append((-1, np.array([rng.uniform(-0.5, 0.5), floor[1] + rng.uniform(0.05, 0.3), rng.uniform(-0.3, 0.3)]),
                          rand_rot(rng) if rng.random() < 0.5 else np.eye(3), rng.uniform(0.15, 0.5, 3)))
        else:
            boxes.append((int(rng.choice(links)), rng.uniform(-0.2, 0.2, 3), rand_rot(rng) if rng.random() < 0.7 else np.eye(3), rng.uniform(0.1, 0.4, 3)))
    A.add_boxes(m, boxes, plane_normal=(0.0, 1.0, 0.0), plane_point=floor, epsilon=eps, mu_coulomb=mu)
    pairs = [(a, b) if rng.random() < 0.5 else (b, a) for a in range(ns) for b in range(a + 1, ns) if sl[a] != sl[b] and rng.random() < 0.5]
    bsp = []
    for b, bx in enumerate(boxes):
        cand = [s for s in range(ns) if sl[s] != bx[0]]
        if not cand: cand = []
        take = [s for s in cand if rng.random() < 0.6]
        if bx[0] < 0 and not take and cand: take = [int(rng.choice(cand))]
        bsp += [(b, s) for s in take]
    bsp = bsp[:A.MH_ARTIC_MAX_PAIRS]
    for b, bx in enumerate(boxes):                                         # (a static box that lost its pairs to the cap keeps one)
        if bx[0] < 0 and not any(p[0] == b for p in bsp): bsp = [(b, 0 if sl[0] != -1 else 1)] + bsp[:A.MH_ARTIC_MAX_PAIRS - 1]
    A.add_pairs(m, pairs[:A.MH_ARTIC_MAX_PAIRS - len(bsp)], no_plane=[s for s in range(ns) if rng.random() < 0.3])
    A.add_box_sphere_pairs(m, bsp)
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
    if REF is not None:                                                    # start every box-sphere pair apart: redraw the worlds that do not
        for _ in range(50):
            reg, dist = REF.regions(m, q)
            kinds = np.array([m.pair_kind[k] for k in range(m.npairs)]) == A.MH_ARTIC_PAIR_BOX_SPHERE
            badw = (dist[:, kinds] < 0.05).any(axis=1) if kinds.any() else np.zeros(B, dtype=bool)
            if not badw.any(): break
            q[badw] = rng.uniform(-0.5, 0.5, (int(badw.sum()), nj)) if not floating else np.concatenate(
                [rng.uniform(-0.3, 0.3, (int(badw.sum()), 3)), rng.uniform(-1.0, 1.0, (int(badw.sum()), 3)), rng.uniform(-0.5, 0.5, (int(badw.sum()), nj - 6))], axis=1)
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
    seed0 = int(sys.argv[1]) if len(sys.argv) > 1 else 7100
    cases = int(sys.argv[2]) if len(sys.argv) > 2 else 300
    ref = build_boxsphere_ref()
    REF = ref
    SKIP_AFTER = 5.0
    bad = skipped = solves = failed = unsup = rows16 = inside = 0
    if len(sys.argv) > 3:                                                     # (no GPU: list what the cases hold and what the reference makes of them)
        for case in range(cases):
            m, q0, qd0, pose, launches = make_case(seed0 + case)
            q_r, qd_r, aux_r = q0.copy(), qd0.copy(), S.new_aux(q0.shape[0])
            ins = False
            for _ in range(len(launches)):
                ref.step(m, q_r, qd_r, aux_r, 1e-3, 10)
                ins = ins or not (np.isfinite(q_r).all() and np.isfinite(qd_r).all()) or bool((ref.regions(m, np.nan_to_num(q_r))[0] == INSIDE).any())
            inside += int(ins)
            print(seed0 + case, "inside" if ins else "", "nj", m.nj, "pairs", m.npairs, "kinds", [m.pair_kind[k] for k in range(m.npairs)], "static", sum(m.box_link[k] < 0 for k in range(m.nboxes)), "mask", m.sphere_no_plane, "solves", int(aux_r["lcp_solves"].sum()), "status", list(aux_r["status"]))
        print("fuzz_artic_boxsphere (reference alone): %d of %d cases with a sphere's centre inside a box (%.1f %%)" % (inside, cases, 100.0 * inside / cases))
        sys.exit(0 if inside <= 0.05 * cases else 1)
    for case in range(cases):
        m, q0, qd0, pose, launches = make_case(seed0 + case)
        B, nj = q0.shape
        try:
            ab = A.ArticBatch(m, np.zeros_like(q0), np.zeros_like(qd0), base_coords="pose" if pose else "angles")
        except _lib.MobyHipError as e:                                         # the pair kernels' LDS image beyond 64 KB (more than 10 joints)
            assert "LDS image" in str(e), e
            skipped += 1; print("seed %d refused by create: %s" % (seed0 + case, e), flush=True); continue
        P0 = ab.base_pose() if pose else None
        # the reference first: a world that keeps hitting the mini-step cap costs minutes on either side -- skip such a case
        q_r, qd_r, aux_r = q0.copy(), qd0.copy(), S.new_aux(B)
        P_r = None if P0 is None else P0.copy()
        t0 = time.time(); done = 0
        ins = False
        for d in launches:
            if time.time() - t0 > SKIP_AFTER:
                break
            ref.step(m, q_r, qd_r, aux_r, 1e-3, 10, pose=P_r, drive=d); done += 1
            ins = ins or not (np.isfinite(q_r).all() and np.isfinite(qd_r).all()) or bool((ref.regions(m, np.nan_to_num(q_r), P_r)[0] == INSIDE).any())
        if ins:
            ab.close(); inside += 1; print("seed %d skipped: a sphere's centre inside a box (the reference's NaN normal)" % (seed0 + case), flush=True); continue
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
            print("MISMATCH seed %d: nj %d pairs %d boxes %d spheres %d alg %d stab %d pose %d; max |dq| %.3e; %s" % (
                seed0 + case, nj, m.npairs, m.nboxes, m.nspheres, m.algorithm, m.cstab_max_iterations, pose, np.nanmax(np.abs(q_g - q_r)),
                [f for f in FIELDS if not np.array_equal(aux_g[f], aux_r[f])]), flush=True)
    print("fuzz_artic_boxsphere: %d cases from seed %d (%d skipped: too slow for the reference, or too many joints for the kernels; %d skipped: a sphere's centre inside a box, "
          "%.1f %%), %d mismatches; %d LCP solves, %d worlds ended by an exception, %d over capacity" % (cases, seed0, skipped, inside, 100.0 * inside / cases, bad, solves, failed, unsup))
    sys.exit(1 if bad or inside > 0.05 * cases else 0)
