"""Fuzz of the DRIVEN articulated step (include/moby_hip_artic.h, mh_artic_batch_step_driven) against the driven reference
(tests/native/artic_drive_ref.cpp): the random models of fuzz_artic.py (make_case / complete_case: trees of 1-8 joints, link spheres on a tilted
plane, limits, restitution, both impact models, both dynamics algorithms; `floating`: floating bases) with random drives -- per-world gains, targets
and forces, PD and feed-forward terms apart and together, held rows and per-step schedules, a new drive every launch of 10 steps; q, qd, the rand()
stream, the warm starts and the counters bit for bit.     python tests/tools/fuzz_artic_drive.py [seed0] [cases] [floating]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from moby_amd import artic as A, scene as S  # noqa: E402
from tests import native_build               # noqa: E402
from tests.oracle_api import Oracle          # noqa: E402
from tests.test_artic_drive import DriveRef, random_drive  # noqa: E402
from tests.tools import fuzz_artic as F      # noqa: E402

FIELDS = F.FIELDS + ("stab_iters", "stab_rows")
TERMS = (A.MH_DRIVE_FORCE, A.MH_DRIVE_PD, A.MH_DRIVE_FORCE | A.MH_DRIVE_PD)

if __name__ == "__main__":
    o = Oracle(os.path.join(ROOT, "oracle", "liboracle.so"))
    seed0 = int(sys.argv[1]) if len(sys.argv) > 1 else 1900
    cases = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    F.FLOATING = len(sys.argv) > 3 and sys.argv[3] == "floating"
    ref = DriveRef(native_build.build(("artic_drive_ref.cpp",), "artic_drive_ref"))
    SKIP_AFTER = 5.0
    bad = skipped = solves = 0
    for case in range(cases):
        m, q0, qd0, nsteps = F.complete_case(o, seed0 + case)
        B, nj = q0.shape
        rng = np.random.default_rng(10 ** 6 + seed0 + case)
        launches = []
        for _ in range((nsteps + 9) // 10):
            rows = 10 if rng.random() < 0.5 else 1
            launches.append(random_drive(rng, B, nj, rows=rows, terms=int(rng.choice(TERMS)), kp=(0.0, 20.0), kv=(0.0, 0.5), qspan=0.8, tau=2.0))
        # the reference first: a world that keeps hitting the mini-step cap costs minutes on either side -- skip such a case
        q_r, qd_r, aux_r = q0.copy(), qd0.copy(), S.new_aux(B)
        t0 = time.time(); done = 0
        for d in launches:
            if time.time() - t0 > SKIP_AFTER:
                break
            ref.step(m, q_r, qd_r, aux_r, 1e-3, 10, d); done += 1
        if done < len(launches):
            skipped += 1; print("seed %d skipped: the reference needed more than %g s" % (seed0 + case, SKIP_AFTER), flush=True); continue
        ab = A.ArticBatch(m, q0, qd0)
        for d in launches:
            ab.step(1e-3, 10, drive=d)
        q_g, qd_g, aux_g = ab.download(); ab.close()
        same = np.array_equal(q_g, q_r, equal_nan=True) and np.array_equal(qd_g, qd_r, equal_nan=True) and all(np.array_equal(aux_g[f], aux_r[f]) for f in FIELDS)
        for w in range(B):
            k = int(aux_r["vns_size"][w]); same = same and np.array_equal(aux_g["vns"][w, :k], aux_r["vns"][w, :k])
            k = int(aux_r["zlast_size"][w]); same = same and np.array_equal(aux_g["zlast"][w, :k], aux_r["zlast"][w, :k])
        solves += int(aux_r["lcp_solves"].sum())
        if not same:
            bad += 1
            print("MISMATCH seed %d: nj %d spheres %d alg %d; max |dq| %.3e; %s" % (seed0 + case, nj, m.nspheres, m.algorithm, np.nanmax(np.abs(q_g - q_r)),
                  [f for f in FIELDS if not np.array_equal(aux_g[f], aux_r[f])]), flush=True)
        else:
            print("case %d ok (nj %d, %d spheres, %d LCP solves so far)" % (case, nj, m.nspheres, solves), flush=True)
    print("fuzz_artic_drive%s: %d cases from seed %d (%d skipped as too slow for the reference), %d mismatches; %d LCP solves"
          % (" (floating bases)" if F.FLOATING else "", cases, seed0, skipped, bad, solves))
    sys.exit(1 if bad else 0)
