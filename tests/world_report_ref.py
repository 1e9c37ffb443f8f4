"""TEST INFRASTRUCTURE shared by tests/test_world_report.py and tests/test_world_report_gpu.py: the cases the contact report is tested on and their
reference results (tests/world_ref.py, the step with a report sink), computed once and read-only."""
import functools

import numpy as np

from moby_amd import scene as S
from tests import world_force_ref as F
from tests import world_params_ref as P
from tests import world_ref
from tests import world_statics_ref as W
from tests.world_ref import REPORT_PAIR, npt_of

ROOT = W.ROOT
FATAL = W.FATAL
SH_MINI, SH_PAIR_CONTACTS, SH_PAIRS_LOADED, SH_RESTITUTION, SH_ZERO, SH_NEG_SIGN = range(6)    # columns of the shape census (tests/native/world_ref.cpp)


def run_ref(sc, stt, st, dt, nsteps, seed=1, aux=None, **kw):
    """the reference with the report on copies -> (state, aux, trajectory or None, report, shape census)"""
    s2, a2, r = world_ref.run_ref(sc, st, dt, nsteps, seed=seed, aux=aux, statics=stt, want_report=True, want_shape=True, **kw)
    return s2, a2, r.traj, r.report, r.shape


def run_ref_params(sc, stt, params, st, dt, nsteps, forces=None, wrench=None):
    """per-world records: one run per world, each against the scene world w is (tests/world_params_ref.py) -> (state, aux, report, shape census)"""
    B = st.shape[0]
    s2 = np.array(st, dtype=np.float64, copy=True)
    aux = S.new_aux(B)
    report = np.zeros((B, nsteps, npt_of(sc, stt), REPORT_PAIR))
    shape = np.zeros((B, nsteps, 6), dtype=np.int32)
    for w in range(B):
        sw, tw = P.world_scene(sc, stt, params, w)
        ww = None if wrench is None else np.ascontiguousarray(np.asarray(wrench)[..., w:w + 1, :, :])
        a, b, _, r, h = run_ref(sw, tw, s2[w:w + 1], dt, nsteps, aux=aux[w:w + 1], forces=forces, wrench=ww)
        s2[w], aux[w], report[w], shape[w] = a[0], b[0], r[0], h[0]
    return s2, aux, report, shape


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
def resting_ball():
    """a ball at rest on a static plane, no restitution: every step its weight times dt comes up through one contact under its centre"""
    r, m = 0.25, 2.0
    sc = W.scene([("sphere", r, m)], 1, epsilon=0.0, mu_coulomb=0.5)
    stt = S.make_statics([dict(plane=True, R=W.R_UP)])
    st = W.sphere_state(1, 1)
    W.set_body(st, 0, 0, (0.5, r, -0.25))
    return sc, stt, st.reshape(1, -1), m, r


def box_ball_batch(B=4):
    """W.box_corner_batch(B, with_ball=True) moved a quarter of a metre off its wall.  As it stands that batch is the capacity case: 4 + 4 vertex contacts
    and the ball's make an LCP of 72 rows, beyond the wave solver, so every world gets MH_WORLD_UNSUPPORTED once the ball lands and its rows are undefined.
    Off the wall the box rests on four vertex contacts of ONE pair (geom1 the plane, the higher index: sign = -1) and the ball lands on it (box-sphere)."""
    sc, stt, st = W.box_corner_batch(B, with_ball=True)
    st = st.reshape(B, 2, S.MH_BODY_STATE).copy()
    st[:, :, 0] += 0.25
    return sc, stt, st.reshape(B, -1)


def plane8_last_batch(B=8):
    """W.plane8_batch with the bodies in reverse order: ntot = 9, 36 pair slots.  As it stands its body 7 is a ball of the upper row and never touches the
    plane, so slot 35 (body 7, the plane) stays empty; reversed, body 7 is the first ball of the row ON the plane and lane / slot 35 of the fold carries a
    load.  The balls are equal, so nothing else changes."""
    sc, stt, st = W.plane8_batch(B)
    st = st.reshape(B, 8, S.MH_BODY_STATE)[:, ::-1].copy()
    return sc, stt, st.reshape(B, -1)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(scene, statics, state, dt, nsteps[, params, forces, wrench]); built once, the arrays read-only.  Each is there for something the
    report can get wrong; shape_conditions() says what and asserts it on the reference run."""
    out = {}

    def add(name, sc, stt, st, dt, nsteps, **kw):
        st = np.array(st, copy=True)
        st.setflags(write=False)
        out[name] = dict(scene=sc, statics=stt, state=st, dt=dt, nsteps=nsteps, **kw)
    add("corner", *W.corner_batch(8), 1e-3, 20)
    add("box_ball", *box_ball_batch(4), 1e-3, 20)
    add("mixed", *W.mixed_batch(8), 2e-3, 60)
    add("noslip_table", *W.table_batch(4, mu=100.0), 1e-3, 20)
    add("plane8", *plane8_last_batch(8), 2e-3, 12)
    v = P.varied_case()
    add("varied", v["scene"], v["statics"], v["state"], v["dt"], v["nsteps"], params=v["params"])
    # the first 12 steps of the forced stack (Stokes drag, damping, a wrench row per step): contacts and several mini-steps per step already, and a
    # reference run of a second or two (spinning spheres in contact cost conservative advancement thousands of sub-steps per step later on)
    f = F.gpu_cases()["stack"]
    add("forced_stack", f["scene"], None, f["state"], f["dt"], 12, forces=f["forces"], wrench=np.ascontiguousarray(f["wrench"][:12]))
    return out


@functools.lru_cache(maxsize=None)
def reference_run(name):
    """(case, final state, final aux, report, shape census) of the reference for cases()[name], computed once per process and handed out read-only.  No
    world of these inputs may carry a bit that makes its rows undefined, so a comparison leaves out none."""
    c = cases()[name]
    if "params" in c:
        st, aux, report, shape = run_ref_params(c["scene"], c["statics"], c["params"], c["state"], c["dt"], c["nsteps"], forces=c.get("forces"), wrench=c.get("wrench"))
    else:
        st, aux, _, report, shape = run_ref(c["scene"], c["statics"], c["state"], c["dt"], c["nsteps"], forces=c.get("forces"), wrench=c.get("wrench"))
    assert ((aux["status"] & FATAL) == 0).all(), (name, aux["status"])
    assert (aux["lcp_solves"] > 0).all() and (report[..., 1].sum(axis=(1, 2)) > 0).all() and np.isfinite(report).all(), name      # every world carried a load
    for a in (st, aux, report, shape):
        a.setflags(write=False)
    return c, st, aux, report, shape


def shape_conditions():
    """what the cases are there for, asserted on the reference runs alone (the numbers are those of tests/native/world_ref.cpp's census)"""
    sh = {n: reference_run(n)[4] for n in ("corner", "box_ball", "mixed", "noslip_table")}
    assert (sh["box_ball"][..., SH_PAIR_CONTACTS] >= 2).any() and (sh["mixed"][..., SH_PAIR_CONTACTS] >= 2).any()       # 1: several contacts of one pair
    assert (sh["corner"][..., SH_PAIRS_LOADED] >= 3).any()                                                                      # 2: three loaded pairs at once
    assert any((s[..., SH_MINI] >= 2).any() for s in sh.values())                                                               # 3: two folded mini-steps with contacts
    assert (sh["mixed"][..., SH_RESTITUTION] > 0).any()                                                                         # 4: a restitution pass added an impulse
    assert any((s[..., SH_ZERO] > 0).any() for s in sh.values())                                                                # 5: a contact counted with zero impulse
    assert (sh["box_ball"][..., SH_NEG_SIGN] > 0).any() and (sh["mixed"][..., SH_NEG_SIGN] > 0).any()                    # 6: geom1 the higher-index body
    rep8 = reference_run("plane8")[3]
    assert rep8.shape[2] == 36 and (rep8[..., 35, 1] > 0).any() and (rep8[..., 0].sum(axis=(0, 1)) > 0).sum() >= 12                 # 7: the last slot, many slots
    return sh
