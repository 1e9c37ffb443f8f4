"""TEST INFRASTRUCTURE shared by tests/test_world_report.py and tests/test_world_report_gpu.py: the ctypes face of the contact-report reference
(tests/native/world_report_ref.cpp), built once per process, the cases the tests run and their reference results, computed once and read-only."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile

import numpy as np

from moby_amd import scene as S
from tests import world_force_ref as F
from tests import world_params_ref as P
from tests import world_statics_ref as W

ROOT = W.ROOT
FATAL = W.FATAL
REPORT_PAIR = 8
SH_MINI, SH_PAIR_CONTACTS, SH_PAIRS_LOADED, SH_RESTITUTION, SH_ZERO, SH_NEG_SIGN = range(6)    # columns of the shape census (world_report_ref.cpp)


def npt_of(sc, stt):
    ntot = sc.nb + sc.has_ground + (stt.n if stt is not None else 0)
    return ntot * (ntot - 1) // 2


class ReportRef:
    """ctypes face of tests/native/world_report_ref.cpp"""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.world_report_ref_step.restype = None

    def step(self, sc, statics, state, aux, dt, nsteps, want_traj=False, forces=None, wrench=None):
        """B worlds x nsteps in place -> (trajectory (B, nsteps, nb, 7) or None, report (B, nsteps, npt, 8), shape census (B, nsteps, 6))"""
        B = state.shape[0]
        Pp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        traj = np.zeros((B, nsteps, sc.nb, 7)) if want_traj else None
        report = np.full((B, nsteps, npt_of(sc, statics), REPORT_PAIR), np.nan)
        shape = np.zeros((B, nsteps, 6), dtype=np.int32)
        w, rows = None, 1
        if wrench is not None:
            w = np.ascontiguousarray(wrench, dtype=np.float64)
            rows = 1 if w.ndim == 3 else w.shape[0]
            assert w.shape[-3:] == (B, sc.nb, 6)
        self.lib.world_report_ref_step(ctypes.byref(sc), None if statics is None else ctypes.byref(statics), int(B), ctypes.c_double(dt), int(nsteps),
                                       Pp(state), Pp(aux), Pp(traj), None if forces is None else ctypes.byref(forces), Pp(w), int(rows), Pp(report), Pp(shape))
        return traj, report, shape


@functools.lru_cache(maxsize=None)
def reference():
    """the report reference, built once per process with g++ and oracle/Makefile's CXXFLAGS (the oracle's floating-point contract: no FMA)"""
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M).group(1).split()
    so = os.path.join(tempfile.mkdtemp(prefix="world_report_ref_"), "libworld_report_ref.so")
    subprocess.check_call(["g++"] + flags + ["-shared", "-I" + os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "native", "world_report_ref.cpp"), "-o", so])
    return ReportRef(so)


def run_ref(sc, stt, st, dt, nsteps, seed=1, aux=None, **kw):
    """the reference on copies -> (state, aux, trajectory or None, report, shape census)"""
    s2 = np.array(st, dtype=np.float64, copy=True)
    a2 = S.new_aux(s2.shape[0], seed) if aux is None else aux.copy()
    traj, report, shape = reference().step(sc, stt, s2, a2, dt, nsteps, **kw)
    return s2, a2, traj, report, shape


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
    """what the cases are there for, asserted on the reference runs alone (the numbers are those of tests/native/world_report_ref.cpp's census)"""
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
