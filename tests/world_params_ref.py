"""TEST INFRASTRUCTURE shared by tests/test_world_params.py and tests/test_world_params_gpu.py: per-world parameters (include/moby_hip.h, "Per-world
parameters") against the existing CPU references, which take ONE scene per call -- so world w of a varied batch is compared with a reference run of
world w's scene: record w written into copies of the scene and the statics.  Also the varied batches of the tests and the conditions on them."""
import functools

import numpy as np

from moby_amd import scene as S
from tests import world_statics_ref as W

FATAL = W.FATAL
SCENE_FIELDS = ("mass", "inertia", "geom_dim", "plane_R", "plane_o", "gravity", "cp_epsilon", "cp_mu_coulomb", "cp_mu_viscous", "cp_compliance")
STATICS_FIELDS = (("st_R", "R"), ("st_o", "o"), ("st_dim", "dim"))


def world_scene(sc, stt, params, w):
    """copies of the scene and the statics (or None) with record w written into them: the scene world w of the batch is"""
    s2 = S.mh_scene.from_buffer_copy(bytes(sc))
    for f in SCENE_FIELDS:
        np.ctypeslib.as_array(getattr(s2, f))[...] = params[f][w]
    t2 = None
    if stt is not None:
        t2 = S.mh_world_statics.from_buffer_copy(bytes(stt))
        for f, g in STATICS_FIELDS:
            np.ctypeslib.as_array(getattr(t2, g))[...] = params[f][w]
    return s2, t2


def step_ref_params(sc, stt, params, st, aux, dt, nsteps, want_traj=False, forces=None, wrench=None):
    """the reference on the worlds of a varied batch IN PLACE (st (B, nb * 13), aux B records), one run per world -> trajectory or None.
    wrench: (B, nb, 6) or (rows, B, nb, 6), as the batch takes it; world w reads its own entries"""
    B = st.shape[0]
    traj = np.zeros((B, nsteps, sc.nb, 7)) if want_traj else None
    for w in range(B):
        s2, t2 = world_scene(sc, stt, params, w)
        sw, aw = st[w:w + 1].copy(), aux[w:w + 1].copy()
        ww = None if wrench is None else np.ascontiguousarray(np.asarray(wrench)[..., w:w + 1, :, :])
        tr = W.reference().step(s2, sw, aw, dt, nsteps, statics=t2, want_traj=want_traj, forces=forces, wrench=ww).traj
        st[w], aux[w] = sw[0], aw[0]
        if want_traj:
            traj[w] = tr[0]
    return traj


def run_ref_params(sc, stt, params, st, dt, nsteps, seed=1, **kw):
    """the reference per world on copies -> (state, aux, trajectory or None)"""
    s2 = np.array(st, dtype=np.float64, copy=True)
    aux = S.new_aux(s2.shape[0], seed)
    traj = step_ref_params(sc, stt, params, s2, aux, dt, nsteps, **kw)
    return s2, aux, traj


# ---- the varied batch: the mixed scene of tests/world_statics_ref.py, every world but world 0 a scene of its own ---------------------------------------
VARIED_DT, VARIED_NSTEPS = 2e-3, 60


def varied_records(sc, stt, B):
    """world 0 keeps the scene; world w >= 1 draws from RandomState(500 + w).  Bodies only shrink (x U(0.97, 1)), the ground and the wall only recede, the
    static box's top only sinks: the start states of mixed_batch stay clear of everything."""
    p = S.make_params(sc, stt, B)
    ntot = sc.nb + sc.has_ground + stt.n
    for w in range(1, B):
        r = np.random.RandomState(500 + w)
        for b in range(sc.nb):
            m = r.uniform(0.5, 2.0)
            p["mass"][w, b] *= m
            p["inertia"][w, b] *= m * r.uniform(0.8, 1.25, 3)
            p["geom_dim"][w, b] *= r.uniform(0.97, 1.0, 3)
        p["gravity"][w, 1] *= r.uniform(0.7, 1.3)
        p["gravity"][w, 0] = 0.3 * (r.uniform() - 0.5)
        p["gravity"][w, 2] = 0.3 * (r.uniform() - 0.5)
        p["plane_o"][w] -= p["plane_R"][w].reshape(3, 3)[:, 1] * r.uniform(0.0, 2e-3)         # the ground 0-2 mm down its normal
        p["st_o"][w, 0] -= p["st_R"][w, 0].reshape(3, 3)[:, 1] * r.uniform(0.0, 2e-3)        # the wall 0-2 mm back along its normal
        p["st_dim"][w, 1, 0] *= r.uniform(0.9, 1.2)                                          # the static box: x and z edges
        p["st_dim"][w, 1, 2] *= r.uniform(0.9, 1.2)
        shift = np.array([r.uniform(-0.025, 0.025), -r.uniform(0.0, 1e-3), r.uniform(-0.025, 0.025)])
        p["st_o"][w, 1] += p["st_R"][w, 1].reshape(3, 3) @ shift                              # ... its centre, in its own axes
        for q in range(ntot * (ntot - 1) // 2):
            p["cp_epsilon"][w, q] = min(1.0, p["cp_epsilon"][w, q] * r.uniform(0.5, 1.5))
            p["cp_mu_coulomb"][w, q] *= r.uniform(0.5, 1.5)
            p["cp_mu_viscous"][w, q] *= r.uniform(0.5, 1.5)
    return p


VARIED_FORCES = dict(stokes=((0.3, 0.2, 0.4), (0.05, 0.03, 0.02)), damping=((0.1, 0.02, 0.05, 0.01), (0.2, 0.03, 0.04, 0.02), (0.15, 0.01, 0.06, 0.03)))


@functools.lru_cache(maxsize=None)
def varied_case():
    """dict(scene, statics, params, state, dt, nsteps, forces, wrench) of the varied batch; built once, the arrays read-only"""
    sc, stt, st = W.mixed_batch(8)
    p = varied_records(sc, stt, 8)
    wrench = np.random.RandomState(13).uniform(-1.0, 1.0, size=(VARIED_NSTEPS, 8, 3, 6))
    for a in (st, p, wrench):
        a.setflags(write=False)
    return dict(scene=sc, statics=stt, params=p, state=st, dt=VARIED_DT, nsteps=VARIED_NSTEPS, forces=S.make_forces(3, **VARIED_FORCES), wrench=wrench)


def check_conditions(aux, nsteps):
    """what every varied input must satisfy, asserted on the reference alone"""
    assert ((aux["status"] & FATAL) == 0).all(), aux["status"]
    assert (aux["lcp_solves"] > 0).all(), aux["lcp_solves"]
    assert (aux["mini_steps"] <= 50 * nsteps).all(), aux["mini_steps"]            # bounds the GPU test's run time


@functools.lru_cache(maxsize=None)
def varied_run(forced=False):
    """(case, state, aux, trajectory) of the reference per world for the varied batch -- with the stored forces and the wrench schedule if `forced` --
    computed once per process and handed out read-only, its conditions asserted"""
    c = varied_case()
    kw = dict(forces=c["forces"], wrench=c["wrench"]) if forced else {}
    st, aux, traj = run_ref_params(c["scene"], c["statics"], c["params"], c["state"], c["dt"], c["nsteps"], want_traj=True, **kw)
    check_conditions(aux, c["nsteps"])
    if not forced:
        st_s = W.reference_run("mixed")[1]                                            # the shared-scene run of the same start states
        np.testing.assert_array_equal(st[0], st_s[0])                                 # world 0 keeps the scene
        assert all(not np.array_equal(st[w], st_s[w]) for w in range(1, 8))
    for a in (st, aux, traj):
        a.setflags(write=False)
    return c, st, aux, traj


# ---- the last slots: body lane 7 and pair slot 35 (plane8), the last static slot (ring) ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def slots_case(name):
    """`plane8`: nb = 8, one static plane; per-world plane height and radii -- pair slot 35 (body 7, the plane) and body lane 7 of the fill carry values of
    their own.  `ring`: nb = 1, eight statics with per-world frames -- static slot 7 is used."""
    c = W.gpu_cases()[name]
    sc, stt, st = c["scene"], c["statics"], c["state"]
    B = st.shape[0]
    p = S.make_params(sc, stt, B)
    for w in range(1, B):
        r = np.random.RandomState(900 + w)
        if name == "plane8":
            p["geom_dim"][w, :8, 0] *= r.uniform(0.97, 1.0, 8)                          # balls only shrink: the rows stay clear of each other
            p["mass"][w, :8] *= r.uniform(0.5, 2.0, 8)
            p["inertia"][w, :8] *= r.uniform(0.5, 2.0, (8, 1))
            p["st_o"][w, 0, 1] -= r.uniform(0.0, 1e-3)                                  # the plane 0-1 mm lower
            for q in range(36):
                p["cp_mu_coulomb"][w, q] *= r.uniform(0.5, 1.5)
                p["cp_epsilon"][w, q] *= r.uniform(0.5, 1.5)
        else:
            for k in range(8):                                                          # every static recedes from the ball's start over the table
                if stt.type[k] == S.MH_STATIC_PLANE:
                    p["st_o"][w, k] -= p["st_R"][w, k].reshape(3, 3)[:, 1] * r.uniform(0.0, 5e-2)
                else:
                    p["st_dim"][w, k] *= r.uniform(0.9, 1.0, 3)
                    p["st_o"][w, k, 1] -= r.uniform(0.0, 1e-3)
    p.setflags(write=False)
    return dict(scene=sc, statics=stt, params=p, state=st, dt=c["dt"], nsteps=c["nsteps"])
