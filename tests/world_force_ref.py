"""TEST INFRASTRUCTURE shared by tests/test_world_forces.py and tests/test_world_forces_gpu.py: the batches the forced world step is tested on and their
reference results (tests/world_ref.py), computed once and read-only."""
import functools

import numpy as np

from moby_amd import scene as S
from tests.world_ref import reference

G = 9.81


# ---- the batches ------------------------------------------------------------------------------------------------------------------------------
def hover_scene():
    """MH_MAX_BODIES spheres of masses 1 + 0.25 b, no ground, 3 apart along x: nothing ever touches"""
    nb = S.MH_MAX_BODIES
    return S.make_scene([0.5] * nb, [1.0 + 0.25 * b for b in range(nb)], (0.0, -G, 0.0))


def hover_batch(B=3):
    sc = hover_scene()
    rng = np.random.default_rng(5)
    st = np.zeros((B, sc.nb, S.MH_BODY_STATE))
    st[:, :, 0] = 3.0 * np.arange(sc.nb)
    st[:, :, 6] = 1.0
    st[:, :, 7:10] = rng.uniform(-0.5, 0.5, (B, sc.nb, 3))
    st[:, :, 10:13] = rng.uniform(-1.0, 1.0, (B, sc.nb, 3))
    wrench = np.zeros((B, sc.nb, 6))
    for b in range(sc.nb):
        wrench[:, b, 1] = -(sc.gravity[1] * sc.mass[b])
    return sc, st.reshape(B, -1), wrench


def cone_batch():
    """a unit box (m = 1) resting on the plane with mu = 0.5 (friction limit mu m g = 4.905 N), pushed along x with 0, 2, 4 and 8 N"""
    sc = S.box_scene(mu_coulomb=0.5)
    st = np.tile(S.box_state(), (4, 1))
    wrench = np.zeros((4, 1, 6))
    wrench[:, 0, 0] = (0.0, 2.0, 4.0, 8.0)
    return sc, st, wrench


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """name -> dict(scene, state, dt, nsteps, forces, wrench): the batches of tests/test_world_forces_gpu.py, at the smallest shapes at which each
    kernel path can go wrong (every variant, contacts, steps of several mini-steps, per-step rows, body lanes 0..7)"""
    out = {}
    rng = np.random.default_rng(17)
    w = np.concatenate([rng.uniform(-2.0, 2.0, (60, 5, 3, 3)), rng.uniform(-0.4, 0.4, (60, 5, 3, 3))], axis=3)
    out["stack"] = dict(scene=S.sphere_stack_scene(), state=S.sphere_stack_state(5), dt=0.01, nsteps=60,
                        forces=S.make_forces(3, stokes=(0.3, 0.05), damping=(0.2, 0.02, 0.1, 0.01)), wrench=w)
    # one row held for the whole run (rows == 1): the schedule's mean row.  Spheres that spin while in contact cost the reference's conservative
    # advancement tens of thousands of sub-steps per step (here as in Moby: dist / (|omega| r) is tiny), and a torque held for the whole run spins
    # them up: a full-size row (0.4 N m) costs 3 x the scheduled run, on the CPU and on the GPU alike; the mean row (0.07 N m) keeps the same path cheap
    out["stack_const"] = dict(out["stack"], wrench=w.mean(axis=0))
    # ... and a full-size row (torques up to 0.4 N m) held over a run short enough to stay cheap: 12 steps, contacts and several mini-steps per step already
    out["stack_const_full"] = dict(out["stack"], wrench=w[0].copy(), nsteps=12)
    st = np.tile(S.bouncing_ball_state(1), (3, 1)); st[:, 1] = (1.5, 2.0, 3.0)
    out["ball"] = dict(scene=S.bouncing_ball_scene(), state=st, dt=0.01, nsteps=200, forces=S.make_forces(1, stokes=(0.8, 0.1)), wrench=None)
    out["wheel"] = dict(scene=S.rimless_wheel_scene(), state=S.rimless_wheel_state((0.24, 0.4, 0.6)), dt=0.001, nsteps=400,
                        forces=S.make_forces(1, damping=(0.05, 0.05, 0.02, 0.02)), wrench=None)
    sc, st, w = cone_batch()
    out["cone"] = dict(scene=sc, state=st, dt=0.01, nsteps=100, forces=None, wrench=w)
    sc, st, w = hover_batch()
    out["hover_stokes"] = dict(scene=sc, state=st, dt=0.01, nsteps=50, forces=S.make_forces(sc.nb, stokes=(0.3, 0.05)), wrench=w)
    ws = np.concatenate([rng.uniform(-2.0, 2.0, (50,) + w.shape[:2] + (3,)), rng.uniform(-0.4, 0.4, (50,) + w.shape[:2] + (3,))], axis=3)
    out["hover_sched"] = dict(out["hover_stokes"], forces=S.make_forces(sc.nb, damping=(0.2, 0.02, 0.1, 0.01)), wrench=ws)   # one row per step, no contacts
    return out


@functools.lru_cache(maxsize=None)
def reference_run(name):
    """(case, final state, final aux, trajectory) of the reference for gpu_cases()[name], computed once per process and handed out read-only"""
    c = gpu_cases()[name]
    st, aux = c["state"].copy(), S.new_aux(c["state"].shape[0])
    traj = reference().step(c["scene"], st, aux, c["dt"], c["nsteps"], forces=c["forces"], wrench=c["wrench"], want_traj=True).traj
    # a world that ends with an error bit makes the INPUT wrong for a comparison (MH_WORLD_IMPACT_TOL is a warning)
    assert ((aux["status"] & ~S.MH_WORLD_IMPACT_TOL) == 0).all(), (name, aux["status"])
    for a in (st, aux, traj):
        a.setflags(write=False)
    return c, st, aux, traj

