"""Box primitives on links on the GPU (include/moby_hip_artic.h, mh_artic_model.nboxes): the eight box kernels of mh_artic_box.hip /
mh_artic_box_pose.hip against the box reference (tests/native/artic_box_ref.cpp) bit for bit -- q, qd, every aux field and, in pose
coordinates, the base pose -- and the forced box kernels (mh_debug_set key 12) against today's sphere kernels."""
import os

import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import artic as A
from moby_amd import scene as S
from tests.artic_box_ref import build_box_ref
from tests.test_artic_drive import FIELDS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "scenes")


@pytest.fixture(scope="module")
def box_ref():
    return build_box_ref()


def same(got, ref, B):
    (q_g, qd_g, aux_g), (q_r, qd_r, aux_r) = got, ref
    assert np.array_equal(q_g, q_r), "max |dq| = %.3e" % np.nanmax(np.abs(q_g - q_r))
    assert np.array_equal(qd_g, qd_r), "max |dqd| = %.3e" % np.nanmax(np.abs(qd_g - qd_r))
    for f in FIELDS:
        assert np.array_equal(aux_g[f], aux_r[f]), f
    for w in range(B):
        k = int(aux_r["vns_size"][w]); assert np.array_equal(aux_g["vns"][w, :k], aux_r["vns"][w, :k])
        k = int(aux_r["zlast_size"][w]); assert np.array_equal(aux_g["zlast"][w, :k], aux_r["zlast"][w, :k])


def scene(name, B, seed, iters=None, mu=None, eps=None, nk=None):
    """a scene's model and B perturbed starting states (tumbling drops: random base velocities and spins)"""
    m, _, _, q0, qd0, dt = A.load_xml(os.path.join(SCENES, name))
    if iters is not None: m.cstab_max_iterations = iters
    if mu is not None: m.cp_mu_coulomb = mu
    if eps is not None: m.cp_epsilon = eps
    if nk is not None: m.cp_nk = nk
    rng = np.random.default_rng(seed)
    q = np.tile(q0, (B, 1)); qd = np.tile(qd0, (B, 1))
    if m.floating_base:
        q[1:, 1] += rng.uniform(0.0, 0.3, B - 1); q[1:, 3:6] += rng.uniform(-0.6, 0.6, (B - 1, 3))
        qd[1:, :3] += rng.uniform(-1.0, 1.0, (B - 1, 3)); qd[1:, 3:6] += rng.uniform(-4.0, 4.0, (B - 1, 3))
    else:
        q[:] = rng.uniform(-1.2, 1.2, (B, m.nj)); qd[:] = rng.uniform(-2.0, 2.0, (B, m.nj))
    return m, q, qd, dt


def mixed(B, seed):
    """a floating box with a hinged arm whose tip carries a sphere: spheres and boxes in one contact list"""
    rng = np.random.default_rng(seed)
    arm = dict(parent=-1, type=A.MH_JOINT_REVOLUTE, R0=np.eye(3), x0=(0.3, 0.0, 0.0), axis=(0.0, 0.0, 1.0), com=(0.2, 0.0, 0.0),
               inertia=np.eye(3) * 0.01, mass=0.3, lo=-0.8, hi=0.8, restitution=0.2)
    m = A.model_from_links([arm], gravity=(0.0, -9.81, 0.0), floating_base=dict(R0=np.eye(3), x0=(0.0, 0.4, 0.0), mass=2.0, inertia=np.diag([0.2, 0.3, 0.25])))
    A.add_spheres(m, [(6, (0.4, 0.0, 0.0), 0.05)], plane_normal=(0.0, 1.0, 0.0), epsilon=0.3, mu_coulomb=100.0)
    A.add_boxes(m, [(5, (0.0, 0.0, 0.0), np.eye(3), (0.4, 0.3, 0.35))], plane_normal=(0.0, 1.0, 0.0), epsilon=0.3, mu_coulomb=100.0)
    m.cstab_max_iterations = 10
    q = np.zeros((B, 7)); qd = np.zeros((B, 7))
    q[:, 1] = rng.uniform(0.0, 0.2, B); q[:, 3:6] = rng.uniform(-0.4, 0.4, (B, 3)); q[:, 6] = rng.uniform(-0.5, 0.5, B)
    qd[:, :3] = rng.uniform(-1, 1, (B, 3)); qd[:, 3:6] = rng.uniform(-3, 3, (B, 3))
    return m, q, qd, 1e-3


def four_feet(B, seed):
    """a floating slab on four flat box feet under the no-slip model: 16 vertex contacts (MH_NOSLIP_MAX) once it stands -- contact rows on lanes
    32-47 and a tangent set of up to 32 columns in the impact handler"""
    rng = np.random.default_rng(seed)
    m = A.model_from_links([], gravity=(0.0, -9.81, 0.0), floating_base=dict(R0=np.eye(3), x0=(0.0, 0.06, 0.0), mass=5.0, inertia=np.eye(3)))
    A.add_boxes(m, [(5, (x, -0.05, z), np.eye(3), (0.1, 0.02, 0.1)) for x, z in ((-0.4, -0.4), (0.4, -0.4), (-0.4, 0.4), (0.4, 0.4))],
                plane_normal=(0.0, 1.0, 0.0), epsilon=0.2, mu_coulomb=100.0)
    m.cstab_max_iterations = 10
    q = np.zeros((B, 6)); qd = np.zeros((B, 6))
    q[:, 1] = rng.uniform(0.0, 0.02, B); qd[:, 1] = -rng.uniform(0.0, 0.5, B); qd[1:, 3:6] = rng.uniform(-0.05, 0.05, (B - 1, 3))
    return m, q, qd, 1e-3


CASES = {  # name -> (builder, steps per launch)
    "four_feet_noslip": (lambda: four_feet(3, 7), 100),
    "sitting_box_ds": (lambda: scene("floating_sitting_box.xml", 2, 1, iters=0), 25),
    "sitting_box_noslip": (lambda: scene("floating_sitting_box.xml", 3, 2, iters=10, mu=100.0, eps=0.3), 60),
    "table_noslip": (lambda: scene("floating_box_table.xml", 4, 3), 100),
    "table_ds": (lambda: scene("floating_box_table.xml", 3, 4, iters=0, mu=0.5, nk=4), 100),
    "arm_box_foot": (lambda: scene("arm_with_box_foot_urdf.xml", 6, 5, iters=10), 100),
    "mixed": (lambda: mixed(3, 6), 60),
}


def virtual_drive(rng, B, nj, rows):
    sh = (rows, B, nj)
    return A.Drive(kp=rng.uniform(0.0, 3.0, (B, nj)), kv=rng.uniform(0.0, 0.3, (B, nj)), q_des=rng.uniform(-0.3, 0.3, sh),
                   qd_des=rng.uniform(-0.5, 0.5, sh), tau_ff=rng.uniform(-1.0, 1.0, sh))


def run(box_ref, name, coords, driven, stab):
    build, n = CASES[name]
    m, q0, qd0, dt = build()
    if not stab: m.cstab_max_iterations = 0
    elif m.cstab_max_iterations == 0: m.cstab_max_iterations = 10
    B, nj = q0.shape
    pose = coords == "pose"
    ab = A.ArticBatch(m, np.zeros_like(q0), np.zeros_like(qd0), base_coords=coords)
    ab.upload(q0, qd0, S.new_aux(B))
    P = ab.base_pose() if pose else None
    q, qd, aux = q0.copy(), qd0.copy(), S.new_aux(B)
    rng = np.random.default_rng(len(name))
    for launch in range(2):
        d = virtual_drive(rng, B, nj, rows=1 if launch == 0 else n) if driven else None
        ab.step(dt, n, drive=d)
        box_ref.step(m, q, qd, aux, dt, n, pose=P, drive=d)
        q_g, qd_g, aux_g = ab.download()
        same((q_g, qd_g, aux_g), (q, qd, aux), B)
        if pose:
            assert np.array_equal(ab.base_pose(), P), "max |dP| = %.3e" % np.nanmax(np.abs(ab.base_pose() - P))
    ab.close()
    return aux


@pytest.mark.parametrize("stab", [False, True])
@pytest.mark.parametrize("driven", [False, True])
@pytest.mark.parametrize("name,coords", [(n, c) for n in CASES for c in ("angles", "pose") if not (c == "pose" and n == "arm_box_foot")])
def test_box_kernels_match_the_reference(box_ref, name, coords, driven, stab):
    """test 6: k_artic_step_box[_stab][_pose][_drive] -- all eight -- on the free box (Drumwright-Shell and no-slip), the welded table, a
    fixed-base arm with a box foot (angle coordinates only: pose coordinates need a floating base), a sphere-and-box body: two launches, a
    held drive row then a row per step"""
    aux = run(box_ref, name, coords, driven, stab)
    assert (aux["lcp_solves"] > 0).any(), "no contact was resolved"
    if name == "four_feet_noslip":
        assert (aux["lcp_rows"] > 8 * aux["lcp_solves"]).any(), "never more than 8 rows"     # (with a drive, some solves have fewer than 16)


SPHERE_SCENES = {  # sphere-only scenes through both kernel sets
    "spinning_ball": ("floating_spinning_ball.xml", 4, None, 40, None),
    "welded_pair": ("floating_welded_pair.xml", 4, None, 250, None),
    "arm_on_table": ("arm_on_table.xml", 4, None, 400, 10),
}


@pytest.mark.parametrize("name", list(SPHERE_SCENES))
def test_forced_box_kernels_equal_the_sphere_kernels(name):
    """test 7: mh_debug_set(12, 1) sends sphere-only models through the box kernels: bit for bit today's sphere kernels"""
    f, B, dt_, n, iters = SPHERE_SCENES[name]
    m, _, _, q0, qd0, dt = A.load_xml(os.path.join(SCENES, f))
    if iters is not None: m.cstab_max_iterations = iters
    dt = dt_ or dt
    rng = np.random.default_rng(3)
    q = np.tile(q0, (B, 1)) + rng.uniform(-0.05, 0.05, (B, m.nj)); qd = np.tile(qd0, (B, 1)) + rng.uniform(-0.5, 0.5, (B, m.nj))
    lib = _lib.load()
    out = []
    for key in (0, 1):
        _lib.check(lib.mh_debug_set(12, key))
        try:
            ab = A.ArticBatch(m, q, qd, S.new_aux(B))
            ab.step(dt, n)
            out.append(ab.download())
            ab.close()
        finally:
            _lib.check(lib.mh_debug_set(12, 0))
    same(out[1], out[0], B)
    assert (out[0][2]["lcp_solves"] > 0).any()


def test_over_capacity_ends_where_the_reference_does(box_ref):
    """test 7: five flat box feet under the no-slip model (20 vertex contacts > MH_NOSLIP_MAX) -> MH_WORLD_UNSUPPORTED at the same step as the
    reference, and the run ends there"""
    m = A.model_from_links([], gravity=(0.0, -9.81, 0.0), floating_base=dict(R0=np.eye(3), x0=(0.0, 0.06, 0.0), mass=5.0, inertia=np.diag([1.0, 1.0, 1.0])))
    feet = [(5, (x, -0.05, z), np.eye(3), (0.1, 0.02, 0.1)) for x, z in ((-0.4, -0.4), (0.4, -0.4), (-0.4, 0.4), (0.4, 0.4), (0.0, 0.0))]
    A.add_boxes(m, feet, plane_normal=(0.0, 1.0, 0.0), mu_coulomb=100.0)
    B = 2
    q = np.zeros((B, 6)); qd = np.zeros((B, 6)); qd[1, 1] = -0.5
    ab = A.ArticBatch(m, q, qd, S.new_aux(B))
    ab.step(1e-3, 80)
    got = ab.download(); ab.close()
    ref = [q.copy(), qd.copy(), S.new_aux(B)]
    box_ref.step(m, ref[0], ref[1], ref[2], 1e-3, 80)
    same(got, tuple(ref), B)
    assert (ref[2]["status"] & S.MH_WORLD_UNSUPPORTED).all()
    assert (ref[2]["steps"] < 80).all()
