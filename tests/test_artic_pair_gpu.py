"""Sphere contacts between links on the GPU (include/moby_hip_artic.h, mh_artic_model.npairs / sphere_no_plane): the eight pair kernels of
mh_artic_pair.hip / mh_artic_pair_pose.hip against the pair reference (tests/native/artic_pair_ref.cpp) bit for bit -- q, qd, every aux field,
vns / zlast up to their sizes and, in pose coordinates, the base pose -- and the forced pair kernels (mh_debug_set key 13) against the box and
the sphere kernels."""
import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import artic as A
from moby_amd import scene as S
from tests import artic_pair_ref as P
from tests.test_artic_box_gpu import CASES as BOX_CASES, SPHERE_SCENES, same, virtual_drive

pytestmark = pytest.mark.gpu
B = 64


@pytest.fixture(scope="module")
def pair_ref():
    return P.build_pair_ref()


SCENES = {  # name -> (builder, steps per launch, has a floating base)
    "arm_self": (P.arm_self, 150, False),
    "arm_pendulum": (P.arm_pendulum, 150, False),
    "floating_legs": (P.floating_legs, 100, True),
    "mixed_box": (P.mixed_box, 100, True),
    "long_legs": (P.long_legs, 100, True),        # 12 joints: the C X C' blocks in the HBM workspace
}


def run(pair_ref, name, coords, driven, stab, mu, algorithm):
    build, n, _ = SCENES[name]
    m, q0, qd0, dt = build(B, len(name), mu=mu) if mu >= 100.0 else build(B, len(name), mu=mu, eps=0.2)
    m.cstab_max_iterations = 10 if stab else 0
    m.algorithm = algorithm
    nj = q0.shape[1]
    pose = coords == "pose"
    ab = A.ArticBatch(m, np.zeros_like(q0), np.zeros_like(qd0), base_coords=coords)
    ab.upload(q0, qd0, S.new_aux(B))
    Pp = ab.base_pose() if pose else None
    q, qd, aux = q0.copy(), qd0.copy(), S.new_aux(B)
    rng = np.random.default_rng(len(name))
    for launch in range(2):
        d = virtual_drive(rng, B, nj, rows=1 if launch == 0 else n) if driven else None
        ab.step(dt, n, drive=d)
        pair_ref.step(m, q, qd, aux, dt, n, pose=Pp, drive=d)
        got = ab.download()
        same(got, (q, qd, aux), B)
        if pose:
            assert np.array_equal(ab.base_pose(), Pp), "max |dP| = %.3e" % np.nanmax(np.abs(ab.base_pose() - Pp))
    ab.close()
    return aux


@pytest.mark.parametrize("algorithm", [A.MH_ARTIC_CRB, A.MH_ARTIC_FSAB])
@pytest.mark.parametrize("mu", [100.0, 0.5])
@pytest.mark.parametrize("stab", [False, True])
@pytest.mark.parametrize("driven", [False, True])
@pytest.mark.parametrize("name,coords", [(n, c) for n in SCENES for c in ("angles", "pose") if c == "angles" or SCENES[n][2]])
def test_pair_kernels_match_the_reference(pair_ref, name, coords, driven, stab, mu, algorithm):
    """test 8: k_artic_step_pair[_stab][_pose][_drive] -- all eight -- on the self-colliding arm, the arm and the pendulum on two roots, the
    floating base with two legs (angles and pose), the mixed body with a box and a second root (angles and pose); the no-slip and the
    Drumwright-Shell model; CRB and FSAB; 64 perturbed starts; two launches, a held drive row then a row per step"""
    aux = run(pair_ref, name, coords, driven, stab, mu, algorithm)
    assert (aux["lcp_solves"] > 0).any(), "no contact was resolved"


def _both(m, q, qd, dt, n, keys):
    lib = _lib.load()
    out = []
    nB = q.shape[0]
    for key13 in (0, 1):
        for k, v in keys: _lib.check(lib.mh_debug_set(k, v))
        _lib.check(lib.mh_debug_set(13, key13))
        try:
            ab = A.ArticBatch(m, q, qd, S.new_aux(nB))
            ab.step(dt, n); ab.step(dt, n)                              # two launches, as the box tests run their scenes (some land in the second)
            out.append(ab.download())
            ab.close()
        finally:
            _lib.check(lib.mh_debug_set(13, 0))
            for k, _ in keys: _lib.check(lib.mh_debug_set(k, 0))
    same(out[1], out[0], nB)
    assert (out[0][2]["lcp_solves"] > 0).any()


@pytest.mark.parametrize("name", list(SPHERE_SCENES))
def test_forced_pair_kernels_equal_the_sphere_kernels(name):
    """test 9: mh_debug_set(13, 1) sends sphere-only models through the pair kernels: bit for bit the sphere kernels"""
    import os
    from tests.test_artic_box_gpu import SCENES as DIR
    f, nB, dt_, n, iters = SPHERE_SCENES[name]
    m, _, _, q0, qd0, dt = A.load_xml(os.path.join(DIR, f))
    if iters is not None: m.cstab_max_iterations = iters
    rng = np.random.default_rng(3)
    q = np.tile(q0, (nB, 1)) + rng.uniform(-0.05, 0.05, (nB, m.nj)); qd = np.tile(qd0, (nB, 1)) + rng.uniform(-0.5, 0.5, (nB, m.nj))
    _both(m, q, qd, dt_ or dt, n, [])


@pytest.mark.parametrize("name", list(BOX_CASES))
def test_forced_pair_kernels_equal_the_box_kernels(name):
    """test 9: ... and box models: bit for bit the box kernels"""
    build, n = BOX_CASES[name]
    m, q, qd, dt = build()
    _both(m, q, qd, dt, n, [])


def test_over_capacity_ends_where_the_reference_does(pair_ref):
    """test 10: four box feet (16 vertex contacts) and a pair contact under the no-slip model exceed MH_NOSLIP_MAX: MH_WORLD_UNSUPPORTED at the
    same step as the reference, and the run ends there"""
    legs = [P._hinge(-1, (-0.03, 0.2, 0.0), (0.0, 0.1, 0.0), mass=0.2, lo=-0.5, hi=0.5), P._hinge(-1, (0.03, 0.2, 0.0), (0.0, 0.1, 0.0), mass=0.2, lo=-0.5, hi=0.5)]
    m = A.model_from_links(legs, gravity=P.G, floating_base=dict(R0=np.eye(3), x0=(0.0, 0.06, 0.0), mass=5.0, inertia=np.eye(3)))
    feet = [(5, (x, -0.05, z), np.eye(3), (0.1, 0.02, 0.1)) for x, z in ((-0.4, -0.4), (0.4, -0.4), (-0.4, 0.4), (0.4, 0.4))]
    A.add_spheres(m, [(6, (0.0, 0.2, 0.0), 0.03), (7, (0.0, 0.2, 0.0), 0.03)], plane_normal=P.UP, mu_coulomb=100.0)
    A.add_boxes(m, feet, plane_normal=P.UP, mu_coulomb=100.0)
    A.add_pairs(m, [(0, 1)], no_plane=(0, 1))                          # the two antennae touch at q = 0 (centres 0.06 apart, radii 0.03)
    nB = 2
    q = np.zeros((nB, 8)); qd = np.zeros((nB, 8)); qd[:, 6] = -0.5; qd[:, 7] = 0.5; qd[1, 1] = -0.5
    ab = A.ArticBatch(m, q, qd, S.new_aux(nB))
    ab.step(1e-3, 80)
    got = ab.download(); ab.close()
    ref = [q.copy(), qd.copy(), S.new_aux(nB)]
    pair_ref.step(m, ref[0], ref[1], ref[2], 1e-3, 80)
    same(got, tuple(ref), nB)
    assert (ref[2]["status"] & S.MH_WORLD_UNSUPPORTED).all()
    assert (ref[2]["steps"] < 80).all()
