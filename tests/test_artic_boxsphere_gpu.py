"""Box-sphere contacts between links and static boxes on the GPU (include/moby_hip_artic.h, mh_artic_model.pair_kind, box_link = -1): the eight
kernels of mh_artic_bsp.hip / mh_artic_bsp_pose.hip against the box-sphere reference (tests/native/artic_boxsphere_ref.cpp) bit for bit -- q,
qd, every aux field with the rand() ring and the counters, vns / zlast up to their sizes and, in pose coordinates, the base pose -- the forced
kernels (mh_debug_set key 14) against the pair, box and sphere kernels, the refusals of mh_artic_batch_create, and a world over capacity.

The parametrisation is lean on purpose (the -m gpu suite has a time limit): every scene runs the four angle-coordinate kernels, scenes with a
floating base the four pose kernels too; the impact model and the dynamics algorithm alternate over the cases so that both are run by every
kernel family, and the slider scene runs both models in full."""
import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import artic as A
from moby_amd import scene as S
from tests import artic_boxsphere_ref as BS
from tests import artic_pair_ref as P
from tests.test_artic_box_gpu import CASES as BOX_CASES, SPHERE_SCENES, same, virtual_drive

pytestmark = pytest.mark.gpu
B = 64


@pytest.fixture(scope="module")
def ref():
    return BS.build_boxsphere_ref()


SCENES = {  # name -> (steps per launch, has a floating base)
    "arm_static": (100, False),
    "arm_slider_box": (60, False),
    "floating_box_pendulum": (100, True),
    "mixed_all": (100, True),
    "long_arm_static": (100, False),              # 12 joints: the C X C' blocks in the HBM workspace
}
_states = {}


def states(ref, name):
    """the scene's 64 initial states, aimed with the reference (BS.aim) -- and, once per scene, the proof from the reference's own run that they
    exercise what they are for: a world that makes a face contact, one an edge contact, one a vertex contact, none with a sphere's centre
    inside a box"""
    if name not in _states:
        m, sampler, dt = BS.SCENES[name]()
        q, qd = BS.aim(ref, m, sampler, B, len(name))
        touched, _, _, aux, _ = BS.track(ref, m, q, qd, dt, 2 * SCENES[name][0])
        n = touched.sum(axis=0)
        print("%s: worlds touching a face / an edge / a vertex / with a centre inside: %r" % (name, n.tolist()))
        assert n[BS.FACE] >= 1 and n[BS.EDGE] >= 1 and n[BS.VERTEX] >= 1, "the scene no longer reaches every region: %r" % n.tolist()
        assert n[BS.INSIDE] == 0, "a sphere's centre entered a box"
        assert (aux["lcp_solves"] > 0).any()
        _states[name] = (q, qd)
    return _states[name][0].copy(), _states[name][1].copy()


def run(ref, name, coords, driven, stab, mu, algorithm):
    n = SCENES[name][0]
    m, _, dt = BS.SCENES[name](mu=mu) if mu >= 100.0 else BS.SCENES[name](mu=mu, eps=0.2)
    q0, qd0 = states(ref, name)
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
        ref.step(m, q, qd, aux, dt, n, pose=Pp, drive=d)
        assert np.isfinite(q).all() and np.isfinite(qd).all(), "the reference met a NaN normal (a sphere's centre inside a box)"
        reg, _ = ref.regions(m, q, Pp)
        assert not (reg == BS.INSIDE).any()
        got = ab.download()
        same(got, (q, qd, aux), B)
        if pose:
            assert np.array_equal(ab.base_pose(), Pp), "max |dP| = %.3e" % np.nanmax(np.abs(ab.base_pose() - Pp))
    ab.close()
    return aux


def _cases():
    out = []
    i = 0
    for name, (_, floating) in SCENES.items():
        for coords in (("angles", "pose") if floating else ("angles",)):
            for stab in (False, True):
                for driven in (False, True):
                    mus = (100.0, 0.5) if name == "arm_slider_box" else ((100.0, 0.5)[(i // 2) % 2],)
                    for mu in mus:
                        out.append((name, coords, driven, stab, mu, (A.MH_ARTIC_CRB, A.MH_ARTIC_FSAB)[i % 2]))
                        i += 1
    return out


@pytest.mark.parametrize("name,coords,driven,stab,mu,algorithm", _cases())
def test_bsp_kernels_match_the_reference(ref, name, coords, driven, stab, mu, algorithm):
    """k_artic_step_bsp[_stab][_pose][_drive] -- all eight -- on an arm over a static box, an arm over a box on a second-root slider (no-slip and
    mu = 0.5), a floating base carrying a box hit by a pendulum on a second root, the mixed model with a sphere pair, two box-sphere pairs and
    plane contacts in one list, and a 12-joint chain; CRB and FSAB; 64 worlds aimed at faces, edges and corners; two launches, a held drive row
    then a row per step"""
    aux = run(ref, name, coords, driven, stab, mu, algorithm)
    assert (aux["lcp_solves"] > 0).any(), "no contact was resolved"


def _both(m, q, qd, dt, n):
    lib = _lib.load()
    out = []
    nB = q.shape[0]
    for key14 in (0, 1):
        _lib.check(lib.mh_debug_set(14, key14))
        try:
            ab = A.ArticBatch(m, q, qd, S.new_aux(nB))
            ab.step(dt, n); ab.step(dt, n)
            out.append(ab.download())
            ab.close()
        finally:
            _lib.check(lib.mh_debug_set(14, 0))
    same(out[1], out[0], nB)
    assert (out[0][2]["lcp_solves"] > 0).any()


@pytest.mark.parametrize("name", ["arm_self", "mixed_box", "long_legs"])
def test_forced_bsp_kernels_equal_the_pair_kernels(name):
    """mh_debug_set(14, 1) sends models with sphere pairs through the box-sphere kernels: bit for bit the pair kernels"""
    m, q, qd, dt = getattr(P, name)(B, len(name))
    _both(m, q, qd, dt, 100)


@pytest.mark.parametrize("name", list(BOX_CASES)[:2])
def test_forced_bsp_kernels_equal_the_box_kernels(name):
    build, n = BOX_CASES[name]
    m, q, qd, dt = build()
    _both(m, q, qd, dt, n)


@pytest.mark.parametrize("name", list(SPHERE_SCENES)[:2])
def test_forced_bsp_kernels_equal_the_sphere_kernels(name):
    import os
    from tests.test_artic_box_gpu import SCENES as DIR
    f, nB, dt_, n, iters = SPHERE_SCENES[name]
    m, _, _, q0, qd0, dt = A.load_xml(os.path.join(DIR, f))
    if iters is not None: m.cstab_max_iterations = iters
    rng = np.random.default_rng(3)
    q = np.tile(q0, (nB, 1)) + rng.uniform(-0.05, 0.05, (nB, m.nj)); qd = np.tile(qd0, (nB, 1)) + rng.uniform(-0.5, 0.5, (nB, m.nj))
    _both(m, q, qd, dt_ or dt, n)


def _refused(m, what, match):
    with pytest.raises(_lib.MobyHipError, match=match) as e:
        A.ArticBatch(m, np.zeros((1, m.nj)), np.zeros((1, m.nj)), S.new_aux(1))
    assert e.value.code == _lib.MH_ERR_INVALID_ARG, what


def test_create_refusals():
    """mh_artic_batch_create refuses, with MH_ERR_INVALID_ARG: an unknown kind, an index outside the list the kind names, a box-sphere pair on one
    link, a pair listed twice, a static box in no pair, box_link < -1"""
    def base():
        return BS.mixed_all()[0]
    m = base(); m.pair_kind[1] = 2; _refused(m, "unknown kind", "kind 2 is not built")
    m = base(); m.pair_a[1] = 2; _refused(m, "box index", "outside the box list")
    m = base(); m.pair_b[1] = 2; _refused(m, "sphere index", "outside the sphere list")
    m = base(); m.pair_a[1] = 0; m.box_link[0] = m.sphere_link[0]; _refused(m, "one link", "sit on the same link")
    m = base(); m.pair_b[2] = 0; _refused(m, "twice", "already")
    m = base(); m.npairs = 1; _refused(m, "unpaired static box", "appears in no box-sphere pair")
    m = base(); m.box_link[1] = -2; _refused(m, "box_link", "-1 = a static box")
    m = base()                                                               # ... and the model itself is accepted
    ab = A.ArticBatch(m, np.zeros((1, 8)), np.zeros((1, 8)), S.new_aux(1)); ab.close()


def test_over_capacity_ends_where_the_reference_does(ref):
    """four box feet flat on the plane (16 vertex contacts) and a box-sphere contact under the no-slip model exceed MH_NOSLIP_MAX:
    MH_WORLD_UNSUPPORTED at the same step as the reference, and the run ends there"""
    legs = [P._hinge(-1, (0.0, 0.2, 0.0), (0.0, 0.1, 0.0), mass=0.2, lo=-0.5, hi=0.5)]
    m = A.model_from_links(legs, gravity=P.G, floating_base=dict(R0=np.eye(3), x0=(0.0, 0.06, 0.0), mass=5.0, inertia=np.eye(3)))
    feet = [(5, (x, -0.05, z), np.eye(3), (0.1, 0.02, 0.1)) for x, z in ((-0.4, -0.4), (0.4, -0.4), (-0.4, 0.4), (0.4, 0.4))]
    A.add_spheres(m, [(6, (0.0, 0.2, 0.0), 0.03)], plane_normal=P.UP, mu_coulomb=100.0)
    A.add_boxes(m, feet + [(-1, (0.08, 0.46, 0.0), np.eye(3), (0.1, 0.1, 0.1))], plane_normal=P.UP, mu_coulomb=100.0)
    A.add_box_sphere_pairs(m, [(4, 0)], no_plane=(0,))                     # the antenna's tip touches the static box's face at q = 0
    nB = 2
    q = np.zeros((nB, 7)); qd = np.zeros((nB, 7)); qd[:, 6] = -0.5; qd[1, 1] = -0.5
    ab = A.ArticBatch(m, q, qd, S.new_aux(nB))
    ab.step(1e-3, 80)
    got = ab.download(); ab.close()
    r = [q.copy(), qd.copy(), S.new_aux(nB)]
    ref.step(m, r[0], r[1], r[2], 1e-3, 80)
    same(got, tuple(r), nB)
    assert (r[2]["status"] & S.MH_WORLD_UNSUPPORTED).all()
    assert (r[2]["steps"] < 80).all()
