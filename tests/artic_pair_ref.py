"""The pair reference's ctypes face (tests/native/artic_pair_ref.cpp), shared by the CPU and the GPU tests of sphere contacts between links."""
import ctypes

import numpy as np

from moby_amd import artic as A
from moby_amd import scene as S
from tests import native_build



class PairRef:
    """ctypes face of tests/native/artic_pair_ref.cpp"""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.artic_pair_ref_step.restype = None
        self.lib.artic_pair_ref_ca.restype = ctypes.c_int
        self.lib.artic_pair_ref_dist.restype = ctypes.c_int

    def step(self, model, q, qd, aux, dt, nsteps, pose=None, drive=None):
        keep = None
        d = None
        if drive is not None:
            drive.check(q.shape[0], model.nj)
            d = A.mh_artic_drive(terms=drive.terms, rows=drive.rows)
            keep = {k: np.ascontiguousarray(a, dtype=np.float64) for k, a in drive.arrays.items() if a is not None}
            for k, a in keep.items():
                setattr(d, k, a.ctypes.data)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self.lib.artic_pair_ref_step(ctypes.byref(model), int(q.shape[0]), ctypes.c_double(dt), int(nsteps), P(q), P(qd), P(aux),
                                    None if pose is None else P(pose), None if d is None else ctypes.byref(d))
        del keep

    def ca(self, model, q, qd):
        """the conservative-advancement bounds of one state: unmasked spheres, boxes, pairs"""
        q = np.ascontiguousarray(q, dtype=np.float64).copy(); qd = np.ascontiguousarray(qd, dtype=np.float64).copy()
        out = np.zeros(32)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        n = self.lib.artic_pair_ref_ca(ctypes.byref(model), P(q), P(qd), P(out))
        return out[:n]

    def dist(self, model, q):
        """the pairs' signed distances of every world of q (B x nj) -> B x npairs"""
        out = np.zeros((q.shape[0], max(model.npairs, 1)))
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        for b in range(q.shape[0]):
            qb = np.ascontiguousarray(q[b], dtype=np.float64).copy(); z = np.zeros_like(qb)
            self.lib.artic_pair_ref_dist(ctypes.byref(model), P(qb), P(z), P(out[b]))
        return out[:, :model.npairs]


def build_pair_ref():
    return PairRef(native_build.build(("artic_pair_ref.cpp", "artic_box_ref.cpp", "artic_drive_ref.cpp", "artic_pose_ref.cpp"), "artic_pair_ref"))


# ---- scenes shared by the CPU and the GPU tests (gravity along -y, the plane y = 0 unless stated) ----
G = (0.0, -9.81, 0.0)
UP = (0.0, 1.0, 0.0)


def _hinge(parent, x0, com, mass=0.5, lo=None, hi=None, restitution=0.0):
    L = dict(parent=parent, type=A.MH_JOINT_REVOLUTE, R0=np.eye(3), x0=x0, axis=(0.0, 0.0, 1.0), com=com, inertia=np.eye(3) * 0.01, mass=mass,
             restitution=restitution)
    if lo is not None: L["lo"] = lo
    if hi is not None: L["hi"] = hi
    return L


def slider(x0, axis, mass=1.0, inertia=0.4):
    return dict(parent=-1, type=A.MH_JOINT_PRISMATIC, R0=np.eye(3), x0=x0, axis=axis, com=(0.0, 0.0, 0.0), inertia=np.eye(3) * inertia, mass=mass)


def arm_self(B, seed, mu=100.0, eps=0.3, iters=10):
    """a three-link planar arm on a fixed base whose tip sphere can fold back onto a sphere on its first link, and reach the plane"""
    links = [_hinge(-1, (0.0, 1.0, 0.0), (0.2, 0.0, 0.0)), _hinge(0, (0.4, 1.0, 0.0), (0.2, 0.0, 0.0), lo=-2.6, hi=2.6, restitution=0.2),
             _hinge(1, (0.8, 1.0, 0.0), (0.2, 0.0, 0.0), lo=-2.6, hi=2.6, restitution=0.2)]
    m = A.model_from_links(links, gravity=G)
    A.add_spheres(m, [(0, (0.1, 0.0, 0.0), 0.08), (2, (0.4, 0.0, 0.0), 0.08)], plane_normal=UP, epsilon=eps, mu_coulomb=mu)
    A.add_pairs(m, [(1, 0)], no_plane=(0,))
    m.cstab_max_iterations = iters
    rng = np.random.default_rng(seed)
    q = rng.uniform(-1.2, 1.2, (B, 3)); qd = rng.uniform(-2.0, 2.0, (B, 3))
    sg = rng.choice([-1.0, 1.0], B)                                # folded most of the way, and folding on
    q[:, 1] = sg * rng.uniform(1.6, 1.85, B); q[:, 2] = sg * rng.uniform(1.9, 2.15, B)
    qd[:, 1:] = sg[:, None] * rng.uniform(1.0, 4.0, (B, 2))
    return m, q, qd, 1e-3


def arm_pendulum(B, seed, mu=100.0, eps=0.3, iters=10):
    """two roots in one model: a two-link arm whose tip sphere swings into the bob of a pendulum hanging beside it; the bob never meets the plane"""
    links = [_hinge(-1, (0.0, 1.0, 0.0), (0.25, 0.0, 0.0)), _hinge(0, (0.5, 1.0, 0.0), (0.25, 0.0, 0.0), lo=-2.5, hi=2.5, restitution=0.1),
             _hinge(-1, (0.9, 1.0, 0.0), (0.0, -0.6, 0.0), mass=0.8)]
    m = A.model_from_links(links, gravity=G)
    A.add_spheres(m, [(1, (0.5, 0.0, 0.0), 0.1), (2, (0.0, -0.6, 0.0), 0.1)], plane_normal=UP, epsilon=eps, mu_coulomb=mu)
    A.add_pairs(m, [(0, 1)], no_plane=(1,))
    m.cstab_max_iterations = iters
    rng = np.random.default_rng(seed)
    q = np.zeros((B, 3)); qd = np.zeros((B, 3))
    q[:, 0] = rng.uniform(-0.3, 0.1, B); q[:, 1] = rng.uniform(-0.1, 0.1, B); q[:, 2] = rng.uniform(-0.2, 0.2, B)   # the arm above the bob, swinging down
    qd[:, 0] = -rng.uniform(0.5, 3.0, B); qd[:, 1] = rng.uniform(-0.5, 0.5, B); qd[:, 2] = rng.uniform(-1.0, 1.0, B)
    return m, q, qd, 1e-3


def long_legs(B, seed, mu=100.0, eps=0.2, iters=10):
    """floating_legs with three segments per leg: 12 joints, where the pair kernels keep the C X C' blocks in the HBM workspace"""
    legs = []
    for side, x in ((0, -0.1), (1, 0.1)):
        for k in range(3):
            legs.append(_hinge(-1 if k == 0 else 3 * side + k - 1, (x, 0.5 - 0.1 * k, 0.0), (0.0, -0.05, 0.0), mass=0.1, lo=-0.4, hi=0.4, restitution=0.1))
    m = A.model_from_links(legs, gravity=G, floating_base=dict(R0=np.eye(3), x0=(0.0, 0.6, 0.0), mass=2.0, inertia=np.diag([0.2, 0.3, 0.25])))
    A.add_spheres(m, [(8, (0.0, -0.2, 0.0), 0.07), (11, (0.0, -0.2, 0.0), 0.07)], plane_normal=UP, epsilon=eps, mu_coulomb=mu)
    A.add_pairs(m, [(0, 1)])
    m.cstab_max_iterations = iters
    rng = np.random.default_rng(seed)
    q = np.zeros((B, 12)); qd = np.zeros((B, 12))
    q[:, 1] = rng.uniform(0.0, 0.1, B); q[:, 3:6] = rng.uniform(-0.15, 0.15, (B, 3)); q[:, 6] = -rng.uniform(0.0, 0.1, B); q[:, 9] = rng.uniform(0.0, 0.1, B)
    qd[:, :3] = rng.uniform(-0.5, 0.5, (B, 3)); qd[:, 3:6] = rng.uniform(-1.0, 1.0, (B, 3)); qd[:, 6] = rng.uniform(1.0, 3.0, B); qd[:, 9] = -rng.uniform(1.0, 3.0, B)
    qd[:, [7, 8, 10, 11]] = rng.uniform(-1.0, 1.0, (B, 4))
    return m, q, qd, 1e-3


def floating_legs(B, seed, mu=100.0, eps=0.2, iters=10):
    """a floating base with two hinged legs whose foot spheres can touch each other and the plane"""
    legs = [_hinge(-1, (-0.1, 0.5, 0.0), (0.0, -0.2, 0.0), mass=0.3, lo=-0.6, hi=0.6, restitution=0.1),
            _hinge(-1, (0.1, 0.5, 0.0), (0.0, -0.2, 0.0), mass=0.3, lo=-0.6, hi=0.6, restitution=0.1)]
    m = A.model_from_links(legs, gravity=G, floating_base=dict(R0=np.eye(3), x0=(0.0, 0.6, 0.0), mass=2.0, inertia=np.diag([0.2, 0.3, 0.25])))
    A.add_spheres(m, [(6, (0.0, -0.4, 0.0), 0.07), (7, (0.0, -0.4, 0.0), 0.07)], plane_normal=UP, epsilon=eps, mu_coulomb=mu)
    A.add_pairs(m, [(0, 1)])
    m.cstab_max_iterations = iters
    rng = np.random.default_rng(seed)
    q = np.zeros((B, 8)); qd = np.zeros((B, 8))
    q[:, 1] = rng.uniform(0.0, 0.1, B); q[:, 3:6] = rng.uniform(-0.15, 0.15, (B, 3)); q[:, 6] = -rng.uniform(0.0, 0.1, B); q[:, 7] = rng.uniform(0.0, 0.1, B)
    qd[:, :3] = rng.uniform(-0.5, 0.5, (B, 3)); qd[:, 3:6] = rng.uniform(-1.0, 1.0, (B, 3)); qd[:, 6] = rng.uniform(1.0, 3.0, B); qd[:, 7] = -rng.uniform(1.0, 3.0, B)
    return m, q, qd, 1e-3


def mixed_box(B, seed, mu=100.0, eps=0.3, iters=10):
    """a floating box with a hinged arm whose tip carries a sphere, and a pendulum on a second root whose bob that sphere can hit: plane contacts of
    a sphere and a box, and a pair, in one list; the second root does not ride on the floating base"""
    arm = _hinge(-1, (0.3, 0.4, 0.0), (0.2, 0.0, 0.0), mass=0.3, lo=-0.8, hi=0.8, restitution=0.2)
    pend = _hinge(-1, (0.85, 0.9, 0.0), (0.0, -0.5, 0.0), mass=0.5)
    m = A.model_from_links([arm, pend], gravity=G, floating_base=dict(R0=np.eye(3), x0=(0.0, 0.4, 0.0), mass=2.0, inertia=np.diag([0.2, 0.3, 0.25])))
    m.parent[7] = -1                                               # the pendulum hangs from the world (R0 = identity: Rrel stays, trel = its x0)
    for k, v in enumerate((0.85, 0.9, 0.0)): m.trel[7][k] = v
    A.add_spheres(m, [(6, (0.4, 0.0, 0.0), 0.05), (7, (0.0, -0.5, 0.0), 0.08)], plane_normal=UP, epsilon=eps, mu_coulomb=mu)
    A.add_boxes(m, [(5, (0.0, 0.0, 0.0), np.eye(3), (0.4, 0.3, 0.35))], plane_normal=UP, epsilon=eps, mu_coulomb=mu)
    A.add_pairs(m, [(0, 1)], no_plane=(1,))
    m.cstab_max_iterations = iters
    rng = np.random.default_rng(seed)
    q = np.zeros((B, 8)); qd = np.zeros((B, 8))
    q[:, 1] = rng.uniform(0.0, 0.05, B); q[:, 3:6] = rng.uniform(-0.05, 0.05, (B, 3)); q[:, 6] = rng.uniform(-0.2, 0.1, B); q[:, 7] = rng.uniform(0.0, 0.3, B)
    qd[:, :3] = rng.uniform(-0.3, 0.3, (B, 3)); qd[:, 3:6] = rng.uniform(-1, 1, (B, 3)); qd[:, 7] = -rng.uniform(0.5, 2.0, B)   # the bob swings back onto the tip
    return m, q, qd, 1e-3


def sphere_stack(heights=(1.0, 3.0, 5.0), iters=None):
    """example/stacks/sphere-stack.xml as three vertical sliders: unit spheres of mass 1 (J = 0.4), gravity along -z, the plane z = 0, epsilon 0,
    mu 0, 16 cone edges; sphere 0 meets the plane, pairs (1, 0) and (2, 1)"""
    m = A.model_from_links([slider((0.0, 0.0, h), (0.0, 0.0, 1.0)) for h in heights], gravity=(0.0, 0.0, -9.81))
    A.add_spheres(m, [(k, (0.0, 0.0, 0.0), 1.0) for k in range(3)], plane_normal=(0.0, 0.0, 1.0), epsilon=0.0, mu_coulomb=0.0, nk=16)
    A.add_pairs(m, [(1, 0), (2, 1)], no_plane=(1, 2))
    m.cstab_max_iterations = S.MH_CSTAB_DEFAULT_MAX_ITERATIONS if iters is None else iters
    return m
