"""TEST INFRASTRUCTURE: the one ctypes face of the world reference (tests/native/world_ref.cpp), built once per process.  The scenes, the batches and
their reference runs live with their features: tests/world_force_ref.py, world_boxsphere_ref.py, world_statics_ref.py, world_params_ref.py,
world_report_ref.py."""
import collections
import ctypes
import functools

import numpy as np

from moby_amd import scene as S
from tests import native_build

REPORT_PAIR = 8
# what a run hands back beside the state and the records it steps in place; a part that was not asked for is None
Result = collections.namedtuple("Result", "traj census report shape")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _vec(a, n):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    assert a.shape == (n,)
    return a


def npt_of(sc, stt):
    """the pair slots of a scene and its statics (or None)"""
    ntot = sc.nb + sc.has_ground + (stt.n if stt is not None else 0)
    return ntot * (ntot - 1) // 2


class WorldRef:
    """ctypes face of tests/native/world_ref.cpp"""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        for f in ("step", "box_contact", "box_dist", "contact", "dist", "pair"):
            getattr(self.lib, "world_ref_" + f).restype = None

    def step(self, sc, state, aux, dt, nsteps, statics=None, forces=None, wrench=None, want_traj=False, want_census=False, want_report=False, want_shape=False):
        """B worlds x nsteps in place.  statics: S.mh_world_statics or None; forces: S.mh_world_forces or None; wrench: (B, nb, 6) or (rows, B, nb, 6) host
        array or None (forces and wrench both None: the oracle's own forward dynamics).  -> Result(trajectory (B, nsteps, nb, 7), region census
        (B, nsteps, 5), report (B, nsteps, npt, 8), shape census (B, nsteps, 6; filled only beside a report)), each None unless wanted"""
        B = state.shape[0]
        traj = np.zeros((B, nsteps, sc.nb, 7)) if want_traj else None
        census = np.zeros((B, nsteps, 5), dtype=np.int32) if want_census else None
        report = np.full((B, nsteps, npt_of(sc, statics), REPORT_PAIR), np.nan) if want_report else None      # (the entry writes it whole)
        shape = np.zeros((B, nsteps, 6), dtype=np.int32) if want_shape else None
        w, rows = None, 1
        if wrench is not None:
            w = np.ascontiguousarray(wrench, dtype=np.float64)
            rows = 1 if w.ndim == 3 else w.shape[0]
            assert w.shape[-3:] == (B, sc.nb, 6)
        self.lib.world_ref_step(ctypes.byref(sc), None if statics is None else ctypes.byref(statics), int(B), ctypes.c_double(dt), int(nsteps), _ptr(state),
                                _ptr(aux), _ptr(traj), _ptr(census), None if forces is None else ctypes.byref(forces), _ptr(w), int(rows), _ptr(report), _ptr(shape))
        return Result(traj, census, report, shape)

    def _contact(self, fn, cb, frame, nframe, dims, cS, radius, TOL):
        out = np.zeros(9)
        fn(_ptr(_vec(cb, 3)), _ptr(_vec(frame, nframe)), _ptr(_vec(dims, 3)), _ptr(_vec(cS, 3)), ctypes.c_double(radius), ctypes.c_double(TOL), _ptr(out))
        return dict(has=int(out[0]), dist=out[1], point=out[2:5].copy(), normal=out[5:8].copy(), region=int(out[8]))

    def _dist(self, fn, cb, frame, nframe, dims, cS, radius):
        out = np.zeros(7)
        fn(_ptr(_vec(cb, 3)), _ptr(_vec(frame, nframe)), _ptr(_vec(dims, 3)), _ptr(_vec(cS, 3)), ctypes.c_double(radius), _ptr(out))
        return out[0], out[1:4].copy(), out[4:7].copy()

    def box_contact(self, cb, R, dims, cS, radius, TOL):
        """-> dict(has, dist, point, normal, region) of a box (centre, axes R row-major, edge lengths) and a sphere"""
        return self._contact(self.lib.world_ref_box_contact, cb, R, 9, dims, cS, radius, TOL)

    def box_dist(self, cb, R, dims, cS, radius):
        """-> (signed distance, box point, sphere point)"""
        return self._dist(self.lib.world_ref_box_dist, cb, R, 9, dims, cS, radius)

    def contact(self, cb, quat, dims, cS, radius, TOL):
        """box_contact over a box body's pose (centre, quaternion xyzw): the axes are the stepper's own (World::rot)"""
        return self._contact(self.lib.world_ref_contact, cb, quat, 4, dims, cS, radius, TOL)

    def dist(self, cb, quat, dims, cS, radius):
        """box_dist over a box body's pose (centre, quaternion xyzw)"""
        return self._dist(self.lib.world_ref_dist, cb, quat, 4, dims, cS, radius)

    def pair(self, sc, state, p, TOL, statics=None):
        """pair p of a scene (and its statics) in one world's state, as the stepper reads it -> dict(dist, pa, pb, a, b, ncontacts, g1, g2, cdist, point,
        normal, kept: the broad phase keeps the pair)"""
        out = np.zeros(20)
        st = np.ascontiguousarray(state, dtype=np.float64).ravel()
        assert st.size == sc.nb * S.MH_BODY_STATE
        self.lib.world_ref_pair(ctypes.byref(sc), None if statics is None else ctypes.byref(statics), _ptr(st), int(p), ctypes.c_double(TOL), _ptr(out))
        return dict(dist=out[0], pa=out[1:4].copy(), pb=out[4:7].copy(), a=int(out[7]), b=int(out[8]), ncontacts=int(out[9]), g1=int(out[10]), g2=int(out[11]),
                    cdist=out[12], point=out[13:16].copy(), normal=out[16:19].copy(), kept=int(out[19]))


@functools.lru_cache(maxsize=None)
def reference():
    return WorldRef(native_build.build(("world_ref.cpp",), "world_ref"))


def run_ref(sc, st, dt, nsteps, seed=1, aux=None, **kw):
    """the reference on copies (aux: the records to start from; None = fresh ones from `seed`) -> (state, aux, Result)"""
    s2 = np.array(st, dtype=np.float64, copy=True)
    a2 = S.new_aux(s2.shape[0], seed) if aux is None else aux.copy()
    return s2, a2, reference().step(sc, s2, a2, dt, nsteps, **kw)


def assert_aux_equal(a, b):
    """complete records: rand ring, time, status, every counter, zlast / zbuf / vns with their sizes"""
    for f in S.AUX_DTYPE.names:
        if f in ("zlast", "zbuf", "vns", "pad0"):
            continue
        np.testing.assert_array_equal(a[f], b[f], err_msg=f)
    for w in range(len(b)):
        for arr, n in (("zlast", "zlast_size"), ("zbuf", "zbuf_cap"), ("vns", "vns_size")):
            k = int(b[n][w])
            np.testing.assert_array_equal(a[arr][w, :k], b[arr][w, :k], err_msg="%s of world %d" % (arr, w))
