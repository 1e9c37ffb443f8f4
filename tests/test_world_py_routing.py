"""Which library entries moby_amd.world calls, and with what: no GPU and no library -- `_lib.load` is replaced by a recorder whose every entry returns
MH_OK and logs its name and arguments.  The C library guarantees that the entries with fewer arguments equal the general ones with NULL for what is absent
(include/moby_hip.h; tests/test_world_report.py and its neighbours check the refusals), so the Python side has one path to each."""
import ctypes
import itertools

import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import scene as S
from moby_amd import world as MW

B, NSTEPS, DT = 2, 3, 1e-3


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return _lib.MH_OK
        return entry


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: r)
    return r


def _optional(forces, statics, params):
    """the sphere stack (three spheres on the ground) with each optional record present or None"""
    sc = S.sphere_stack_scene()
    f = S.make_forces(sc.nb, stokes=(0.1, 0.01)) if forces else None
    st = S.make_statics([dict(plane=True, rpy=(0.0, 0.0, 0.3), o=(-2.0, 0.0, 0.0))]) if statics else None
    p = S.make_params(sc, st, B) if params else None
    return sc, f, st, p


@pytest.mark.parametrize("forces,statics,params,want_report", list(itertools.product([False, True], repeat=4)))
def test_world_batch_step_is_one_call_to_the_general_entry(rec, forces, statics, params, want_report):
    sc, f, st, p = _optional(forces, statics, params)
    npt = 10 if statics else 6                    # triangular over 3 spheres + ground (+ the static): C(5, 2) or C(4, 2)
    for want_traj in (False, True):
        wb = MW.WorldBatch(sc, S.sphere_stack_state(B), forces=f, statics=st, params=p)
        del rec.calls[:]
        out = wb.step(DT, NSTEPS, want_traj=want_traj, want_report=want_report)
        assert [c[0] for c in rec.calls] == ["mh_world_step_batch_report"]
        a_scene, a_forces, a_statics, a_params, a_B, a_dt, a_nsteps, a_state, a_aux, a_traj, a_report = rec.calls[0][1]
        assert a_scene == ctypes.addressof(sc) and (a_B, a_dt, a_nsteps) == (B, DT, NSTEPS)
        assert a_state == wb.state.ctypes.data and a_aux == wb.aux.ctypes.data
        assert a_forces == (ctypes.addressof(f) if forces else None)
        assert a_statics == (ctypes.addressof(st) if statics else None)
        assert a_params == (wb.params.ctypes.data if params else None)
        traj, report = out if want_report else (out, None)
        assert isinstance(out, tuple) == want_report
        assert (a_traj is None) == (not want_traj) and (traj is None) == (not want_traj)
        assert (a_report is None) == (not want_report)
        if want_traj:
            assert a_traj == traj.ctypes.data and traj.shape == (B, NSTEPS, sc.nb, 7) and traj.dtype == np.float64
        if want_report:
            assert a_report == report.ctypes.data and report.shape == (B, NSTEPS, npt, 8) and report.dtype == np.float64


@pytest.mark.parametrize("statics,params,report", list(itertools.product([False, True], repeat=3)))
def test_world_batch_device_creates_through_the_two_general_entries(rec, statics, params, report):
    sc, _, st, p = _optional(False, statics, params)
    dev = MW.WorldBatchDevice(sc, S.sphere_stack_state(B), statics=st, params=p, report=report)
    names = [c[0] for c in rec.calls]
    assert names == ["mh_world_batch_create_report" if report else "mh_world_batch_create_params", "mh_world_batch_device", "mh_world_batch_upload"]
    a_scene, a_statics, a_params, a_B, _handle = rec.calls[0][1]
    assert a_scene == ctypes.addressof(sc) and a_B == B
    assert a_statics == (ctypes.addressof(st) if statics else None)
    assert (a_params is None) == (not params)
    assert dev.npt == (10 if statics else 6)


def test_world_batch_device_stepping_entries(rec):
    sc = S.sphere_stack_scene()
    dev = MW.WorldBatchDevice(sc, S.sphere_stack_state(B))
    del rec.calls[:]
    dev.step_ids(DT, NSTEPS, 4096, 1)             # without a wrench or a report: its own entry, whose refusals are worded its own way
    assert [c[0] for c in rec.calls] == ["mh_world_batch_step_ids"]
    _h, a_stream, a_dt, a_nsteps, a_ids, a_count = rec.calls[0][1]
    assert (a_stream, a_dt, a_nsteps, a_ids.value, a_count) == (None, DT, NSTEPS, 4096, 1)
    del rec.calls[:]
    dev.step(DT, NSTEPS, traj_ptr=8192)           # the general entry: no ids, no wrench (one row), no report
    dev.step_ids(DT, NSTEPS, 4096, 1, wrench=12288, rows=NSTEPS)
    assert [c[0] for c in rec.calls] == ["mh_world_batch_step_report"] * 2
    assert rec.calls[0][1][2:] == (DT, NSTEPS, 8192, None, 0, None, 1, None)
    _h, _s, a_dt, a_nsteps, a_traj, a_ids, a_count, a_wrench, a_rows, a_report = rec.calls[1][1]
    assert (a_dt, a_nsteps, a_traj, a_ids.value, a_count, a_wrench.value, a_rows, a_report) == (DT, NSTEPS, None, 4096, 1, 12288, NSTEPS, None)
