"""The per-pair contact impulse report of the many-worlds stepper (include/moby_hip.h, "Contact report") without a GPU: the report reference
(tests/native/world_ref.cpp with a report sink) pinned to the step without one and to the momentum balance, the conditions on the GPU cases, the refusals (they run
before the device is looked for), debug key 18 and moby_amd.world.body_impulses."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import scene as S
from moby_amd import world as MW
from tests import world_ref
from tests import world_report_ref as R
from tests import world_statics_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MH_ERR_INVALID_ARG = -1
@pytest.fixture(autouse=True)
def _the_library_has_the_report():
    lib = _lib.load()
    assert all(hasattr(lib, f) for f in ("mh_world_batch_create_report", "mh_world_batch_step_report", "mh_world_step_batch_report")), "libmoby_hip.so has no contact report"


PIN = {"corner": lambda: W.corner_batch(8) + (1e-3, 20), "mixed": lambda: W.mixed_batch(8) + (2e-3, 60), "noslip_table": lambda: W.table_batch(4, mu=100.0) + (1e-3, 20)}


@functools.lru_cache(maxsize=None)
def stepwise(name):
    """the report reference one step per call on a pin batch -> (scene, statics, states (nsteps + 1, B, nb, 13), times (nsteps + 1, B), report); checked
    against the one-call run, which is what the GPU tests compare with"""
    sc, stt, st0, dt, nsteps = PIN[name]()
    B = st0.shape[0]
    st, aux = st0.copy(), S.new_aux(B)
    states, times, rows = [st.copy()], [aux["time"].copy()], []
    for _ in range(nsteps):
        rep = world_ref.reference().step(sc, st, aux, dt, 1, statics=stt, want_report=True).report
        states.append(st.copy()); times.append(aux["time"].copy()); rows.append(rep[:, 0])
    report = np.stack(rows, axis=1)
    _, st1, aux1, rep1, _ = R.reference_run(name)
    np.testing.assert_array_equal(st1, st)
    assert aux1.tobytes() == aux.tobytes()
    np.testing.assert_array_equal(rep1, report)
    return sc, stt, np.array(states).reshape(nsteps + 1, B, sc.nb, S.MH_BODY_STATE), np.array(times), report


@pytest.mark.parametrize("name", sorted(PIN))
def test_the_report_sink_changes_no_step(name):
    """the same entry (world_ref_step) without and with a report sink: state, trajectory and the complete aux record are bit-equal, so the fold behind
    handle_impacts only reads"""
    sc, stt, st0, dt, nsteps = PIN[name]()
    st_w, aux_w, (traj_w, _, no_rep, no_shape) = world_ref.run_ref(sc, st0, dt, nsteps, statics=stt, want_traj=True)
    assert no_rep is None and no_shape is None
    st_r, aux_r, traj_r, rep, _ = R.run_ref(sc, stt, st0, dt, nsteps, want_traj=True)
    np.testing.assert_array_equal(st_r, st_w)
    np.testing.assert_array_equal(traj_r, traj_w)
    assert aux_r.tobytes() == aux_w.tobytes()
    assert np.isfinite(rep).all() and rep[..., 0].sum() > 0


@pytest.mark.parametrize("name", sorted(PIN))
def test_momentum_balance(name):
    """for every body and step, m (v_after - v_before) - m g h equals body_impulses of the step's rows, h the step's integrated time: the contact impulses
    are the only other change of momentum (the stabiliser restores the velocities), so only rounding separates the two -- 1e-9 of the largest term.  This
    pins the sign convention: a flipped sign of any pair's row doubles the difference instead of cancelling it."""
    sc, stt, states, times, report = stepwise(name)
    nb, ntot = sc.nb, sc.nb + sc.has_ground + stt.n
    m = np.array(sc.mass[:nb])[None, None, :, None]
    g = np.array(sc.gravity[:])[None, None, None, :]
    h = np.diff(times, axis=0).T[:, :, None, None]                                # (B, nsteps, 1, 1)
    v = states[:, :, :, 7:10].transpose(1, 0, 2, 3)                               # (B, nsteps + 1, nb, 3)
    dp = m * (v[:, 1:] - v[:, :-1]) - m * g * h
    imp = MW.body_impulses(report, nb, ntot)
    scale = np.maximum.reduce([np.abs(m * v[:, 1:]).max(axis=-1), np.abs(m * v[:, :-1]).max(axis=-1), np.abs(m * g * h).max(axis=-1),
                               np.abs(imp).max(axis=-1)])
    err = np.abs(dp - imp).max(axis=-1)
    assert (np.abs(imp).max(axis=-1) > 0).any()
    assert (err <= 1e-9 * scale).all(), (err / scale).max()


def test_resting_ball():
    """a ball at rest on a plane: each step the row's impulse along the plane's normal is m |g| dt, and the centre of pressure is the contact point under
    the ball -- the reference's sphere-plane contact point, midway between the ball's lowest point and the plane (CCD.inl:804-886; the stabiliser leaves the
    ball a few 1e-8 above the plane, so that point is not exactly on it)"""
    sc, stt, st0, m, r = R.resting_ball()
    dt, nsteps = 1e-3, 5
    st, aux = st0.copy(), S.new_aux(1)
    for s in range(nsteps):
        before = st[0].copy()
        rep = world_ref.reference().step(sc, st, aux, dt, 1, statics=stt, want_report=True).report
        assert aux["status"][0] == 0 and rep.shape == (1, 1, 1, 8)
        row = rep[0, 0, 0]
        assert row[0] >= 1.0 and row[1] > 0.0
        assert abs(row[3] - m * 9.81 * dt) <= 1e-9 * m * 9.81 * dt, row                  # up = +y
        np.testing.assert_allclose(row[5:8] / row[1], [before[0], 0.5 * (before[1] - r), before[2]], rtol=0, atol=1e-12)
        assert abs(before[0] - 0.5) <= 1e-12 and abs(before[1] - r) <= 1e-6 and abs(before[2] + 0.25) <= 1e-12
        assert abs(row[2]) <= 1e-9 * row[3] and abs(row[4]) <= 1e-9 * row[3]
    np.testing.assert_allclose(st[0, 7:10], 0.0, atol=1e-12)


def test_gpu_cases_contain_what_they_are_there_for():
    """(1) a pair with >= 2 contacts, (2) >= 3 loaded pairs at once, (3) >= 2 folded mini-steps with contacts in a step, (4) a restitution pass that
    added a second impulse, (5) a contact counted with zero impulse, (6) sign = -1, (7) pair slot 35 of 36 loaded -- and no world of any case carries a bit that would leave it out"""
    R.shape_conditions()
    for name in ("varied", "forced_stack"):
        R.reference_run(name)


def test_rows_of_a_passed_over_world_are_zero():
    """a world that carries MH_WORLD_LCP_FAILED is not stepped and writes zero rows"""
    sc, stt, st0 = W.corner_batch(2)
    aux = S.new_aux(2); aux["status"][1] = S.MH_WORLD_LCP_FAILED
    st, a2, _, rep, _ = R.run_ref(sc, stt, st0, 1e-3, 3, aux=aux)
    assert (rep[1] == 0.0).all() and rep[0, :, :, 0].sum() > 0 and np.array_equal(st[1], st0[1]) and a2["steps"][1] == 0


# ---- the library without a device ------------------------------------------------------------------------------------------------------------------------
def _create(entry, sc, stt, params, B):
    h = ctypes.c_void_p()
    rc = getattr(_lib.load(), entry)(ctypes.addressof(sc), None if stt is None else ctypes.addressof(stt), None if params is None else params.ctypes.data, B, ctypes.byref(h))
    msg = _lib.load().mh_last_error().decode()
    if h:
        _lib.load().mh_world_batch_destroy(h)
    return rc, msg


def test_create_report_refuses_what_create_params_refuses():
    """same return codes, same messages, before the device is looked for"""
    inputs = []
    sc, stt = W.mixed_scene_and_statics()
    for field, idx, value in (("mass", (3, 1), 0.0), ("geom_dim", (0, 1, 2), -0.5), ("gravity", (2, 1), float("inf")), ("cp_epsilon", (1, 14), float("nan")),
                              ("st_dim", (3, 1, 0), 0.0), ("st_R", (0, 0, 8), float("nan"))):
        p = S.make_params(sc, stt, 4)
        p[field][idx] = value
        inputs.append((sc, stt, p, 4))
    inputs.append((sc, stt, S.make_params(sc, stt, 1), 0))
    inputs.append((sc, stt, None, -1))
    box = W.scene([("box", (1.0, 1.0, 1.0), 1.0)], 1)
    inputs.append((box, S.make_statics([dict(box=(1.0, 1.0, 1.0), o=(0.0, -2.0, 0.0))]), None, 2))
    inputs.append((S.rimless_wheel_scene(), S.make_statics([dict(plane=True, R=W.R_UP)]), None, 2))
    bad = S.sphere_stack_scene(); bad.nb = 0
    inputs.append((bad, None, None, 2))
    for sc_, stt_, p, B in inputs:
        a = _create("mh_world_batch_create_params", sc_, stt_, p, B)
        b = _create("mh_world_batch_create_report", sc_, stt_, p, B)
        assert a == b and a[0] == MH_ERR_INVALID_ARG and a[1], (a, b)
    assert _lib.load().mh_world_batch_create_report(ctypes.addressof(sc), None, None, 2, None) == MH_ERR_INVALID_ARG


def test_step_report_validates_without_a_batch():
    lib = _lib.load()
    buf = ctypes.c_void_p(8)
    assert lib.mh_world_batch_step_report(None, None, 1e-3, 1, None, None, 0, None, 1, buf) == MH_ERR_INVALID_ARG and b"null batch" in lib.mh_last_error()
    assert lib.mh_world_batch_step_report(None, None, 1e-3, -1, None, None, 0, None, 1, buf) == MH_ERR_INVALID_ARG
    assert lib.mh_world_batch_step_report(None, None, 1e-3, 4, None, None, 0, None, 2, buf) == MH_ERR_INVALID_ARG and b"rows" in lib.mh_last_error()
    assert lib.mh_world_batch_step_report(None, None, 1e-3, 1, None, None, 0, None, 1, None) == MH_ERR_INVALID_ARG           # NULL report: mh_world_batch_step_wrench
    assert lib.mh_world_step_batch_report(None, None, None, None, 0, 1e-3, 1, None, None, None, None) == 0
    assert lib.mh_world_step_batch_report(None, None, None, None, 2, 1e-3, 1, None, None, None, buf) == MH_ERR_INVALID_ARG


def test_key_18_validates_its_values():
    lib = _lib.load()
    try:
        assert lib.mh_debug_set(18, 1) == 0 and lib.mh_debug_set(18, 0) == 0
        for v in (-1, 2, 18):
            assert lib.mh_debug_set(18, v) == MH_ERR_INVALID_ARG and b"outside {0, 1}" in lib.mh_last_error()
    finally:
        assert lib.mh_debug_set(18, 0) == 0


def test_header_macros_and_adapter_compile(tmp_path):
    src = tmp_path / "m.c"
    src.write_text('#include <stdio.h>\n#include "moby_hip.h"\nint main(void) { printf("%d %d %d\\n", MH_WORLD_REPORT, MH_REPORT_PAIR, MH_VERSION); return 0; }\n')
    exe = str(tmp_path / "m")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert subprocess.check_output([exe]).split() == [b"1", b"8", b"102"] and MW.REPORT_PAIR == 8
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", os.path.join(ROOT, "moby_amd", "cpp", "example_world.cpp")])


def test_body_impulses_on_a_hand_written_report():
    """nb = 2 bodies and a ground (ntot = 3): slots (0,1), (0,2), (1,2).  Body 0 gets +row(0,1) + row(0,2), body 1 gets -row(0,1) + row(1,2)"""
    import torch
    rep = np.zeros((2, 3, 3, 8))
    rep[1, 2, 0, 2:5] = (1.0, 2.0, 3.0)
    rep[1, 2, 1, 2:5] = (0.5, 0.25, -1.0)
    rep[1, 2, 2, 2:5] = (10.0, 20.0, 30.0)
    rep[0, 0, 2, 2:5] = (0.0, 7.0, 0.0)
    rep[..., 0] = 5.0; rep[..., 1] = 9.0; rep[..., 5:] = 4.0                      # the other entries are not looked at
    want = np.zeros((2, 3, 2, 3))
    want[1, 2, 0] = (1.5, 2.25, 2.0)
    want[1, 2, 1] = (9.0, 18.0, 27.0)
    want[0, 0, 1] = (0.0, 7.0, 0.0)
    got = MW.body_impulses(rep, 2, 3)
    assert isinstance(got, np.ndarray)
    np.testing.assert_array_equal(got, want)
    got_t = MW.body_impulses(torch.from_numpy(rep), 2, 3)
    assert isinstance(got_t, torch.Tensor) and got_t.dtype == torch.float64
    np.testing.assert_array_equal(got_t.numpy(), want)
    np.testing.assert_array_equal(MW.body_impulses(rep[1, 2], 2, 3), want[1, 2])   # a single step's rows
    # bodies only (ntot = nb = 2, one slot): fewer slots than bodies
    one = np.zeros((1, 8)); one[0, 2:5] = (1.0, 0.0, -1.0)
    np.testing.assert_array_equal(MW.body_impulses(one, 2, 2), [[1.0, 0.0, -1.0], [-1.0, 0.0, 1.0]])
    assert MW.report_npt(W.mixed_scene_and_statics()[0], W.mixed_scene_and_statics()[1]) == 15
