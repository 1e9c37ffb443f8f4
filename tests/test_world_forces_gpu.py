"""Recurrent forces and per-world body wrenches in the one-wavefront world kernels (mh_world_{small,wheel,large}_forces.hip) on the GPU: every
variant bit for bit against the forced reference (tests/native/world_ref.cpp) -- states and complete aux records, no tolerance anywhere --
schedules, split launches, id lists, dead worlds, trajectories, residency, the unforced paths through the new entry points, and a scene file."""
import ctypes
import os

import numpy as np
import pytest

from moby_amd import scene as S
from moby_amd.world import WorldBatch, WorldBatchDevice
from tests.world_force_ref import reference_run
from tests.world_ref import assert_aux_equal, reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def force_ref():
    return reference()


@pytest.fixture(scope="module")
def force_runs():
    """name -> (case, final state, final aux, trajectory) of the reference (cached per process in tests/world_force_ref.py)"""
    return reference_run


def dev_wrench(w):
    import torch
    return None if w is None else torch.as_tensor(np.ascontiguousarray(w, dtype=np.float64), device="cuda")


def run_device(case, launches=1, want_traj=False):
    """the case on a device batch, in `launches` equal launches -> (state, aux, trajectory or None)"""
    import torch
    dev = WorldBatchDevice(case["scene"], case["state"])
    try:
        if case["forces"] is not None:
            dev.set_forces(case["forces"])
        B, n = case["state"].shape[0], case["nsteps"] // launches
        w = dev_wrench(case["wrench"])
        trajs = []
        for k in range(launches):
            traj = torch.zeros((B, n, case["scene"].nb, 7), dtype=torch.float64, device="cuda") if want_traj else None
            wk = w if (w is None or w.dim() == 3) else w[k * n:(k + 1) * n].contiguous()
            dev.step(case["dt"], n, traj_ptr=None if traj is None else traj.data_ptr(), wrench=wk)
            trajs.append(traj)
        st, aux = dev.download()
        return st, aux, (torch.cat(trajs, dim=1).cpu().numpy() if want_traj else None)
    finally:
        dev.close()


@pytest.fixture(scope="module")
def stack_on_device(force_runs):
    """batch (a) in one launch with its trajectory: shared by (a) and (j) -- its spinning spheres make it the one expensive launch of this file"""
    return run_device(force_runs("stack")[0], want_traj=True)


@pytest.mark.parametrize("name", ["stack", "ball", "wheel", "cone", "hover_stokes"])
def test_forced_kernels_equal_the_reference(force_runs, stack_on_device, name):
    """(a) small variant, contacts + several mini-steps per step + one wrench row per step; (c) small variant, impacts with restitution under drag;
    (d) wheel variant, no-slip model under damping; (e) large variant, a box pushed inside and outside its friction cone by a wrench alone;
    (f) large variant at MH_MAX_BODIES: body lanes 0..7, Stokes drag and a hovering wrench"""
    case, st_r, aux_r, _ = force_runs(name)
    st, aux, _ = stack_on_device if name == "stack" else run_device(case)
    np.testing.assert_array_equal(st, st_r)
    assert_aux_equal(aux, aux_r)
    if name in ("stack", "wheel", "ball"):
        assert (aux_r["lcp_solves"] > 0).all()
    if name == "stack":
        assert (aux_r["mini_steps"] > aux_r["steps"]).all()             # steps of several mini-steps: the row is re-read by each
    if name == "cone":
        assert np.abs(st[:3, 0]).max() < 1e-9 and st[3, 0] > 1.0


def test_one_row_in_three_launches_equals_one_launch(force_runs):
    """(b) rows == 1: the row holds for every step of a launch, so 3 launches of 20 are 1 launch of 60 -- and both are the reference"""
    case, st_r, aux_r, _ = force_runs("stack_const")
    st1, aux1, _ = run_device(case, launches=1)
    st3, aux3, _ = run_device(case, launches=3)
    np.testing.assert_array_equal(st1, st_r)
    assert_aux_equal(aux1, aux_r)
    np.testing.assert_array_equal(st3, st_r)
    assert_aux_equal(aux3, aux_r)


def test_a_full_size_row_held_over_split_launches(force_runs):
    """(b) again with full-size torques (the schedule's row 0) on the contact scene, over 12 steps: 3 launches of 4 are 1 launch of 12 are the reference"""
    case, st_r, aux_r, _ = force_runs("stack_const_full")
    assert (aux_r["lcp_solves"] > 0).all() and (aux_r["mini_steps"] > aux_r["steps"]).all()
    for launches in (1, 3):
        st, aux, _ = run_device(case, launches=launches)
        np.testing.assert_array_equal(st, st_r)
        assert_aux_equal(aux, aux_r)


def test_schedule_split_over_launches_equals_one_launch(force_runs):
    """one row per step at MH_MAX_BODIES under damping, whole and cut in 2: each launch starts reading at ITS row 0"""
    case, st_r, aux_r, _ = force_runs("hover_sched")
    for launches in (1, 2):
        st, aux, _ = run_device(case, launches=launches)
        np.testing.assert_array_equal(st, st_r)
        assert_aux_equal(aux, aux_r)


def test_id_list_steps_the_named_worlds_under_their_own_wrench_rows(force_runs):
    """(g) worlds 1 and 3 of batch (a): they equal the reference (so each read the wrench at its own index in the batch, not at its place in the
    list), the other three keep their uploaded state and aux bit for bit"""
    import torch
    case, st_r, aux_r, _ = force_runs("stack")
    dev = WorldBatchDevice(case["scene"], case["state"])
    try:
        dev.set_forces(case["forces"])
        st0, aux0 = dev.download()
        ids = torch.tensor([1, 3], dtype=torch.int32, device="cuda")
        dev.step_ids(case["dt"], case["nsteps"], ids.data_ptr(), 2, wrench=dev_wrench(case["wrench"]))
        st, aux = dev.download()
    finally:
        dev.close()
    for w in (1, 3):
        np.testing.assert_array_equal(st[w], st_r[w])
        assert_aux_equal(aux[w:w + 1], aux_r[w:w + 1])
    for w in (0, 2, 4):
        np.testing.assert_array_equal(st[w], st0[w])
        assert aux[w:w + 1].tobytes() == aux0[w:w + 1].tobytes()


def test_a_dead_world_is_passed_over_under_forces(force_runs):
    """(h) a world uploaded with MH_WORLD_LCP_FAILED is not stepped; its neighbours are"""
    case, st_r, aux_r, _ = force_runs("hover_sched")
    aux0 = S.new_aux(3)
    aux0["status"][1] = S.MH_WORLD_LCP_FAILED
    dev = WorldBatchDevice(case["scene"], case["state"], aux=aux0)
    try:
        dev.set_forces(case["forces"])
        dev.step(case["dt"], case["nsteps"], wrench=dev_wrench(case["wrench"]))
        st, aux = dev.download()
    finally:
        dev.close()
    np.testing.assert_array_equal(st[1], case["state"][1])
    assert aux[1:2].tobytes() == aux0[1:2].tobytes()
    for w in (0, 2):
        np.testing.assert_array_equal(st[w], st_r[w])
        assert_aux_equal(aux[w:w + 1], aux_r[w:w + 1])


def test_unforced_paths_are_the_plain_kernel(oracle):
    """(i) a batch that never saw set_forces, stepped through step_wrench(NULL wrench), is mh_world_batch_step, which is the oracle; a forced batch
    after set_forces(NULL) is the plain kernel again"""
    from moby_amd import _lib
    sc, st0 = S.sphere_stack_scene(), S.sphere_stack_state(5)
    st_o, aux_o = st0.copy(), S.new_aux(5)
    oracle.world_step_batch(sc, st_o, aux_o, 0.01, 40)
    plain = WorldBatch(sc, st0.copy())
    plain.step(0.01, 40)
    np.testing.assert_array_equal(plain.state, st_o)
    assert_aux_equal(plain.aux, aux_o)
    dev = WorldBatchDevice(sc, st0)
    try:
        _lib.check(_lib.load().mh_world_batch_step_wrench(dev.handle, None, 0.01, 40, None, None, 0, None, 1))
        st, aux = dev.download()
    finally:
        dev.close()
    np.testing.assert_array_equal(st, plain.state)
    assert aux.tobytes() == plain.aux.tobytes()
    dev = WorldBatchDevice(sc, st0)
    try:
        dev.set_forces(S.make_forces(3, stokes=(0.3, 0.05)))
        dev.set_forces(None)
        dev.step(0.01, 40)
        st, aux = dev.download()
    finally:
        dev.close()
    np.testing.assert_array_equal(st, plain.state)
    assert aux.tobytes() == plain.aux.tobytes()


def test_stored_forces_are_honoured_by_the_plain_entry_points(force_runs):
    """after set_forces, mh_world_batch_step / _step_ids (no wrench argument at all) and the host convenience run under the scene's forces"""
    import torch
    case, st_r, aux_r, traj_r = force_runs("ball")
    dev = WorldBatchDevice(case["scene"], case["state"])
    try:
        dev.set_forces(case["forces"])
        ids = torch.tensor([2, 0, 1], dtype=torch.int32, device="cuda")
        dev.step_ids(case["dt"], case["nsteps"], ids.data_ptr(), 3)
        st, aux = dev.download()
    finally:
        dev.close()
    np.testing.assert_array_equal(st, st_r)
    assert_aux_equal(aux, aux_r)
    host = WorldBatch(case["scene"], case["state"].copy(), forces=case["forces"])
    traj = host.step(case["dt"], case["nsteps"], want_traj=True)
    np.testing.assert_array_equal(host.state, st_r)
    assert_aux_equal(host.aux, aux_r)
    np.testing.assert_array_equal(traj, traj_r)


def test_profile_launch_honours_stored_forces(force_runs):
    """mh_world_batch_profile of a batch with stored forces launches the forced production kernel: the worlds are stepped under their forces (the
    reference's states and records) and, that kernel having no stamps, every cycle count is zero"""
    from moby_amd import _lib
    lib = _lib.load()
    case, st_r, aux_r, _ = force_runs("ball")
    nph = lib.mh_world_profile_phase_count() + 4
    cyc = np.full(nph, -1.0)
    dev = WorldBatchDevice(case["scene"], case["state"])
    try:
        dev.set_forces(case["forces"])
        _lib.check(lib.mh_world_batch_profile(dev.handle, case["dt"], case["nsteps"], cyc.ctypes.data, nph))
        st, aux = dev.download()
    finally:
        dev.close()
    np.testing.assert_array_equal(st, st_r)
    assert_aux_equal(aux, aux_r)
    assert (cyc == 0.0).all(), cyc


def test_trajectory_under_forces(force_runs, stack_on_device):
    """(j) the per-step coordinates of a forced launch are the reference's"""
    _, _, _, traj_r = force_runs("stack")
    np.testing.assert_array_equal(stack_on_device[2], traj_r)


def test_forced_small_variant_keeps_its_residency():
    """(k) the runtime's occupancy query for the forced small-variant kernel equals the plain one's (the image grew by 12 MHW_NB doubles)"""
    dev = WorldBatchDevice(S.sphere_stack_scene(), S.sphere_stack_state(2))
    try:
        plain = dev.occupancy()
        dev.set_forces(S.make_forces(3, stokes=(0.3, 0.05), damping=(0.2, 0.02, 0.1, 0.01)))
        forced = dev.occupancy()
    finally:
        dev.close()
    print("workgroups per CU: plain %d, forced %d" % (plain, forced))
    assert plain > 0 and forced == plain


def test_drag_scene_file_runs_as_the_reference(force_ref):
    """(l) tests/scenes/ball_in_syrup.xml through load_xml_forces and the stepper"""
    from moby_amd import io as mio
    sc, st0, ids, dt, forces = mio.load_xml_forces(os.path.join(ROOT, "tests", "scenes", "ball_in_syrup.xml"))
    assert forces.terms == S.MH_FORCE_STOKES and dt == 0.01
    st_r, aux_r = st0.copy(), S.new_aux(1)
    force_ref.step(sc, st_r, aux_r, dt, 150, forces=forces)
    assert aux_r["status"][0] == 0 and aux_r["lcp_solves"][0] > 0
    host = WorldBatch(sc, st0.copy(), forces=forces)
    host.step(dt, 150)
    np.testing.assert_array_equal(host.state, st_r)
    assert_aux_equal(host.aux, aux_r)
