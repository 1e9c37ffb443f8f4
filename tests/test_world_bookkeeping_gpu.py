"""The bookkeeping of the one-wavefront world kernels (mh_world_wave.inc) on the GPU: the pair count, contact count, island
masks and polygon offsets handed from phase to phase as values, the step-start broad phase made only where its list is read, the matrix norm taken
while G is built.  None of it is arithmetic of the reference, so every batch is held bit for bit to the CPU oracle: states and the complete aux record
(every counter, zlast / zbuf with their sizes, the rand() ring, status, time), no tolerance anywhere.  The batches and their oracle results are in
tests/world_bookkeeping_ref.py; tests/test_world_bookkeeping.py checks on the oracle that they contain what they are here for."""
import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import scene as S
from moby_amd.world import WorldBatchDevice
from tests.world_bookkeeping_ref import cases, reference_run
from tests.world_ref import assert_aux_equal, reference as force_reference

pytestmark = pytest.mark.gpu


LARGE_PER_CU = 5          # resident workgroups per CU of every object of the large family (28-31 KB of LDS); the small and the wheel objects (9.6 KB) hold more


def run_device(case, launches=1, params=None, forces=None, large=None):
    """the case on a device batch in `launches` equal launches -> (state, aux); large: whether the batch must have picked an object of the large family"""
    dev = WorldBatchDevice(case["scene"], case["state"], params=params)
    try:
        if large is not None:
            assert (dev.occupancy() == LARGE_PER_CU) == large, dev.occupancy()
        if forces is not None:
            dev.set_forces(forces)
        assert case["nsteps"] % launches == 0
        for _ in range(launches):
            dev.step(case["dt"], case["nsteps"] // launches)
        return dev.download()
    finally:
        dev.close()


def assert_equal_oracle(name, st, aux):
    _, st_o, aux_o, _, _ = reference_run(name)
    np.testing.assert_array_equal(st, st_o)
    assert_aux_equal(aux, aux_o)


@pytest.mark.parametrize("launches", [1, 60])
def test_sphere_stack_landings_in_one_launch_and_in_sixty(launches):
    """8 stacks x 60 steps from t = 0 (islands of 1 and of 3 contacts, n = 14 and n = 42, steps of several mini-steps): as one launch and as 60 launches
    of one step -- the counters, the values that travel between the phases and the step-start pair list across launch boundaries.  Both equal the oracle,
    hence each other"""
    st, aux = run_device(cases()["stack"], launches=launches)
    assert_equal_oracle("stack", st, aux)


def test_two_separated_balls_two_islands_in_a_mini_step():
    """two islands in one mini-step: the search's masks between two next_island calls, the active-contact mask, and the second island's normal
    velocities taken before the first island's impulses were applied"""
    st, aux = run_device(cases()["two_balls"])
    assert_equal_oracle("two_balls", st, aux)


@pytest.mark.parametrize("records", [False, True])
def test_rimless_wheel(records):
    """the lone-wheel path, which keeps the step-start broad phase: on the wheel object, and -- a batch created with per-world records, each a copy of
    the scene's values -- on the large family"""
    c = cases()["wheel"]
    st, aux = run_device(c, params=S.make_params(c["scene"], None, c["state"].shape[0]) if records else None, large=records)
    assert_equal_oracle("wheel", st, aux)


def test_box_and_ball_on_the_plane():
    """the large object: box vertices and a sphere, two islands, friction and restitution"""
    st, aux = run_device(cases()["box_ball"], large=True)
    assert_equal_oracle("box_ball", st, aux)


def test_island_of_eight_contacts():
    """four spheres in a square, one island of 8 contacts (n = 64): more than the packed polygon offsets hold, so the offsets go through gi[I_KOFF..]"""
    st, aux = run_device(cases()["square"], large=True)
    assert_equal_oracle("square", st, aux)


def test_stabiliser_reads_the_pair_list_of_the_last_mini_step():
    """a stack that violates cstab_eps from the start: the stabiliser works in step 1 on the pair list whose length the mini-step stored for it"""
    st, aux = run_device(cases()["sunk_stack"])
    assert_equal_oracle("sunk_stack", st, aux)


def test_a_step_of_dt_zero_is_refused():
    """A step without a mini-step (dt = 0) would have the stabiliser read the step-start pair list.  The entry points refuse dt <= 0 (MH_ERR_INVALID_ARG)
    before anything is launched, so that is what is asserted here; the batch stays as it was uploaded"""
    c = cases()["sunk_stack"]
    dev = WorldBatchDevice(c["scene"], c["state"])
    try:
        st0, aux0 = dev.download()
        for dt in (0.0, -1e-3, float("nan")):
            with pytest.raises(_lib.MobyHipError) as e:
                dev.step(dt, 1)
            assert e.value.code == _lib.MH_ERR_INVALID_ARG
        st, aux = dev.download()
    finally:
        dev.close()
    np.testing.assert_array_equal(st, st0)
    assert aux.tobytes() == aux0.tobytes()


def test_impact_lcp_whose_attempt_zero_fails():
    """the ladder's offdiag_max (the norm kept from compute_problem_data): the reference scene's first steps, whose impact solves fail attempt 0 and are
    regularised (tests/test_world_bookkeeping.py shows it on the oracle's trace); most steps of the stack batch above do the same"""
    st, aux = run_device(cases()["regularised"])
    assert_equal_oracle("regularised", st, aux)


def test_forces_object_with_a_stored_drag_term():
    """the _forces object: the stack batch under Stokes drag against the forced reference (tests/native/world_ref.cpp)"""
    c = cases()["stack"]
    forces = S.make_forces(3, stokes=(0.3, 0.05))
    st_r, aux_r = c["state"].copy(), S.new_aux(c["state"].shape[0])
    force_reference().step(c["scene"], st_r, aux_r, c["dt"], c["nsteps"], forces=forces)
    assert ((aux_r["status"] & ~S.MH_WORLD_IMPACT_TOL) == 0).all() and (aux_r["lcp_solves"] > 0).all()
    st, aux = run_device(c, forces=forces)
    np.testing.assert_array_equal(st, st_r)
    assert_aux_equal(aux, aux_r)


def test_profile_object_steps_as_the_plain_object():
    """the _prof object through mh_world_batch_profile: state and aux of the plain launch (= the oracle's), stamps that are not zero, and a phase sum
    that lies between the fastest and the slowest world's cycle count of the launch"""
    c = cases()["stack"]
    lib = _lib.load()
    phc = lib.mh_world_profile_phase_count()
    cyc = np.full(phc + 4, -1.0)
    dev = WorldBatchDevice(c["scene"], c["state"])
    try:
        _lib.check(lib.mh_world_batch_profile(dev.handle, float(c["dt"]), int(c["nsteps"]), cyc.ctypes.data, phc + 4))
        st, aux = dev.download()
    finally:
        dev.close()
    print("cycles", cyc)
    assert_equal_oracle("stack", st, aux)
    st_p, aux_p = run_device(c)
    np.testing.assert_array_equal(st, st_p)
    assert aux.tobytes() == aux_p.tobytes()
    assert np.isfinite(cyc).all() and (cyc >= 0).all()
    assert (cyc[[0, 1, 2, 3, 4, 5, 6, 7, 8]] > 0).all()          # broad+CA .. apply: every phase of an impact step was stamped
    total, slowest, fastest = cyc[:10].sum(), cyc[phc], cyc[phc + 1]
    assert 0 < fastest <= total <= slowest
