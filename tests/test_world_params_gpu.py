"""Per-world parameters of the many-worlds stepper (include/moby_hip.h, "Per-world parameters"; mh_world_large_pw*.hip) against the CPU references, which
take one scene per call: world w of a varied batch equals a reference run of world w's scene (tests/world_params_ref.py), bit for bit -- states,
trajectories and complete aux records, no tolerance anywhere."""
import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import scene as S
from moby_amd.world import WorldBatch, WorldBatchDevice
from tests.world_ref import assert_aux_equal
from tests import world_params_ref as P
from tests import world_statics_ref as W

pytestmark = pytest.mark.gpu


def run_host(case, want_traj=True, forced=False):
    wb = WorldBatch(case["scene"], case["state"].copy(), statics=case["statics"], params=case["params"], forces=case["forces"] if forced else None)
    traj = wb.step(case["dt"], case["nsteps"], want_traj=want_traj, wrench=case["wrench"].copy() if forced else None)
    return wb.state, wb.aux, traj


@pytest.mark.parametrize("name", ["corner", "noslip_table", "mixed_forces"])
def test_key_17_changes_no_result(name):
    """(1) same scene: a statics batch through mh_world_large_pw* (key 17 = 1, every record filled from the scene by the library) equals the reference;
    `mixed_forces` launches the forced object under a wrench schedule"""
    case, st_r, aux_r, traj_r, _ = W.reference_run(name)
    lib = _lib.load()
    try:
        _lib.check(lib.mh_debug_set(17, 1))
        wb = WorldBatch(case["scene"], case["state"].copy(), forces=case.get("forces"), statics=case["statics"])
        traj = wb.step(case["dt"], case["nsteps"], want_traj=True, wrench=case.get("wrench"))
    finally:
        _lib.check(lib.mh_debug_set(17, 0))
    np.testing.assert_array_equal(traj, traj_r)
    np.testing.assert_array_equal(wb.state, st_r)
    assert_aux_equal(wb.aux, aux_r)


def test_varied_batch():
    """(2) eight worlds of the mixed scene, seven of them with masses, inertias, shapes, gravity, ground, wall, static box and contact parameters of their
    own (conditions on the input: tests/world_params_ref.py varied_run)"""
    case, st_r, aux_r, traj_r = P.varied_run()
    st, aux, traj = run_host(case)
    np.testing.assert_array_equal(traj, traj_r)
    np.testing.assert_array_equal(st, st_r)
    assert_aux_equal(aux, aux_r)


@pytest.mark.parametrize("name", ["plane8", "ring"])
def test_last_slots(name):
    """(3) plane8: nb = 8 and one static plane, per-world radii, masses, friction and plane height -- body lane 7 and pair slot 35 of the fill;
    ring: nb = 1 and eight statics with per-world frames -- static slot 7"""
    case = P.slots_case(name)
    st_r, aux_r, traj_r = P.run_ref_params(case["scene"], case["statics"], case["params"], case["state"], case["dt"], case["nsteps"], want_traj=True)
    P.check_conditions(aux_r, case["nsteps"])
    wb = WorldBatch(case["scene"], case["state"].copy(), statics=case["statics"], params=case["params"])
    traj = wb.step(case["dt"], case["nsteps"], want_traj=True)
    np.testing.assert_array_equal(traj, traj_r)
    np.testing.assert_array_equal(wb.state, st_r)
    assert_aux_equal(wb.aux, aux_r)


def test_step_ids_reads_the_record_of_the_world_not_of_the_workgroup():
    """(4) the varied batch resident on the device: one launch of the worlds [5, 2, 7], then one of the rest.  After the first the unlisted worlds are
    untouched; after the second every world equals the reference"""
    import torch
    case, st_r, aux_r, _ = P.varied_run()
    aux0 = S.new_aux(8)
    dev = WorldBatchDevice(case["scene"], case["state"], statics=case["statics"], params=case["params"])
    try:
        first = torch.tensor([5, 2, 7], dtype=torch.int32, device="cuda")
        rest = torch.tensor([0, 1, 3, 4, 6], dtype=torch.int32, device="cuda")
        dev.step_ids(case["dt"], case["nsteps"], first.data_ptr(), 3)
        st1, aux1 = dev.download()
        dev.step_ids(case["dt"], case["nsteps"], rest.data_ptr(), 5)
        st2, aux2 = dev.download()
    finally:
        dev.close()
    for w in (0, 1, 3, 4, 6):
        np.testing.assert_array_equal(st1[w], case["state"][w])
        assert aux1[w].tobytes() == aux0[w].tobytes()
    for w in (5, 2, 7):
        np.testing.assert_array_equal(st1[w], st_r[w], err_msg="world %d" % w)
    np.testing.assert_array_equal(st2, st_r)
    assert_aux_equal(aux2, aux_r)


def test_both_impact_models_in_one_batch():
    """(5) mu-coulomb = 100 (the no-slip model) in worlds 0 and 2, 0.4 (Drumwright-Shell) in worlds 1 and 3 of one batch: the model is chosen per island
    from the contacts' own mu"""
    sc, stt, st0 = W.table_batch(4, mu=100.0)
    p = S.make_params(sc, stt, 4)
    p["cp_mu_coulomb"][1] = 0.4
    p["cp_mu_coulomb"][3] = 0.4
    st_r, aux_r, traj_r = P.run_ref_params(sc, stt, p, st0, 1e-3, 20, want_traj=True)
    assert list(aux_r["vns_size"]) == [1, 0, 1, 0] and (aux_r["status"] == 0).all() and (aux_r["lcp_solves"] >= 19).all()
    wb = WorldBatch(sc, st0.copy(), statics=stt, params=p)
    traj = wb.step(1e-3, 20, want_traj=True)
    np.testing.assert_array_equal(traj, traj_r)
    np.testing.assert_array_equal(wb.state, st_r)
    assert_aux_equal(wb.aux, aux_r)


@pytest.mark.parametrize("from_device", [False, True])
def test_records_replaced_between_launches(from_device):
    """(6) ten steps, new gravity and a moved static box in worlds 3-5, ten more steps == the reference in two legs; from a host array (set_params) and
    from a torch tensor on a stream of its own, followed by a step on that stream (set_params_dev)"""
    import torch
    case = P.varied_case()
    sc, stt, dt = case["scene"], case["statics"], case["dt"]
    p2 = case["params"].copy()
    for w in (3, 4, 5):
        p2["gravity"][w] = (0.4 * (w - 4), -7.0 - w, 0.25)
        p2["st_o"][w, 1] += p2["st_R"][w, 1].reshape(3, 3) @ np.array([0.01 * w, -5e-4, -0.02])
    st_r, aux_r = case["state"].copy(), S.new_aux(8)
    P.step_ref_params(sc, stt, case["params"], st_r, aux_r, dt, 10)
    mid = st_r.copy()
    P.step_ref_params(sc, stt, p2, st_r, aux_r, dt, 10)
    keep = st_r.copy(), aux_r.copy()
    P.check_conditions(aux_r, 20)
    st_same, aux_same = case["state"].copy(), S.new_aux(8)
    P.step_ref_params(sc, stt, case["params"], st_same, aux_same, dt, 20)
    assert all(not np.array_equal(st_r[w], st_same[w]) for w in (3, 4, 5))           # the new records matter
    dev = WorldBatchDevice(sc, case["state"], statics=stt, params=case["params"])
    try:
        if from_device:
            stream = torch.cuda.Stream()
            t = torch.as_tensor(np.ascontiguousarray(p2[3:6]).view(np.float64).reshape(3, S.PARAMS_DOUBLES), device="cuda")
            torch.cuda.synchronize()
            dev.step(dt, 10, stream=stream.cuda_stream)
            with pytest.raises(ValueError):
                dev.set_params_dev(t.to(torch.float32), first=3)
            with pytest.raises(ValueError):
                dev.set_params_dev(t[:, :300].contiguous(), first=3)
            dev.set_params_dev(t, first=3, stream=stream.cuda_stream)
            dev.step(dt, 10, stream=stream.cuda_stream)
        else:
            dev.step(dt, 10)
            st_m, _ = dev.download()
            np.testing.assert_array_equal(st_m, mid)
            with pytest.raises(_lib.MobyHipError, match="outside the batch"):
                dev.set_params(p2[3:6], first=6)
            bad = p2[3:6].copy(); bad["mass"][1, 0] = 0.0
            with pytest.raises(_lib.MobyHipError, match="world 4: mass"):
                dev.set_params(bad, first=3)
            dev.set_params(p2[3:6], first=3)
            dev.step(dt, 10)
        st, aux = dev.download()
    finally:
        dev.close()
    np.testing.assert_array_equal(st, keep[0])
    assert_aux_equal(aux, keep[1])


def test_set_params_needs_a_batch_created_with_records():
    case = P.varied_case()
    dev = WorldBatchDevice(case["scene"], case["state"], statics=case["statics"])
    try:
        with pytest.raises(_lib.MobyHipError, match="without per-world parameters"):
            dev.set_params(case["params"])
    finally:
        dev.close()


def test_varied_batch_with_forces():
    """(7) the varied batch through the forced object (mh_world_large_pw_forces.hip): Stokes drag and damping stored, a wrench row per step"""
    case, st_r, aux_r, traj_r = P.varied_run(forced=True)
    assert case["forces"].terms == 3 and case["wrench"].shape == (case["nsteps"], 8, 3, 6)
    st, aux, traj = run_host(case, forced=True)
    np.testing.assert_array_equal(traj, traj_r)
    np.testing.assert_array_equal(st, st_r)
    assert_aux_equal(aux, aux_r)
    assert not np.array_equal(st, P.varied_run()[1])


WHEEL_SLOPES = (0.05, 0.08, 0.1, 0.15)
WHEEL_RATES = (0.5, 0.41, 0.33, 0.24)         # the slow wheel on the steep slope: every one of the four gets over its first spoke (0.24 on 0.05 rolls back)
WHEEL_STEPS, WHEEL_CHUNK = 4300, 50           # the last first impact is world 3's, in step 4200; the four oracle runs take about three seconds


def test_rimless_wheel_on_four_slopes(oracle):
    """(8) the rimless wheel (spokes geometry, no-slip model: a scene that takes the wheel variant without records) with gravity (sin a, 0, -cos a), mass
    and inertia of its own in every world, against the oracle per world.  The oracle runs in chunks of 50 steps so that the spoke impact can be seen
    on it: the wheel's rate drops by more than 0.1 rad/s in the chunk of an impact and by about 0.01 rad/s while it pivots"""
    sc = S.rimless_wheel_scene()
    st0 = S.rimless_wheel_state(WHEEL_RATES)
    p = S.make_params(sc, None, 4)
    for w, a in enumerate(WHEEL_SLOPES):
        p["gravity"][w] = (np.sin(a), 0.0, -np.cos(a))
        p["mass"][w, 0] *= 1.0 + w / 2.0
        p["inertia"][w, 0] *= 1.0 + w / 2.0
    st_o, aux_o = st0.copy(), S.new_aux(4)
    traj_o = np.zeros((4, WHEEL_STEPS, 1, 7))
    impacts = np.zeros(4, dtype=int)
    for w in range(4):
        s2, _ = P.world_scene(sc, None, p, w)
        for k in range(0, WHEEL_STEPS, WHEEL_CHUNK):
            rate = st_o[w, 11]
            traj_o[w, k:k + WHEEL_CHUNK] = np.asarray(oracle.world_step(s2, st_o[w], aux_o[w:w + 1], 1e-3, WHEEL_CHUNK)["traj"]).reshape(WHEEL_CHUNK, 1, 7)
            impacts[w] += st_o[w, 11] < rate - 0.05
    assert ((aux_o["status"] & P.FATAL) == 0).all() and (aux_o["vns_size"] > 0).all() and (impacts >= 1).all(), (aux_o["status"], aux_o["vns_size"], impacts)
    assert all(not np.array_equal(st_o[i], st_o[j]) for i in range(4) for j in range(i + 1, 4))
    wb = WorldBatch(sc, st0.copy(), params=p)
    traj = wb.step(1e-3, WHEEL_STEPS, want_traj=True)
    np.testing.assert_array_equal(traj, traj_o)
    np.testing.assert_array_equal(wb.state, st_o)
    assert_aux_equal(wb.aux, aux_o)


def test_occupancy_and_profile_of_a_params_batch():
    """(9) occupancy() reports the object the batch launches (plain, and forced once forces are stored) and equals the statics build's; there is no
    stamped build: mh_world_batch_profile steps the worlds with the production object and every cycle count is exactly zero"""
    def profile(dev, dt, nsteps):
        phc = _lib.load().mh_world_profile_phase_count()
        cyc = np.full(phc + 4, -1.0)
        _lib.check(_lib.load().mh_world_batch_profile(dev.handle, float(dt), int(nsteps), cyc.ctypes.data, phc + 4))
        return cyc, phc
    case, st_r, aux_r, _ = P.varied_run()
    dev = WorldBatchDevice(case["scene"], case["state"], statics=case["statics"], params=case["params"])
    twin = WorldBatchDevice(case["scene"], case["state"], statics=case["statics"])
    try:
        occ = (dev.occupancy(), twin.occupancy())
        cyc, phc = profile(dev, case["dt"], case["nsteps"])
        st, aux = dev.download()
        dev.set_forces(case["forces"]); twin.set_forces(case["forces"])
        occ_f = (dev.occupancy(), twin.occupancy())
    finally:
        dev.close(); twin.close()
    print("occupancy params / statics twin:", occ, "with forces:", occ_f)
    assert occ[0] == occ[1] >= 1 and occ_f[0] == occ_f[1] >= 1
    np.testing.assert_array_equal(st, st_r)
    assert_aux_equal(aux, aux_r)
    assert (cyc == 0.0).all(), cyc
