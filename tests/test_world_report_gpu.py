"""The per-pair contact impulse report of the many-worlds stepper (include/moby_hip.h, "Contact report"; mh_world_large_rp*.hip) against the report
reference (tests/native/world_ref.cpp): states, complete aux records and EVERY report row bit for bit, no tolerance anywhere.  What each case is
there for is asserted on the reference in tests/test_world_report.py (tests/world_report_ref.py shape_conditions)."""
import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import scene as S
from moby_amd.world import WorldBatch, WorldBatchDevice, report_npt
from tests.world_ref import assert_aux_equal
from tests import world_params_ref as P
from tests import world_report_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _the_library_has_the_report():
    lib = _lib.load()
    assert all(hasattr(lib, f) for f in ("mh_world_batch_create_report", "mh_world_batch_step_report", "mh_world_step_batch_report")), "libmoby_hip.so has no contact report"


def assert_rows_equal(got, want):
    """row for row, naming the first world / step / pair slot that differs"""
    if np.array_equal(got, want):
        return
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    w, s, p, k = bad[0]
    raise AssertionError("%d entries differ; first: world %d step %d slot %d entry %d: %r != %r" % (len(bad), w, s, p, k, got[w, s, p, k], want[w, s, p, k]))


def device_batch(case, report=True):
    dev = WorldBatchDevice(case["scene"], case["state"], statics=case["statics"], params=case.get("params"), report=report)
    if case.get("forces") is not None:
        dev.set_forces(case["forces"])
    return dev


@pytest.mark.parametrize("name", ["corner", "box_ball", "mixed", "noslip_table", "plane8", "varied", "forced_stack"])
def test_parity(name):
    """plane8: nb = 8 and a static plane, all 36 pair slots, the last one loaded; corner: three loaded pairs in one island; box_ball: four vertex contacts of one pair (sign = -1) and a box-sphere contact; mixed: restitution passes,
    several folded mini-steps, contacts with zero impulse; noslip_table: the no-slip model's impulses; varied: per-world records, each world against a run
    of its own scene; forced_stack: the forced object under a wrench schedule (a scene with a ground and no statics)"""
    case, st_r, aux_r, rep_r, _ = R.reference_run(name)
    assert ((aux_r["status"] & R.FATAL) == 0).all()                       # no world is left out of the comparison
    wb = WorldBatch(case["scene"], case["state"].copy(), statics=case["statics"], params=case.get("params"), forces=case.get("forces"))
    _, rep = wb.step(case["dt"], case["nsteps"], wrench=case.get("wrench"), want_report=True)
    assert rep.shape == rep_r.shape == (case["state"].shape[0], case["nsteps"], report_npt(case["scene"], case["statics"]), 8)
    np.testing.assert_array_equal(wb.state, st_r)
    assert_aux_equal(wb.aux, aux_r)
    assert_rows_equal(rep, rep_r)


def test_one_launch_of_three_steps_is_three_launches_of_one():
    import torch
    case, _, _, rep_r, _ = R.reference_run("corner")
    B, npt = 8, rep_r.shape[2]
    one, three = device_batch(case), device_batch(case)
    try:
        r3 = torch.full((B, 3, npt, 8), float("nan"), dtype=torch.float64, device="cuda")
        one.step(case["dt"], 3, report=r3)
        parts = []
        for _ in range(3):
            r1 = torch.full((B, 1, npt, 8), float("nan"), dtype=torch.float64, device="cuda")
            three.step(case["dt"], 1, report=r1)
            parts.append(r1)
        st_a, aux_a = one.download()
        st_b, aux_b = three.download()
    finally:
        one.close(); three.close()
    r3 = r3.cpu().numpy()
    assert_rows_equal(torch.cat(parts, dim=1).cpu().numpy(), r3)
    assert_rows_equal(r3, rep_r[:, :3])
    np.testing.assert_array_equal(st_a, st_b)
    assert_aux_equal(aux_a, aux_b)


def test_step_ids_writes_the_rows_of_the_listed_worlds_only():
    """worlds [5, 2, 7] in a launch of their own: their rows, at their own index in the batch, equal the whole-batch run; every other row keeps the NaN
    it was filled with; the wrong shape is refused in Python"""
    import torch
    case, st_r, _, rep_r, _ = R.reference_run("corner")
    dev = device_batch(case)
    try:
        ids = torch.tensor([5, 2, 7], dtype=torch.int32, device="cuda")
        rep = torch.full(rep_r.shape, float("nan"), dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError, match="shape"):
            dev.step_ids(case["dt"], case["nsteps"], ids.data_ptr(), 3, report=rep[:3].contiguous())
        dev.step_ids(case["dt"], case["nsteps"], ids.data_ptr(), 3, report=rep)
        st, _ = dev.download()
    finally:
        dev.close()
    rep = rep.cpu().numpy()
    for w in range(8):
        if w in (5, 2, 7):
            assert_rows_equal(rep[w:w + 1], rep_r[w:w + 1])
            np.testing.assert_array_equal(st[w], st_r[w])
        else:
            assert np.isnan(rep[w]).all(), w
            np.testing.assert_array_equal(st[w], case["state"][w])
    assert len(set(rep_r[w].tobytes() for w in range(8))) == 8            # the worlds' rows differ, so a row under another world's index would show


def test_a_world_that_is_passed_over_writes_zero_rows():
    import torch
    case, _, _, rep_r, _ = R.reference_run("corner")
    aux = S.new_aux(8); aux["status"][3] = S.MH_WORLD_LCP_FAILED
    dev = WorldBatchDevice(case["scene"], case["state"], aux=aux, statics=case["statics"], report=True)
    try:
        rep = torch.full((8, 5) + rep_r.shape[2:], float("nan"), dtype=torch.float64, device="cuda")
        dev.step(case["dt"], 5, report=rep)
        st, a2 = dev.download()
    finally:
        dev.close()
    rep = rep.cpu().numpy()
    assert (rep[3] == 0.0).all() and a2["steps"][3] == 0
    np.testing.assert_array_equal(st[3], case["state"][3])
    keep = [w for w in range(8) if w != 3]
    assert_rows_equal(rep[keep], rep_r[keep, :5])


@pytest.mark.parametrize("forced", [False, True])
def test_key_18_changes_no_result(forced):
    """the varied batch of the per-world-parameters tests through the report objects with a NULL report (key 18) is the params build, bit for bit"""
    case, st_r, aux_r, traj_r = P.varied_run(forced=forced)
    lib = _lib.load()
    out = []
    for key in (0, 1):
        try:
            _lib.check(lib.mh_debug_set(18, key))
            wb = WorldBatch(case["scene"], case["state"].copy(), statics=case["statics"], params=case["params"], forces=case["forces"] if forced else None)
            traj = wb.step(case["dt"], case["nsteps"], want_traj=True, wrench=case["wrench"].copy() if forced else None)
        finally:
            _lib.check(lib.mh_debug_set(18, 0))
        out.append((wb.state, wb.aux, traj))
        np.testing.assert_array_equal(traj, traj_r)
        np.testing.assert_array_equal(wb.state, st_r)
        assert_aux_equal(wb.aux, aux_r)
    np.testing.assert_array_equal(out[0][0], out[1][0])
    assert_aux_equal(out[0][1], out[1][1])


def _both_models_case():
    """mu-coulomb = 100 (the no-slip model) in worlds 0 and 2, 0.4 in worlds 1 and 3 of one batch (tests/test_world_params_gpu.py)"""
    from tests import world_statics_ref as W
    sc, stt, st0 = W.table_batch(4, mu=100.0)
    p = S.make_params(sc, stt, 4)
    p["cp_mu_coulomb"][1] = 0.4
    p["cp_mu_coulomb"][3] = 0.4
    return dict(scene=sc, statics=stt, params=p, state=st0, dt=1e-3, nsteps=20)


@pytest.mark.parametrize("name", ["plane8", "ring", "both_models"])
def test_key_18_on_the_other_params_cases(name):
    """the remaining batches of the per-world-parameters tests -- the last slots (body lane 7 and pair slot 35; static slot 7) and both impact models in
    one batch -- through the report objects with a NULL report equal the params build bit for bit: states, trajectories, complete aux records (the params
    build itself is held to the reference by tests/test_world_params_gpu.py)"""
    case = _both_models_case() if name == "both_models" else P.slots_case(name)
    lib = _lib.load()
    out = []
    for key in (0, 1):
        try:
            _lib.check(lib.mh_debug_set(18, key))
            wb = WorldBatch(case["scene"], case["state"].copy(), statics=case["statics"], params=case["params"])
            traj = wb.step(case["dt"], case["nsteps"], want_traj=True)
        finally:
            _lib.check(lib.mh_debug_set(18, 0))
        out.append((wb.state, wb.aux, traj))
    assert (out[0][1]["lcp_solves"] > 0).all() and ((out[0][1]["status"] & R.FATAL) == 0).all()
    np.testing.assert_array_equal(out[1][2], out[0][2])
    np.testing.assert_array_equal(out[1][0], out[0][0])
    assert_aux_equal(out[1][1], out[0][1])


def test_a_tensor_on_another_device_or_of_another_kind_is_refused_in_python():
    import torch
    case = R.cases()["noslip_table"]
    dev = device_batch(case)
    try:
        assert dev.device == torch.cuda.current_device()
        rep = torch.zeros((4, 2, dev.npt, 8), dtype=torch.float64)
        with pytest.raises(ValueError, match="on the device"):
            dev.step(case["dt"], 2, report=rep)                            # a host tensor
        dev.device += 1                                                       # as if the batch lived elsewhere
        with pytest.raises(ValueError, match="the batch on device"):
            dev.step(case["dt"], 2, report=rep.cuda())
        with pytest.raises(ValueError, match="the batch on device"):
            dev.step(case["dt"], 2, wrench=torch.zeros((4, 1, 6), dtype=torch.float64, device="cuda"))
    finally:
        dev.close()


def test_the_report_pointer_changes_no_step():
    """a report batch stepped by the plain entries (NULL report) ends where the run that wrote the report ended; a report on a batch not created for it
    is refused, so are a tensor of the wrong type and shape"""
    import torch
    case, st_r, aux_r, rep_r, _ = R.reference_run("mixed")
    dev, plain = device_batch(case), device_batch(case, report=False)
    try:
        dev.step(case["dt"], case["nsteps"])
        st, aux = dev.download()
        rep = torch.zeros(rep_r.shape, dtype=torch.float64, device="cuda")
        with pytest.raises(_lib.MobyHipError, match="without the contact report"):
            plain.step(case["dt"], case["nsteps"], report=rep)
        with pytest.raises(ValueError, match="float64"):
            dev.step(case["dt"], case["nsteps"], report=rep.to(torch.float32))
        with pytest.raises(ValueError, match="shape"):
            dev.step(case["dt"], case["nsteps"] - 1, report=rep)
    finally:
        dev.close(); plain.close()
    np.testing.assert_array_equal(st, st_r)
    assert_aux_equal(aux, aux_r)


def test_occupancy_and_profile_of_a_report_batch():
    """five workgroups per CU by the runtime's query, plain and forced; there is no stamped build: every cycle count is zero"""
    case, st_r, aux_r, _, _ = R.reference_run("corner")
    dev = device_batch(case)
    try:
        occ = dev.occupancy()
        phc = _lib.load().mh_world_profile_phase_count()
        cyc = np.full(phc + 4, -1.0)
        _lib.check(_lib.load().mh_world_batch_profile(dev.handle, float(case["dt"]), int(case["nsteps"]), cyc.ctypes.data, phc + 4))
        st, aux = dev.download()
        dev.set_forces(S.make_forces(1, stokes=(0.3, 0.05)))
        occ_f = dev.occupancy()
    finally:
        dev.close()
    print("occupancy of the report objects: plain %d, forced %d" % (occ, occ_f))
    assert occ == 5 and occ_f == 5
    assert (cyc == 0.0).all(), cyc
    np.testing.assert_array_equal(st, st_r)
    assert_aux_equal(aux, aux_r)
