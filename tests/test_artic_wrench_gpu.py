"""Link wrenches and link damping of the articulated stepper on the GPU (include/moby_hip_artic.h, "Link wrenches"): the kernels of mh_artic_wr.hip /
mh_artic_wr_pose.hip against tests/native/artic_wrench_ref.cpp, one reference run per world on the model with that world's record
(tests/artic_wrench_ref.py), bit for bit -- q, qd, every aux field, the base pose and every report row.  B = 3 worlds, 4 steps, one launch per case.
The reference itself is pinned by tests/test_artic_wrench.py."""
import ctypes

import numpy as np
import pytest
import torch

from moby_amd import _lib
from moby_amd import artic as A
from moby_amd import scene as S
from tests import artic_params_ref as P
from tests import artic_wrench_ref as W
from tests.test_artic_box_gpu import same

pytestmark = pytest.mark.gpu
B, N = W.B, W.NSTEPS
MH_ERR_INVALID_ARG = -1


@pytest.fixture(scope="module")
def ref():
    return W.build_wrench_ref()


def make_batch(c, wrench=True, aux0=None):
    """a batch created at q = 0, switched to its coordinates there, then given its start state"""
    z = np.zeros_like(c["q"])
    ab = A.ArticBatch(c["m"], z, z, base_coords=c.get("coords", "angles"), report=c.get("report", False), params=c.get("params", True), wrench=wrench)
    ab.upload(c["q"], c["qd"], S.new_aux(B) if aux0 is None else aux0)
    return ab


def launch(ab, c, wrench="case"):
    """one launch of the case on the batch -> dict(q, qd, aux, pose, report) as W.reference_of returns it"""
    rep = torch.full((B, N, ab.report_slots, A.REPORT_PAIR), float("nan"), dtype=torch.float64, device=ab._device()) if ab.report else None
    wr = c["wrench"] if isinstance(wrench, str) else wrench
    ab.step(c["dt"], N, drive=c.get("drive"), report=rep, wrench=None if wr is None else W.to_device(wr, ab._device()))
    q, qd, aux = ab.download()
    return dict(q=q, qd=qd, aux=aux, pose=ab.base_pose() if c.get("coords") == "pose" else None, report=None if rep is None else rep.cpu().numpy())


def check(got, want, worlds=range(B)):
    ws = list(worlds)
    same((got["q"][ws], got["qd"][ws], got["aux"][ws]), (want["q"][ws], want["qd"][ws], want["aux"][ws]), len(ws))
    if want["pose"] is not None:
        assert np.array_equal(got["pose"][ws], want["pose"][ws]), "max |dP| = %.3e" % np.abs(got["pose"][ws] - want["pose"][ws]).max()
    if got["report"] is not None:
        assert not np.isnan(got["report"]).any(), "%d entries of the report were not written" % int(np.isnan(got["report"]).sum())
        assert np.array_equal(got["report"][ws], want["report"][ws]), "max |d row| = %.3e" % np.abs(got["report"][ws] - want["report"][ws]).max()


def run_case(ref, c):
    want = W.reference_of(ref, c)
    ab = make_batch(c)
    got = launch(ab, c)
    ab.close()
    check(got, want)
    return got, want


@pytest.mark.parametrize("rows", [1, N], ids=["held", "row_per_step"])
@pytest.mark.parametrize("algorithm", [W.CRB, W.FSAB], ids=["crb", "fsab"])
def test_chain_without_geometry(ref, algorithm, rows):
    """the chain of 3, no geometry at all, a wrench on every link in model axes: k_artic_step_wr, both dynamics algorithms, a held row and a row per step"""
    c = W.case_chain(algorithm, rows)
    got, want = run_case(ref, c)
    assert np.abs(want["qd"] - W.reference_of(ref, c, wrench=None)["qd"]).max() > 1e-2


def test_arm_that_lands_during_the_launch(ref):
    """the sphere-tipped arm: some step has two mini-steps, so the wrench is evaluated twice inside it, with the link frames of each mini-step's q;
    MH_LINK_WRENCH_LINK_AXES, a schedule row per step, with the drive and the report (k_artic_step_wr_drive)"""
    c = W.case_arm()
    got, want = run_case(ref, c)
    assert (want["aux"]["mini_steps"] > N).all() and (want["aux"]["lcp_solves"] > 0).all() and (want["report"][..., 0] > 0).any()


def test_floating_box_foot_in_pose_coordinates_with_the_stabiliser(ref):
    """the floating box landing flat, pose coordinates, stabiliser on, damping plus a held wrench on the base link and the pendulum, the report
    (k_artic_step_wr_stab_pose)"""
    c = W.case_foot()
    got, want = run_case(ref, c)
    assert c["m"].cstab_max_iterations > 0 and (want["aux"]["mini_steps"] > N).all() and (want["report"][..., 1] > 0).any()


def test_records_and_wrenches_that_differ_per_world(ref):
    """a params batch whose records differ per world, mu on either side of 100, with a wrench that differs per world; then the wrench rows of worlds
    0 and 2 exchanged: world 1 keeps its result to the bit, worlds 0 and 2 follow the reference under the other's rows"""
    c = W.case_params()
    mu = c["params"]["cp_mu_coulomb"]
    assert (mu < 100.0).any() and (mu >= 100.0).any()
    got, want = run_case(ref, c)
    assert (want["aux"]["lcp_solves"] > 0).all()
    sw = W.swapped(c["wrench"], 0, 2)
    want2 = W.reference_of(ref, c, wrench=sw)
    ab = make_batch(c)
    got2 = launch(ab, c, wrench=sw)
    ab.close()
    check(got2, want2)
    check(got2, got, worlds=[1])
    for w in (0, 2):
        assert not np.array_equal(got2["qd"][w], got["qd"][w])


def test_damping_alone_with_gains_per_world(ref):
    c = W.case_chain_damped()
    got, want = run_case(ref, c)
    k = c["wrench"].arrays["kl"]
    assert not np.array_equal(k[0], k[1]) and np.abs(want["qd"] - W.reference_of(ref, c, wrench=None)["qd"]).max() > 1e-3


def _c_step(ab, c, w, rep=None):
    return _lib.load().mh_artic_batch_step_wrench(ab.handle, None, ctypes.c_double(c["dt"]), N, None, None if w is None else ctypes.byref(w), rep)


def test_no_wrench_is_the_params_batch(ref):
    """a wrench batch stepped without a wrench -- through ArticBatch.step, and through mh_artic_batch_step_wrench with NULL and with terms = 0 -- equals
    the same model through mh_artic_batch_create_params bit for bit (state, aux, pose, rows); so does a params batch under mh_debug_set(21, 1)"""
    c = W.case_foot()
    pb = make_batch(c, wrench=False)
    want = launch(pb, c, wrench=None)
    pb.close()
    check(want, W.reference_of(ref, c, wrench=None))
    ab = make_batch(c)
    check(launch(ab, c, wrench=None), want)
    ab.close()
    for w in (None, A.mh_artic_wrench(terms=0)):
        ab = make_batch(c)
        rep = torch.full((B, N, ab.report_slots, A.REPORT_PAIR), float("nan"), dtype=torch.float64, device=ab._device())
        _lib.check(_c_step(ab, c, w, rep.data_ptr()))
        q, qd, aux = ab.download()
        check(dict(q=q, qd=qd, aux=aux, pose=ab.base_pose(), report=rep.cpu().numpy()), want)
        ab.close()
    lib = _lib.load()
    _lib.check(lib.mh_debug_set(21, 1))
    try:
        kb = make_batch(c, wrench=False)
    finally:
        _lib.check(lib.mh_debug_set(21, 0))
    check(launch(kb, c, wrench=None), want)
    kb.close()


def test_a_failed_world_is_passed_over(ref):
    """world 1 carries MH_WORLD_LCP_FAILED: it keeps its state and counters, its neighbours follow the reference"""
    c = W.case_chain(W.CRB, N)
    aux0 = S.new_aux(B); aux0["status"][1] = S.MH_WORLD_LCP_FAILED
    want = W.reference_of(ref, c, aux0=aux0)
    ab = make_batch(c, aux0=aux0)
    got = launch(ab, c)
    ab.close()
    check(got, want)
    assert np.array_equal(got["q"][1], c["q"][1]) and got["aux"]["steps"][1] == 0 and (got["aux"]["steps"][[0, 2]] == N).all()


def test_python_and_c_abi_give_identical_bytes(ref):
    """the arm case through mh_artic_batch_create_wrench / _upload / _step_wrench / _download by hand against ArticBatch"""
    c = W.case_arm()
    ab = make_batch(c)
    want = launch(ab, c)
    ab.close()
    lib = _lib.load()
    m = c["m"]
    h = ctypes.c_void_p()
    _lib.check(lib.mh_artic_batch_create_wrench(ctypes.byref(m), None, B, A.MH_ARTIC_CREATE_REPORT, ctypes.byref(h)))
    try:
        dev = torch.device("cuda", lib.mh_artic_batch_device(h))
        q, qd, aux = c["q"].copy(), c["qd"].copy(), S.new_aux(B)
        _lib.check(lib.mh_artic_batch_upload(h, q.ctypes.data, qd.ctypes.data, aux.ctypes.data))
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        dr = c["drive"]; dt_ = {k: T(a) for k, a in dr.arrays.items() if a is not None}
        d = A.mh_artic_drive(terms=dr.terms, rows=dr.rows, **{k: t.data_ptr() for k, t in dt_.items()})
        wt = T(c["wrench"].arrays["w"])
        w = A.mh_artic_wrench(terms=c["wrench"].terms, rows=c["wrench"].rows, w=wt.data_ptr())
        rep = torch.full((B, N, A.report_slots(m), A.REPORT_PAIR), float("nan"), dtype=torch.float64, device=dev)
        _lib.check(lib.mh_artic_batch_step_wrench(h, None, ctypes.c_double(c["dt"]), N, ctypes.byref(d), ctypes.byref(w), rep.data_ptr()))
        _lib.check(lib.mh_artic_batch_download(h, q.ctypes.data, qd.ctypes.data, aux.ctypes.data))
        got = dict(q=q, qd=qd, aux=aux, pose=None, report=rep.cpu().numpy())
    finally:
        lib.mh_artic_batch_destroy(h)
    assert got["q"].tobytes() == want["q"].tobytes() and got["qd"].tobytes() == want["qd"].tobytes() and got["report"].tobytes() == want["report"].tobytes()
    check(got, want)


def test_refusals_that_need_a_batch():
    """a wrench on a batch of another create; report_dev on a batch without the report flag; the Python side says the same before the call"""
    c = W.case_chain(W.CRB, 1)
    wt = torch.zeros((B, 3, 6), dtype=torch.float64, device="cuda")
    w = A.mh_artic_wrench(terms=A.MH_LINK_WRENCH, rows=1, w=wt.data_ptr())
    lib = _lib.load()
    pb = make_batch(c, wrench=False)
    assert _c_step(pb, c, w) == MH_ERR_INVALID_ARG and "not created by mh_artic_batch_create_wrench" in lib.mh_last_error().decode()
    with pytest.raises(ValueError, match="wrench=True"):
        pb.step(c["dt"], N, wrench=A.LinkWrench(w=wt))
    pb.close()
    ab = make_batch(c)
    assert _c_step(ab, c, w, wt.data_ptr()) == MH_ERR_INVALID_ARG and lib.mh_last_error().decode().startswith("report_dev")
    assert _c_step(ab, c, None, wt.data_ptr()) == MH_ERR_INVALID_ARG and lib.mh_last_error().decode().startswith("report_dev")
    ab.close()
