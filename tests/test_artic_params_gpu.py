"""Per-world parameters of the articulated stepper on the GPU (include/moby_hip_artic.h, "Per-world parameters"): the eight kernels of mh_artic_pw.hip /
mh_artic_pw_pose.hip against one reference run per world on "the model with record w written into it" (tests/artic_params_ref.py), bit for bit -- q,
qd, every aux field, the base pose and every report row; a batch whose records all equal the model against the batch of mh_artic_batch_create; the
setters; the model queries per world; the refusals that need a device.  The cases' coverage is proven on the reference by tests/test_artic_params.py."""
import numpy as np
import pytest
import torch

from moby_amd import _lib
from moby_amd import artic as A
from moby_amd import scene as S
from tests import artic_boxsphere_ref as BS
from tests import artic_params_ref as P
from tests import artic_report_ref as R
from tests.test_artic_box_gpu import same

pytestmark = pytest.mark.gpu
B = P.B


@pytest.fixture(scope="module")
def ref():
    return R.build_report_ref()


def nan_report(ab, n):
    return torch.full((ab.B, n, ab.report_slots, A.REPORT_PAIR), float("nan"), dtype=torch.float64, device=ab._device())


def make_batch(m, q0, qd0, coords, params, report):
    """a batch created at q = 0, switched to its coordinates there, then given its start state"""
    ab = A.ArticBatch(m, np.zeros_like(q0), np.zeros_like(qd0), base_coords=coords, report=report, params=params)
    ab.upload(q0, qd0, S.new_aux(q0.shape[0]))
    return ab


def check_launch(ab, w, n, rep, pose):
    same(ab.download(), (w["q"], w["qd"], w["aux"]), ab.B)
    if pose:
        assert np.array_equal(ab.base_pose(), w["pose"]), "max |dP| = %.3e" % np.nanmax(np.abs(ab.base_pose() - w["pose"]))
    if rep is not None:
        got = rep.cpu().numpy()
        assert not np.isnan(got).any(), "%d entries of the report were not written" % int(np.isnan(got).sum())
        assert np.array_equal(got, w["report"]), "max |d row| = %.3e in %d rows" % (np.abs(got - w["report"]).max(), int((got != w["report"]).any(axis=-1).sum()))


@pytest.mark.parametrize("case", P.CASES, ids=P.case_id)
def test_every_world_steps_as_its_own_model(ref, case):
    """k_artic_step_pw[_stab][_pose][_drive] -- all eight between the cases, CRB and FSAB -- on the mixed model, the floating box pendulum, a sphere-only
    arm, the 16-joint arm (the largest LDS image) and a 6-link chain with no geometry at all; 6 worlds whose records vary masses, inertias, centres of
    mass, link offsets, limits, restitution, gravity, sphere radii, box sizes and centres, the plane frame and mu on both sides of 100; two launches, a
    held drive row then a row per step"""
    m, q0, qd0, dt, n, p, want = P.reference_run(ref, case)
    pose = case[1] == "pose"
    report = case[4] is not None                                     # (a model without geometry has no slot: no report batch)
    ab = make_batch(m, q0, qd0, case[1], p, report)
    if pose:
        assert np.array_equal(ab.base_pose(), P.world_pose(m, p))     # each world's start pose from its own record
    for launch in range(2):
        w = want[launch]
        rep = nan_report(ab, n) if report else None
        ab.step(dt, n, drive=w["drive"], report=rep)
        check_launch(ab, w, n, rep, pose)
    ab.close()
    assert (want[-1]["aux"]["lcp_solves"] > 0).any()


EQUAL_CASES = [c for c in P.CASES if (c[0], c[1], c[3]) in (("chain6", "angles", False), ("chain6", "angles", True), ("arm_on_table", "angles", False),
                                                           ("mixed_all", "pose", True), ("floating_box_pendulum", "angles", True))]


@pytest.mark.parametrize("case", EQUAL_CASES, ids=P.case_id)
def test_equal_records_are_the_plain_batch(ref, case):
    """records that all equal the model (given, and NULL through the C entry) against the batch of mh_artic_batch_create -- which takes the plain
    kernels for the chain without geometry, the sphere kernels for the arm on the table, the box-sphere kernels for the others: bit for bit"""
    m, q0, qd0, dt, n, _ = P.case_model(ref, case)
    pose = case[1] == "pose"
    rng = np.random.default_rng(5)
    drives = [P.case_drive(rng, m.nj, n, launch) if case[2] else None for launch in range(2)]

    def run(ab):
        ab.upload(q0, qd0, S.new_aux(B))
        for d in drives:
            ab.step(dt, n, drive=d)
        out = ab.download() + ((ab.base_pose(),) if pose else ())
        ab.close()
        return out

    z = np.zeros_like(q0)
    plain = run(A.ArticBatch(m, z, z, base_coords=case[1]))
    assert (plain[2]["lcp_solves"] > 0).any()
    if case[0] == "chain6":          # (the plain kernels do not freeze a world that carries MH_WORLD_UNSUPPORTED, the contact kernels do: none here)
        assert not (plain[2]["status"] & S.MH_WORLD_UNSUPPORTED).any()
    for other in (run(A.ArticBatch(m, z, z, base_coords=case[1], params=A.make_params(m, B))), run(A.ArticBatch(m, z, z, base_coords=case[1], params=True))):
        same(other[:3], plain[:3], B)
        if pose:
            assert np.array_equal(other[3], plain[3])


def test_a_report_batch_under_key_20_is_the_report_batch(ref):
    """mh_debug_set(20, 1) sends a report batch through the per-world-parameters kernels with B images of the model: state and rows bit for bit"""
    case = P.CASES[0]
    m, q0, qd0, dt, n, _ = P.case_model(ref, case)
    lib = _lib.load()
    rng = np.random.default_rng(6)
    d = P.case_drive(rng, m.nj, n, 1)

    def run(key20):
        _lib.check(lib.mh_debug_set(20, key20))
        try:
            ab = make_batch(m, q0, qd0, case[1], None, True)
        finally:
            _lib.check(lib.mh_debug_set(20, 0))
        rep = nan_report(ab, n)
        ab.step(dt, n, drive=d, report=rep)
        out = ab.download() + (ab.base_pose(), rep.cpu().numpy())
        with pytest.raises(_lib.MobyHipError, match="not created by mh_artic_batch_create_params"):      # its images are not records to set
            ab.set_params(A.make_params(m, 1))
        ab.close()
        return out

    a, b = run(0), run(1)
    same(b[:3], a[:3], B)
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and (a[4][..., 1] > 0.0).any()


@pytest.mark.parametrize("dev", [False, True], ids=["set_params", "set_params_dev"])
def test_setters_change_exactly_their_worlds(ref, dev):
    """set_params(first=2, count=3) between two launches -- and set_params_dev from a tensor on the stepping stream -- gives worlds 2..4 other records:
    every world matches the per-world reference run that switches records between the launches, and the others match the unswitched run too"""
    case = P.CASES[1]
    m, q0, qd0, dt, n, p, want = P.reference_run(ref, case, P.switched, "switched")
    keep = P.reference_run(ref, case)[-1]
    ab = make_batch(m, q0, qd0, case[1], p, True)
    stream = torch.cuda.Stream(device=ab._device()) if dev else None
    sh = None if stream is None else stream.cuda_stream
    rep = nan_report(ab, n)
    if stream is not None: stream.wait_stream(torch.cuda.current_stream(ab._device()))
    ab.step(dt, n, stream=sh, report=rep)
    new = want[1]["params"][2:5]
    if dev:
        with torch.cuda.stream(stream):
            t = torch.from_numpy(np.ascontiguousarray(new).view(np.float64).reshape(3, A.PARAMS_DOUBLES).copy()).to(ab._device(), non_blocking=False)
        ab.set_params_dev(t, first=2, stream=sh)
    else:
        check_launch(ab, want[0], n, rep, False)
        ab.set_params(new, first=2)
    rep2 = nan_report(ab, n)
    if stream is not None: stream.wait_stream(torch.cuda.current_stream(ab._device()))
    ab.step(dt, n, stream=sh, report=rep2)
    torch.cuda.synchronize(ab._device())
    check_launch(ab, want[1], n, rep2, False)
    q = ab.download()[0]
    for w in range(B):
        assert np.array_equal(q[w], keep[1]["q"][w]) == (w not in (2, 3, 4)), w
    ab.close()


@pytest.mark.parametrize("coords", ["angles", "pose"])
def test_model_queries_read_each_worlds_image(ref, coords):
    """fwd_dyn (qdd and H), link_poses and jacobian of a params batch equal, per world, those of a one-world plain batch of that world's model"""
    case = P.CASES[0]
    m, q0, qd0, dt, n, p = P.case_model(ref, case)
    rng = np.random.default_rng(9)
    tau = rng.uniform(-1.0, 1.0, (B, m.nj)); pts = rng.uniform(-0.5, 0.5, (B, 3)); link = 6
    ab = make_batch(m, q0, qd0, coords, p, False)
    qdd, H = ab.fwd_dyn(tau); poses = ab.link_poses(); J = ab.jacobian(link, pts)
    ab.close()
    base = make_batch(m, q0, qd0, coords, None, False)
    H0 = base.fwd_dyn(tau)[1]
    base.close()
    for w in range(B):
        one = make_batch(P.model_of_world(m, p, w), q0[w:w + 1], qd0[w:w + 1], coords, None, False)
        qdd1, H1 = one.fwd_dyn(tau[w:w + 1]); poses1 = one.link_poses(); J1 = one.jacobian(link, pts[w:w + 1])
        one.close()
        assert np.array_equal(qdd[w], qdd1[0]) and np.array_equal(H[w], H1[0]) and np.array_equal(poses[w], poses1[0]) and np.array_equal(J[w], J1[0]), w
        assert not np.array_equal(H[w], H0[w])                          # ... and not the shared model's


def test_refusals_that_need_a_device(ref):
    """a batch not created with records, a range outside the batch, a refused record (none is written), a tensor of the wrong dtype, shape or device"""
    m = BS.mixed_all()[0]
    z = np.zeros((B, m.nj))
    plain = A.ArticBatch(m, z, z)
    for call in (lambda: plain.set_params(A.make_params(m, 1)), lambda: plain.set_params_dev(torch.zeros((1, A.PARAMS_DOUBLES), dtype=torch.float64, device=plain._device()))):
        with pytest.raises(_lib.MobyHipError, match="not created by mh_artic_batch_create_params") as e:
            call()
        assert e.value.code == _lib.MH_ERR_INVALID_ARG
    plain.close()
    p = P.vary(m, B, 3, P.NOSLIP)
    ab = A.ArticBatch(m, z, z, params=p)
    dev = ab._device()
    for first, count in ((4, 3), (-1, 2), (B, 1), (0, B + 1)):
        with pytest.raises(_lib.MobyHipError, match="outside the batch"):
            ab.set_params(A.make_params(m, count), first=first)
        with pytest.raises(_lib.MobyHipError, match="outside the batch"):
            ab.set_params_dev(torch.zeros((count, A.PARAMS_DOUBLES), dtype=torch.float64, device=dev), first=first)
    for bad in (torch.zeros((2, A.PARAMS_DOUBLES), dtype=torch.float32, device=dev), torch.zeros((2, A.PARAMS_DOUBLES - 1), dtype=torch.float64, device=dev),
                torch.zeros((2, A.PARAMS_DOUBLES), dtype=torch.float64), torch.zeros((2 * A.PARAMS_DOUBLES,), dtype=torch.float64, device=dev),
                torch.zeros((A.PARAMS_DOUBLES, 2), dtype=torch.float64, device=dev).t()):
        with pytest.raises(ValueError, match="expected a contiguous float64 tensor"):
            ab.set_params_dev(bad)
    with pytest.raises(ValueError, match="PARAMS_DTYPE"):
        ab.set_params(np.zeros((2, A.PARAMS_DOUBLES)))
    # a refused record: none of the three is written, the batch steps as before
    q0 = np.tile(np.array([0.0, 0.3, 0.0, 0.0, 0.0, 0.0, 0.1, 0.0]), (B, 1))
    ab.upload(q0, z, S.new_aux(B))
    new = p[[5, 0, 1]].copy(); new["mass"][2, 6] = -1.0
    with pytest.raises(_lib.MobyHipError, match=r"world 4: link 6: mass"):
        ab.set_params(new, first=2)
    ab.step(1e-3, 20)
    got = ab.download()
    ab.close()
    q, qd, aux = q0.copy(), z.copy(), S.new_aux(B)
    P.step_worlds(ref, m, p, q, qd, aux, 1e-3, 20)
    same(got, (q, qd, aux), B)
