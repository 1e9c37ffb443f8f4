"""Episodes on the device on the GPU (include/moby_hip_artic.h, "Episodes on the device"): mh_artic_batch_reset_dev, _status_dev and _link_poses_dev
against the CPU reference of tests/artic_reset_ref.py (a reset is array assignment, the stepping the per-world report reference) and against the
host routes they stand in for (download / edit / upload + set_base_pose; download's aux; link_poses) -- every comparison bit for bit, no tolerance.
The cases' coverage is proven on the reference by tests/test_artic_reset.py."""
import numpy as np
import pytest
import torch

from moby_amd import _lib
from moby_amd import artic as A
from moby_amd import scene as S
from tests import artic_params_ref as P
from tests import artic_report_ref as R
from tests import artic_reset_ref as E
from tests.test_artic_box_gpu import same
from tests.test_artic_params_gpu import check_launch, make_batch, nan_report

pytestmark = pytest.mark.gpu
B = E.B
NAN = float("nan")


@pytest.fixture(scope="module")
def ref():
    return R.build_report_ref()


def dev_rows(ab, a, worlds=None, dtype=torch.float64):
    """a host array as a tensor on the batch's device; with `worlds`, every other world's row is NaN (the reset must not read it)"""
    a = np.array(a, copy=True)
    if worlds is not None:
        a[[w for w in range(a.shape[0]) if w not in worlds]] = NAN
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(ab._device())


def mask_of(ab, worlds):
    m = np.zeros(ab.B, dtype=np.int32); m[list(worlds)] = 1
    return torch.from_numpy(m).to(ab._device())


@pytest.mark.parametrize("case", E.CASES, ids=P.case_id)
def test_reset_worlds_step_as_fresh_worlds(ref, case):
    """launch 0, reset with mask [0, 1, 0, -7, 1, 0] (the floating box pendulum: [0, 1, 0, -7, 0, 1], tests/artic_reset_ref.py) from rows whose unmasked worlds are NaN, launch 1: all six worlds against the reference after each
    launch -- the nonzero rule, unread rows, untouched worlds, and nothing hidden surviving a reset on the no-slip, the Drumwright-Shell, the
    stabiliser, the pose and the plain-kernel routes"""
    m, q0, qd0, dt, n, p, pose0, want, after = E.reset_run(ref, case)
    pose = case[1] == "pose"
    report = case[4] is not None
    mask, worlds = E.mask_of(case)
    ab = make_batch(m, q0, qd0, case[1], p, report)
    for launch in range(2):
        if launch == 1:
            ab.reset(mask=torch.from_numpy(mask).to(ab._device()), q=dev_rows(ab, q0, worlds), qd=dev_rows(ab, qd0, worlds),
                     pose=dev_rows(ab, pose0, worlds) if pose else None)
            q, qd, aux = ab.download()
            assert np.array_equal(q, after["q"]) and np.array_equal(qd, after["qd"]) and (not pose or np.array_equal(ab.base_pose(), after["pose"]))
            for w in worlds:
                assert aux[w].tobytes() == S.new_aux(1)[0].tobytes(), w      # the whole record, padding included
        rep = nan_report(ab, n) if report else None
        ab.step(dt, n, drive=want[launch]["drive"], report=rep)
        check_launch(ab, want[launch], n, rep, pose)
    ab.close()


def test_the_box_family_with_the_stabiliser_after_a_reset(ref):
    """a plain batch of four_feet (boxes only: mh_artic_box.hip) with the stabiliser, whose rows and distances live in the batch's workspace: launch,
    reset of worlds {1, 3, 4}, launch -- all six worlds against the reference after each"""
    m, q0, qd0, dt, n, want = E.box_family_run(ref)
    ab = A.ArticBatch(m, np.zeros_like(q0), np.zeros_like(qd0))
    ab.upload(q0, qd0, S.new_aux(B))
    for launch in range(2):
        if launch == 1:
            ab.reset(mask=torch.from_numpy(E.MASK).to(ab._device()), q=dev_rows(ab, q0, E.RESET_WORLDS), qd=dev_rows(ab, qd0, E.RESET_WORLDS))
        ab.step(dt, n)
        same(ab.download(), (want[launch]["q"], want[launch]["qd"], want[launch]["aux"]), B)
    ab.close()


KINDS = [("plain", ("chain6", "angles", False, False), {}), ("spheres", ("arm_on_table", "angles", True, False), {}),
         ("report", ("mixed_all", "angles", False, False), dict(report=True)), ("params", ("mixed_all", "pose", True, True), dict(params=True, report=True)),
         ("wrench", ("floating_box_pendulum", "pose", False, False), dict(params=True, wrench=True))]


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
def test_reset_equals_upload_on_every_batch_kind(ref, kind):
    """one batch takes reset, its twin download, the same edit on the host, upload (+ set_base_pose): the aux records byte for byte after it, and q, qd,
    aux and the pose after one more launch.  The pose rows carry quaternions of length 1.7: the device's normalisation is the host setter's"""
    _, key, kw = kind
    case = next(c for c in P.CASES if c[:4] == key)
    m, q0, qd0, dt, n, p = P.case_model(ref, case)
    pose = case[1] == "pose"
    kw = dict(kw, params=p) if kw.get("params") else kw
    worlds = E.RESET_WORLDS
    q_new, qd_new = q0.copy(), 0.5 * qd0

    def batch():
        ab = A.ArticBatch(m, np.zeros_like(q0), np.zeros_like(qd0), base_coords=case[1], **kw)
        ab.upload(q0, qd0, S.new_aux(B))
        ab.step(dt, n)
        return ab

    a, t = batch(), batch()
    P_new = None
    if pose:
        P_new = a.base_pose(); P_new[:, :3] += 0.01; P_new[:, 3:] *= 1.7
    a.reset(mask=torch.from_numpy(E.MASK).to(a._device()), q=dev_rows(a, q_new, worlds), qd=dev_rows(a, qd_new, worlds), pose=dev_rows(a, P_new, worlds) if pose else None)
    q, qd, aux = t.download()
    for w in worlds:
        q[w], qd[w], aux[w] = q_new[w], qd_new[w], S.new_aux(1)[0]
    t.upload(q, qd, aux)
    if pose:
        Pt = t.base_pose(); Pt[list(worlds)] = P_new[list(worlds)]
        t.set_base_pose(Pt)
    for both in range(2):
        ga, gt = a.download(), t.download()
        assert np.array_equal(ga[0], gt[0]) and np.array_equal(ga[1], gt[1]) and ga[2].tobytes() == gt[2].tobytes()
        same(ga, gt, B)
        if pose:
            assert np.array_equal(a.base_pose(), t.base_pose())
            assert (np.abs(np.linalg.norm(a.base_pose()[:, 3:], axis=1) - 1.0) < 1e-15).all()
        if both == 0:
            assert (ga[2]["steps"][list(worlds)] == 0).all() and (ga[2]["steps"][[0, 2, 5]] > 0).all()
            a.step(dt, n); t.step(dt, n)
    assert (ga[2]["steps"][list(worlds)] > 0).all() and (ga[2]["steps"][list(worlds)] <= n).all()      # the reset worlds' counters started again
    a.close(); t.close()


def test_a_failed_world_comes_back(ref):
    """world 1 carries MH_WORLD_LCP_FAILED and steps = 7: a launch passes it over; reset of world 1 alone, then a launch: it follows the reference from
    a fresh record, and status_into shows 0 for it"""
    case = E.CASES[1]
    m, q0, qd0, dt, n, p = P.case_model(ref, case)
    aux0 = S.new_aux(B); aux0["status"][1] = S.MH_WORLD_LCP_FAILED; aux0["steps"][1] = 7
    ab = make_batch(m, q0, qd0, case[1], p, True)
    ab.upload(q0, qd0, aux0)
    q, qd, aux = q0.copy(), qd0.copy(), aux0.copy()
    st = torch.full((B,), -1, dtype=torch.int32, device=ab._device())
    for launch in range(2):
        if launch == 1:
            ab.reset(mask=mask_of(ab, (1,)), q=dev_rows(ab, q0, (1,)), qd=dev_rows(ab, qd0, (1,)))
            E.reset_worlds((1,), q, qd, aux, None, q0, qd0, None)
        rep = nan_report(ab, n)
        ab.step(dt, n, report=rep)
        want = P.step_worlds(ref, m, p, q, qd, aux, dt, n)
        check_launch(ab, dict(q=q, qd=qd, aux=aux, report=want), n, rep, False)
        ab.status_into(st)
        got = st.cpu().numpy()
        assert np.array_equal(got, aux["status"])
        if launch == 0:
            assert got[1] == S.MH_WORLD_LCP_FAILED and aux["steps"][1] == 7 and np.array_equal(ab.download()[0][1], q0[1])
        else:
            assert got[1] == 0 and aux["steps"][1] == n and aux["lcp_solves"][1] > 0
    ab.close()


def test_null_arguments(ref):
    """a NULL mask resets all six worlds; q=None leaves the positions while qd and aux are replaced; pose=None on a pose batch leaves the pose"""
    case = E.CASES[2]
    m, q0, qd0, dt, n, p, pose0, want, _ = E.reset_run(ref, case)
    ab = make_batch(m, q0, qd0, case[1], p, True)
    ab.step(dt, n)
    qd_new = 0.25 * qd0
    ab.reset(qd=dev_rows(ab, qd_new))
    q, qd, aux = ab.download()
    assert np.array_equal(q, want[0]["q"]) and np.array_equal(qd, qd_new) and aux.tobytes() == S.new_aux(B).tobytes()
    assert np.array_equal(ab.base_pose(), want[0]["pose"]) and not np.array_equal(want[0]["pose"], pose0)
    rep = nan_report(ab, n)
    ab.step(dt, n, report=rep)
    Pp = want[0]["pose"].copy()
    r = P.step_worlds(ref, m, p, q, qd, aux, dt, n, pose=Pp)
    check_launch(ab, dict(q=q, qd=qd, aux=aux, pose=Pp, report=r), n, rep, True)
    ab.reset()                                                           # nothing given: fresh records, state and pose stay
    g = ab.download()
    assert np.array_equal(g[0], q) and np.array_equal(g[1], qd) and g[2].tobytes() == S.new_aux(B).tobytes() and np.array_equal(ab.base_pose(), Pp)
    ab.close()


def test_stream_order(ref):
    """step, reset, state_into, step on a torch stream that is not the default one, no host synchronisation between them (the drives are device
    tensors, so nothing is staged): one synchronisation, then test 1's expectation; the tensors of state_into hold the reset values"""
    case = E.CASES[0]
    m, q0, qd0, dt, n, p, pose0, want, after = E.reset_run(ref, case)
    ab = make_batch(m, q0, qd0, case[1], p, True)
    dev = ab._device()
    drives = [A.Drive(**{k: (None if a is None else dev_rows(ab, a)) for k, a in w["drive"].arrays.items()}) for w in want]
    mask = torch.from_numpy(E.MASK).to(dev)
    rows = [dev_rows(ab, q0, E.RESET_WORLDS), dev_rows(ab, qd0, E.RESET_WORLDS), dev_rows(ab, pose0, E.RESET_WORLDS)]
    reps = [nan_report(ab, n), nan_report(ab, n)]
    q_t = torch.full((B, m.nj), NAN, dtype=torch.float64, device=dev); qd_t = q_t.clone(); pose_t = torch.full((B, 7), NAN, dtype=torch.float64, device=dev)
    st_t = torch.full((B,), -1, dtype=torch.int32, device=dev); time_t = torch.full((B,), NAN, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
    torch.cuda.synchronize(dev)
    sh = stream.cuda_stream
    ab.step(dt, n, stream=sh, drive=drives[0], report=reps[0])
    ab.reset(mask=mask, q=rows[0], qd=rows[1], pose=rows[2], stream=sh)
    ab.state_into(q_t, qd_t, stream=sh); ab.base_pose_into(pose_t, stream=sh); ab.status_into(st_t, time_t, stream=sh)
    ab.step(dt, n, stream=sh, drive=drives[1], report=reps[1])
    stream.synchronize()
    assert np.array_equal(q_t.cpu().numpy(), after["q"]) and np.array_equal(qd_t.cpu().numpy(), after["qd"]) and np.array_equal(pose_t.cpu().numpy(), after["pose"])
    assert np.array_equal(st_t.cpu().numpy(), after["aux"]["status"]) and np.array_equal(time_t.cpu().numpy(), after["aux"]["time"])
    assert (time_t.cpu().numpy()[list(E.RESET_WORLDS)] == 0.0).all() and (time_t.cpu().numpy()[[0, 2, 5]] > 0.0).all()
    assert np.array_equal(reps[0].cpu().numpy(), want[0]["report"])
    check_launch(ab, want[1], n, reps[1], True)
    ab.close()


def test_status_into_is_downloads_status_and_time(ref):
    m, q0, qd0, dt = P.chain6()
    q0, qd0 = q0[:B].copy(), qd0[:B].copy()
    aux0 = S.new_aux(B); aux0["status"][2] = S.MH_WORLD_LCP_FAILED | S.MH_WORLD_IMPACT_TOL; aux0["time"][2] = 0.375; aux0["time"][4] = 1.5
    ab = A.ArticBatch(m, q0, qd0, aux0)
    ab.step(dt, 20)
    dev = ab._device()
    st = torch.full((B,), -1, dtype=torch.int32, device=dev); tm = torch.full((B,), NAN, dtype=torch.float64, device=dev)
    st1, tm1 = st.clone(), tm.clone()
    ab.status_into(st, tm); ab.status_into(status_t=st1); ab.status_into(time_t=tm1)
    aux = ab.download()[2]
    ab.close()
    for s, t in ((st, tm), (st1, tm1)):
        assert np.array_equal(s.cpu().numpy(), aux["status"]) and np.array_equal(t.cpu().numpy(), aux["time"])
    assert aux["status"][2] == 3 and aux["time"][2] == 0.375 and aux["time"][4] > 1.5 and (aux["steps"][[0, 1, 3, 4, 5]] == 20).all()


@pytest.mark.parametrize("params", [False, True], ids=["shared_image", "per_world_images"])
@pytest.mark.parametrize("coords", ["angles", "pose"])
def test_link_poses_into_equals_link_poses(ref, coords, params):
    """the four launchers -- k_artic_fwd_dyn, its pose form, and the per-world-parameters forms of both -- on a caller's stream into a caller's tensor:
    bit-equal to the host call, on states a launch has moved"""
    case = E.CASES[0]
    m, q0, qd0, dt, n, p = P.case_model(ref, case)
    ab = make_batch(m, q0, qd0, coords, p if params else None, False)
    ab.step(dt, 10)
    want = ab.link_poses()
    dev = ab._device()
    t = torch.full((B, m.nj, 12), NAN, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    ab.link_poses_into(t, stream=stream.cuda_stream)
    stream.synchronize()
    t0 = torch.full_like(t, NAN)
    ab.link_poses_into(t0)
    ab.close()
    assert np.isfinite(want).all() and np.array_equal(t.cpu().numpy(), want) and np.array_equal(t0.cpu().numpy(), want)
    assert not np.array_equal(want[0], want[1])


def test_refusals_that_need_a_device(ref):
    m, q0, qd0, dt = P.chain6()
    q0, qd0 = q0[:B].copy(), qd0[:B].copy()
    ab = A.ArticBatch(m, q0, qd0)
    dev = ab._device()
    z = lambda *sh, **kw: torch.zeros(sh, dtype=kw.get("dtype", torch.float64), device=kw.get("device", dev))
    with pytest.raises(_lib.MobyHipError, match="angle coordinates") as e:
        ab.reset(pose=z(B, 7))
    assert e.value.code == _lib.MH_ERR_INVALID_ARG
    with pytest.raises(_lib.MobyHipError, match="both NULL") as e:
        ab.status_into()
    assert e.value.code == _lib.MH_ERR_INVALID_ARG
    for call in (lambda: ab.reset(q=z(B, m.nj + 1)), lambda: ab.reset(qd=z(B, m.nj, device="cpu")), lambda: ab.reset(q=z(B, m.nj, dtype=torch.float32)),
                 lambda: ab.reset(mask=z(B + 1, dtype=torch.int32)), lambda: ab.reset(mask=z(B, dtype=torch.int32, device="cpu")),
                 lambda: ab.reset(mask=z(2 * B, dtype=torch.int32)[::2]), lambda: ab.status_into(z(B)), lambda: ab.status_into(time_t=z(B, dtype=torch.int32)),
                 lambda: ab.status_into(z(B - 1, dtype=torch.int32)), lambda: ab.link_poses_into(z(B, m.nj, 11)), lambda: ab.link_poses_into(z(B, m.nj, 12, device="cpu"))):
        with pytest.raises(ValueError, match="expected a contiguous"):
            call()
    for bad in (z(B), z(B, dtype=torch.bool), z(B, dtype=torch.int64)):
        with pytest.raises(ValueError, match="convert"):
            ab.reset(mask=bad)
    assert np.array_equal(ab.download()[0], q0)                          # nothing was written by a refused call
    ab.close()
