"""The articulated stepper's contact report on the GPU (include/moby_hip_artic.h, "Contact report"): the eight kernels of mh_artic_rp.hip /
mh_artic_rp_pose.hip against the report reference (tests/native/artic_report_ref.cpp) bit for bit -- q, qd, every aux field, the base pose and
every row of the report -- on the cases of tests/artic_report_ref.py (their coverage is proven on the reference's run by tests/test_artic_report.py);
a report batch that writes nothing and a batch under mh_debug_set(19, 1) against the plain batch; a world that is passed over; the refusals."""
import numpy as np
import pytest
import torch

from moby_amd import _lib
from moby_amd import artic as A
from moby_amd import scene as S
from tests import artic_report_ref as R
from tests.test_artic_box_gpu import same

pytestmark = pytest.mark.gpu
B = R.B


@pytest.fixture(scope="module")
def ref():
    return R.build_report_ref()


def nan_report(ab, n):
    """the launch's report tensor, filled with NaN so that a row the kernel did not write shows"""
    return torch.full((ab.B, n, ab.report_slots, A.REPORT_PAIR), float("nan"), dtype=torch.float64, device=ab._device())


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_report_kernels_match_the_reference(ref, case):
    """k_artic_step_rp[_stab][_pose][_drive] -- all eight, each at least twice -- on an arm over a static box, an arm over a box on a slider (both
    impact models), a floating box hit by a pendulum, the mixed model, a 12-joint chain (the C X C' blocks in the workspace), a 16-joint chain (the
    largest LDS image), four box feet (16 contacts: every accumulator) and a sphere-only arm; CRB and FSAB; 64 worlds; two launches, a held drive
    row then a row per step"""
    m, q0, qd0, dt, n, want = R.reference_run(ref, case)
    pose = case[1] == "pose"
    ab = A.ArticBatch(m, np.zeros_like(q0), np.zeros_like(qd0), base_coords=case[1], report=True)
    ab.upload(q0, qd0, S.new_aux(B))
    if pose:
        assert np.array_equal(ab.base_pose(), R.model_pose(m, B))
    for launch in range(2):
        w = want[launch]
        rep = nan_report(ab, n)
        ab.step(dt, n, drive=w["drive"], report=rep)
        same(ab.download(), (w["q"], w["qd"], w["aux"]), B)
        if pose:
            assert np.array_equal(ab.base_pose(), w["pose"]), "max |dP| = %.3e" % np.nanmax(np.abs(ab.base_pose() - w["pose"]))
        got = rep.cpu().numpy()
        assert not np.isnan(got).any(), "%d entries of the report were not written" % int(np.isnan(got).sum())
        assert np.array_equal(got, w["report"]), "max |d row| = %.3e in %d rows" % (np.abs(got - w["report"]).max(), int((got != w["report"]).any(axis=-1).sum()))
    ab.close()
    assert (want[-1]["aux"]["lcp_solves"] > 0).any() and (want[-1]["report"][..., 1] > 0.0).any()


NULL_CASES = [c for c in R.CASES if (c[0], c[1]) in (("mixed_all", "angles"), ("arm_static", "angles"), ("four_feet", "pose"), ("arm_on_table", "angles"))][:4]


@pytest.mark.parametrize("case", NULL_CASES, ids=R.case_id)
def test_a_report_batch_that_writes_nothing_equals_the_plain_batch(ref, case):
    """the same model on a batch of mh_artic_batch_create (whatever kernels that takes: box-sphere, box, sphere) and on a report batch stepped with
    report=None, and -- where the plain batch would take the box-sphere kernels -- on a plain batch created under mh_debug_set(19, 1): bit for bit"""
    m, q0, qd0, dt, n = R.case_model(ref, case)
    lib = _lib.load()

    def run(report, key19):
        _lib.check(lib.mh_debug_set(19, key19))
        try:
            ab = A.ArticBatch(m, np.zeros_like(q0), np.zeros_like(qd0), base_coords=case[1], report=report)
        finally:
            _lib.check(lib.mh_debug_set(19, 0))
        ab.upload(q0, qd0, S.new_aux(B))
        ab.step(dt, n); ab.step(dt, n)
        out = ab.download() + ((ab.base_pose(),) if case[1] == "pose" else ())
        ab.close()
        return out

    plain = run(False, 0)
    assert (plain[2]["lcp_solves"] > 0).any()
    for other in [run(True, 0)] + ([run(False, 1)] if case[0] in ("mixed_all", "arm_static") else []):
        same(other[:3], plain[:3], B)
        if case[1] == "pose":
            assert np.array_equal(other[3], plain[3])


def test_a_world_that_is_passed_over_writes_zero_rows(ref):
    """a world uploaded with MH_WORLD_LCP_FAILED keeps its state and writes all-zero rows for every step; its neighbours are the reference's"""
    case = next(c for c in R.CASES if c[0] == "mixed_all" and c[1] == "angles")
    m, q0, qd0, dt, n = R.case_model(ref, case)
    aux0 = S.new_aux(B); aux0["status"][5] = S.MH_WORLD_LCP_FAILED
    ab = A.ArticBatch(m, q0, qd0, aux0.copy(), report=True)
    rep = nan_report(ab, n)
    ab.step(dt, n, report=rep)
    got = rep.cpu().numpy()
    q, qd, aux = q0.copy(), qd0.copy(), aux0.copy()
    want = ref.step_report(m, q, qd, aux, dt, n)
    same(ab.download(), (q, qd, aux), B)
    ab.close()
    assert np.array_equal(got[5], np.zeros_like(got[5]))
    assert np.array_equal(q[5], q0[5]) and aux["steps"][5] == 0
    assert np.array_equal(got, want) and (got[..., 1] > 0.0).any()


def test_contacts_beyond_the_handler_fold_with_zero_impulse(ref):
    """four box feet flat on the plane and a box-sphere contact: 17 contacts, one more than the impact handler holds.  The mini-step that meets them
    all is refused (MH_WORLD_UNSUPPORTED) and folds every contact with zero impulse, the seventeenth without an accumulator; the rows are the
    reference's"""
    from tests import artic_pair_ref as P
    legs = [P._hinge(-1, (0.0, 0.2, 0.0), (0.0, 0.1, 0.0), mass=0.2, lo=-0.5, hi=0.5)]
    m = A.model_from_links(legs, gravity=P.G, floating_base=dict(R0=np.eye(3), x0=(0.0, 0.06, 0.0), mass=5.0, inertia=np.eye(3)))
    feet = [(5, (x, -0.05, z), np.eye(3), (0.1, 0.02, 0.1)) for x, z in ((-0.4, -0.4), (0.4, -0.4), (-0.4, 0.4), (0.4, 0.4))]
    A.add_spheres(m, [(6, (0.0, 0.2, 0.0), 0.03)], plane_normal=P.UP, mu_coulomb=100.0)
    A.add_boxes(m, feet + [(-1, (0.08, 0.46, 0.0), np.eye(3), (0.1, 0.1, 0.1))], plane_normal=P.UP, mu_coulomb=100.0)
    A.add_box_sphere_pairs(m, [(4, 0)], no_plane=(0,))
    nB, n = 2, 80
    q = np.zeros((nB, 7)); qd = np.zeros((nB, 7)); qd[:, 6] = -0.5; qd[1, 1] = -0.5
    ab = A.ArticBatch(m, q, qd, S.new_aux(nB), report=True)
    rep = nan_report(ab, n)
    ab.step(1e-3, n, report=rep)
    got = rep.cpu().numpy()
    r = [q.copy(), qd.copy(), S.new_aux(nB)]
    want = ref.step_report(m, r[0], r[1], r[2], 1e-3, n)
    same(ab.download(), tuple(r), nB)
    ab.close()
    assert (r[2]["status"] & S.MH_WORLD_UNSUPPORTED).all()
    assert np.array_equal(got, want)
    assert (want[..., 0].sum(axis=-1) == 17.0).any(), "no mini-step met all 17 contacts"


def test_refusals():
    """mh_artic_batch_create_report on a model without geometry; a report tensor on a plain batch; a wrong shape, dtype or device"""
    bare = A.chain_model(3)
    with pytest.raises(_lib.MobyHipError, match="no slot") as e:
        A.ArticBatch(bare, np.zeros((1, 3)), np.zeros((1, 3)), report=True)
    assert e.value.code == _lib.MH_ERR_INVALID_ARG
    from tests import artic_boxsphere_ref as BS
    m = BS.mixed_all()[0]
    z = np.zeros((2, 8))
    plain = A.ArticBatch(m, z, z)
    ok = torch.zeros((2, 3, 7, 8), dtype=torch.float64, device=plain._device())
    with pytest.raises(ValueError, match="report=True"):
        plain.step(1e-3, 3, report=ok)
    assert _lib.load().mh_artic_batch_step_report(plain.handle, None, 1e-3, 3, None, ok.data_ptr()) == _lib.MH_ERR_INVALID_ARG
    plain.close()
    ab = A.ArticBatch(m, z, z, report=True)
    assert ab.report_slots == 7
    for bad in (torch.zeros((2, 3, 7, 7), dtype=torch.float64, device=ab._device()), torch.zeros((2, 4, 7, 8), dtype=torch.float64, device=ab._device()),
                torch.zeros((2, 3, 7, 8), dtype=torch.float32, device=ab._device()), torch.zeros((2, 3, 7, 8), dtype=torch.float64),
                torch.zeros((2, 3, 8, 7), dtype=torch.float64, device=ab._device()).transpose(2, 3)):
        with pytest.raises(ValueError, match="expected a contiguous float64 tensor"):
            ab.step(1e-3, 3, report=bad)
    ab.step(1e-3, 3, report=ok)                                      # ... and the right one is taken
    torch.cuda.synchronize()
    assert not torch.isnan(ok).any()
    ab.close()
