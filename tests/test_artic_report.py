"""The articulated stepper's contact report without a GPU (include/moby_hip_artic.h, "Contact report"): the report reference
(tests/native/artic_report_ref.cpp) against the box-sphere reference it restates, against a hand-written case and against the momentum balance; the
rows' properties; the coverage of the cases the GPU test runs, proven on the reference's own run; the host-side helpers and the build checks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import artic as A
from moby_amd import scene as S
from tests import artic_boxsphere_ref as BS
from tests import artic_report_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53                                  # unit round-off of a double


@pytest.fixture(scope="module")
def ref():
    return R.build_report_ref()


@pytest.fixture(scope="module")
def bs_ref():
    return BS.build_boxsphere_ref()


# ---- 1. the sink adds no physics ----
SINK_CASES = [("arm_slider_box", 100.0), ("arm_slider_box", 0.5), ("mixed_all", 100.0), ("four_feet", 100.0), ("arm_on_table", 100.0)]


@pytest.mark.parametrize("name,mu", SINK_CASES)
def test_the_sink_adds_no_physics(ref, bs_ref, name, mu):
    """with a NULL sink and with a sink the report reference equals artic_boxsphere_ref_step (the existing library's) bit for bit: q, qd and every aux
    field; an arm over a box on a slider (no-slip and mu 0.5), the mixed model, four box feet, a sphere-only arm"""
    m, q0, qd0, dt, n = R.case_model(ref, (name, "angles", False, True, mu, A.MH_ARTIC_CRB))
    want = [q0.copy(), qd0.copy(), S.new_aux(R.B)]
    bs_ref.step(m, want[0], want[1], want[2], dt, n)
    assert (want[2]["lcp_solves"] > 0).any()
    for sink in (False, True):
        got = [q0.copy(), qd0.copy(), S.new_aux(R.B)]
        rep = ref.step_report(m, got[0], got[1], got[2], dt, n, sink=sink)
        assert (rep is None) == (not sink)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, sink)
        for f in want[2].dtype.names:
            assert np.array_equal(got[2][f], want[2][f]), (name, sink, f)
        if sink:
            assert not np.isnan(rep).any() and (rep[..., 1] > 0.0).any()


# ---- 2. / 3. a floating ball ----
M_BALL, I_BALL, R_BALL = 2.0, 0.5, 0.5          # dyadic mass, inertia (isotropic), radius
DT = 2.0 ** -10


def ball(eps, mu, gravity):
    m = A.model_from_links([], gravity=gravity, floating_base=dict(R0=np.eye(3), x0=(0.0, 0.0, 0.0), mass=M_BALL, inertia=np.eye(3) * I_BALL))
    A.add_spheres(m, [(5, (0.0, 0.0, 0.0), R_BALL)], plane_normal=(0.0, 1.0, 0.0), epsilon=eps, mu_coulomb=mu)
    return m


def derived_tolerance():
    """unit round-off x cond(H) x 1000 operations, relative to the largest term.  H, the generalized inertia of the floating ball about its centre of
    mass, is diag(m, m, m, I, I, I) at q = 0 and keeps those eigenvalues under rotation (the inertia is isotropic): cond(H) = max(m, I) / min(m, I)"""
    cond = max(M_BALL, I_BALL) / min(M_BALL, I_BALL)
    return U * cond * 1000.0


def test_a_hand_written_impact(ref):
    """a ball that starts in contact and moves straight into the plane, no gravity, dyadic numbers: the first step's row is one contact with
    [1] = m |v| (1 + eps), [2..4] = that along the plane normal, [5..7] = p [1]"""
    eps, v = 0.5, 1.0
    m = ball(eps, 100.0, (0.0, 0.0, 0.0))
    q = np.zeros((1, 6)); qd = np.zeros((1, 6))
    q[0, :3] = (0.25, R_BALL, -0.75); qd[0, 1] = -v
    aux = S.new_aux(1)
    rep = ref.step_report(m, q, qd, aux, DT, 2)
    tol = derived_tolerance()
    want = M_BALL * v * (1.0 + eps)
    print("derived tolerance: %.3e relative (u = 2^-53, cond(H) = %g, 1000 operations); [1] = %.17g, expected %.17g" % (tol, 4.0, rep[0, 0, 0, 1], want))
    row = rep[0, 0, 0]
    assert row[0] == 1.0
    assert abs(row[1] - want) <= tol * want
    assert np.abs(row[2:5] - want * np.array([0.0, 1.0, 0.0])).max() <= tol * want
    p = np.array([0.25, 0.0, -0.75])                                  # the contact point: under the centre, on the plane
    assert np.abs(row[5:8] - p * row[1]).max() <= tol * want
    assert abs(qd[0, 1] - eps * v) <= tol * v                         # ... and the ball left with eps |v|
    assert np.array_equal(rep[0, 1], np.zeros((1, 8)))                # the second step: in the air


@pytest.mark.parametrize("mu", [100.0, 0.5])
def test_momentum_balance(ref, mu):
    """the same ball under gravity, sliding and bouncing for 50 steps: per step, m (v_end - v_start) - m g dt equals the sum of [2..4] over the slots"""
    g = np.array([0.0, -9.81, 0.0])
    m = ball(0.25, mu, tuple(g))
    nB = 4
    q = np.zeros((nB, 6)); qd = np.zeros((nB, 6))
    q[:, 1] = R_BALL + np.array([0.0, 2.0 ** -12, 2.0 ** -11, 2.0 ** -10])
    qd[:, 0] = 0.5; qd[:, 1] = -0.125; qd[:, 2] = (0.0, 0.25, -0.25, 0.125); qd[:, 3] = (0.0, 0.0, 1.0, -2.0)
    aux = S.new_aux(nB)
    tol = derived_tolerance()
    worst = 0.0; impacts = 0; tangential = 0
    for s in range(50):
        v0 = qd[:, :3].copy()
        rep = ref.step_report(m, q, qd, aux, DT, 1)
        assert (aux["status"] == 0).all()
        lhs = M_BALL * (qd[:, :3] - v0) - M_BALL * g * DT
        rhs = rep[:, 0, :, 2:5].sum(axis=1)
        scale = np.maximum.reduce([np.abs(M_BALL * qd[:, :3]).max(axis=1), np.abs(M_BALL * v0).max(axis=1), np.full(nB, np.abs(M_BALL * g * DT).max()), np.abs(rhs).max(axis=1)])
        err = np.abs(lhs - rhs).max(axis=1) / scale
        worst = max(worst, err.max())
        assert (err <= tol).all(), (s, err, tol)
        assert np.array_equal(A.link_impulses(rep, m)[:, 0, 5], rep[:, 0, 0, 2:5])
        impacts += int((rep[:, 0, 0, 1] > 0.0).sum()); tangential += int((np.abs(rep[:, 0, 0, [2, 4]]).max(axis=1) > 0.0).sum())
    print("mu = %g: worst relative imbalance %.3e against the derived tolerance %.3e; %d impacts, %d with a tangential impulse" % (mu, worst, tol, impacts, tangential))
    assert impacts >= nB and tangential >= 1                           # every ball lands, and friction acts


# ---- 4. row properties ----
def test_row_properties_on_mixed_all(ref):
    """mixed_all with its floating box flat on the plane and its arm swinging down onto the static box: [0] is integer-valued; the rows of the masked
    sphere's and the static box's slots are exactly zero; the flat box counts 4 per folded mini-step; a step with two mini-steps counts both"""
    m, _, dt = BS.mixed_all(eps=0.0)
    q = np.zeros((1, 8)); qd = np.zeros((1, 8))
    q[0, 1] = -0.25; q[0, 6] = 0.6; qd[0, 6] = -5.0
    aux = S.new_aux(1)
    rep, folds, _ = ref.step_report(m, q, qd, aux, dt, 150, diag=True)
    assert aux["status"][0] == 0
    assert np.array_equal(rep[..., 0], np.round(rep[..., 0]))
    ns, nb = m.nspheres, m.nboxes
    assert m.sphere_no_plane == 2 and m.box_link[1] == -1
    assert np.array_equal(rep[:, :, 1], np.zeros_like(rep[:, :, 1]))            # sphere 1 is masked off the plane
    assert np.array_equal(rep[:, :, ns + 1], np.zeros_like(rep[:, :, ns + 1]))  # box 1 is static
    assert np.array_equal(rep[0, :, ns, 0], 4.0 * folds[0])                     # four vertices down, every folded mini-step
    two = np.nonzero(folds[0] == 2)[0]
    assert len(two) >= 1, "no step with two mini-steps"
    assert (rep[0, two, ns, 0] == 8.0).all()
    assert (rep[0, two, ns + nb + 1, 0] >= 1.0).all()                           # ... the one in which the tip met the static box (pair 1)
    assert (rep[0, :, ns, 1] > 0.0).any()


# ---- 5. coverage of the GPU cases ----
def _kinds(m):
    """slot -> kind, for the slots that can carry a contact: a masked sphere and a static box cannot"""
    out = {}
    for s in range(m.nspheres):
        if not (m.sphere_no_plane >> s) & 1: out[s] = "sphere-plane"
    for b in range(m.nboxes):
        if m.box_link[b] >= 0: out[m.nspheres + b] = "box-plane"
    for k in range(m.npairs):
        out[m.nspheres + m.nboxes + k] = "box-sphere pair" if m.pair_kind[k] == A.MH_ARTIC_PAIR_BOX_SPHERE else "sphere pair"
    return out


# The kinds each scene's run must show with a non-zero normal impulse.  A kind the model lists but the run cannot reach is left out, with the reason:
# arm_static's arm is 0.96 long with its shoulder 1.0 above the plane; the two long arms hang 0.9 above it and meet the static box first.
SCENE_KINDS = {
    "arm_static": {"box-sphere pair"},
    "arm_slider_box": {"sphere-plane", "box-plane", "box-sphere pair"},
    "floating_box_pendulum": {"box-plane", "box-sphere pair"},
    "mixed_all": {"sphere-plane", "box-plane", "sphere pair", "box-sphere pair"},
    "long_arm_static": {"box-sphere pair"},
    "long_arm_16": {"box-sphere pair"},
    "four_feet": {"box-plane"},
    "arm_on_table": {"sphere-plane"},
}


@pytest.mark.parametrize("name", list(SCENE_KINDS))
def test_gpu_scenes_cover_what_they_are_for(ref, name):
    """the reference's own run of every case of the scene (the two launches the GPU test makes): every case has a step with more than one folded
    mini-step that carries contacts, and a row whose [1] exceeds the first solve's cn (a restitution pass); over the scene's cases, every slot kind
    the scene reaches has a world with a non-zero [1]"""
    shown = set()
    cases = [c for c in R.CASES if c[0] == name]
    assert cases
    for c in cases:
        m, _, _, _, _, out = R.reference_run(ref, c)
        rep = np.concatenate([o["report"] for o in out], axis=1); folds = np.concatenate([o["folds"] for o in out], axis=1)
        first = np.concatenate([o["first_cn"] for o in out], axis=1)
        assert not np.isnan(rep).any(), "a row was left unwritten"
        assert np.isfinite(out[-1]["q"]).all()
        for slot, kind in _kinds(m).items():
            if (rep[:, :, slot, 1] != 0.0).any(): shown.add(kind)
        multi = int(((folds > 1) & (rep[..., 0].sum(axis=-1) > 0)).sum())
        total = rep[..., 1].sum(axis=-1)
        rest = int((total > first * (1.0 + 1e-9)).sum())
        print("%s: steps with > 1 folded mini-step %d, rows beyond the first solve %d, kinds %s" % (R.case_id(c), multi, rest, sorted(shown)))
        assert multi >= 1, R.case_id(c)
        assert rest >= 1, R.case_id(c)
    assert SCENE_KINDS[name] <= shown, (name, shown)


def test_gpu_cases_run_every_kernel_twice_and_every_kind():
    runs = {}
    for c in R.CASES:
        k = (c[1], c[2], c[3]); runs[k] = runs.get(k, 0) + 1
    assert len(runs) == 8 and min(runs.values()) >= 2, runs
    assert set().union(*SCENE_KINDS.values()) == {"sphere-plane", "box-plane", "sphere pair", "box-sphere pair"}
    assert {c[5] for c in R.CASES} == {A.MH_ARTIC_CRB, A.MH_ARTIC_FSAB} and {c[4] for c in R.CASES} == {100.0, 0.5}


# ---- 6. host-side helpers and build checks ----
def test_report_slots_and_refusals_without_a_gpu():
    lib = _lib.load()
    m = BS.mixed_all()[0]
    assert lib.mh_artic_report_slots(ctypes.byref(m)) == 7 and A.report_slots(m) == 7
    assert A.report_slots(BS.arm_static()[0]) == 3
    assert lib.mh_artic_report_slots(None) == _lib.MH_ERR_INVALID_ARG and b"null model" in lib.mh_last_error()
    bad = BS.mixed_all()[0]; bad.npairs = A.MH_ARTIC_MAX_PAIRS + 1
    assert lib.mh_artic_report_slots(ctypes.byref(bad)) == _lib.MH_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    assert lib.mh_artic_batch_create_report(None, 1, ctypes.byref(h)) == _lib.MH_ERR_INVALID_ARG
    assert lib.mh_artic_batch_create_report(ctypes.byref(m), 1, None) == _lib.MH_ERR_INVALID_ARG
    assert lib.mh_artic_batch_create_report(ctypes.byref(m), 0, ctypes.byref(h)) == _lib.MH_ERR_INVALID_ARG
    bare = A.chain_model(3)                                              # no geometry: no slot (refused before the device is looked for)
    assert lib.mh_artic_batch_create_report(ctypes.byref(bare), 1, ctypes.byref(h)) == _lib.MH_ERR_INVALID_ARG and b"no slot" in lib.mh_last_error()
    assert h.value is None
    assert lib.mh_artic_batch_step_report(None, None, 1e-3, 1, None, None) == _lib.MH_ERR_INVALID_ARG
    buf = np.zeros(8)
    assert lib.mh_artic_batch_step_report(None, None, 1e-3, 1, None, buf.ctypes.data) == _lib.MH_ERR_INVALID_ARG


def test_ctypes_prototypes():
    _vp, _i, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert _lib.SYMBOLS["mh_artic_report_slots"] == (_i, [_vp])
    assert _lib.SYMBOLS["mh_artic_batch_create_report"] == (_i, [_vp, _i, ctypes.POINTER(_vp)])
    assert _lib.SYMBOLS["mh_artic_batch_step_report"] == (_i, [_vp, _vp, _d, _i, _vp, _vp])
    lib = _lib.load()
    for n in ("mh_artic_report_slots", "mh_artic_batch_create_report", "mh_artic_batch_step_report"):
        assert getattr(lib, n).argtypes == _lib.SYMBOLS[n][1]


def test_debug_key_19_takes_0_and_1():
    lib = _lib.load()
    try:
        assert lib.mh_debug_set(19, 1) == _lib.MH_OK and lib.mh_debug_set(19, 0) == _lib.MH_OK
        assert lib.mh_debug_set(19, 2) == _lib.MH_ERR_INVALID_ARG and lib.mh_debug_set(19, -1) == _lib.MH_ERR_INVALID_ARG
    finally:
        assert lib.mh_debug_set(19, 0) == _lib.MH_OK


def test_header_states_the_report(tmp_path):
    src = tmp_path / "v.c"
    src.write_text('#include <stdio.h>\n#include "moby_hip_artic.h"\nint main(void) { printf("%d %d %d\\n", MH_ARTIC_REPORT, MH_REPORT_PAIR, MH_VERSION); return 0; }\n')
    exe = str(tmp_path / "v")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert subprocess.check_output([exe]).split() == [b"1", b"8", b"102"]


def test_link_impulses_on_a_hand_written_report():
    """+[2..4] on A's link, -[2..4] on B's; a static box is skipped; numpy and torch alike, any leading shape"""
    import torch
    m = BS.mixed_all()[0]          # spheres on links 6, 7 (7 masked); boxes on link 5 and static; pairs: spheres (0, 1), box-sphere (1, 0), (1, 1)
    rng = np.random.default_rng(0)
    rep = rng.integers(-8, 9, size=(2, 3, 7, 8)).astype(np.float64)
    want = np.zeros((2, 3, 8, 3))
    want[..., 6, :] += rep[..., 0, 2:5]                                  # sphere 0 on the plane
    want[..., 7, :] += rep[..., 1, 2:5]                                  # sphere 1's slot (zero in a real report)
    want[..., 5, :] += rep[..., 2, 2:5]                                  # box 0 on the plane
    want[..., 6, :] += rep[..., 4, 2:5]; want[..., 7, :] -= rep[..., 4, 2:5]      # sphere pair (0, 1): A = sphere 0's link
    want[..., 6, :] -= rep[..., 5, 2:5]                                  # static box 1 against sphere 0: only B's share
    want[..., 7, :] -= rep[..., 6, 2:5]                                  # static box 1 against sphere 1
    np.testing.assert_array_equal(A.link_impulses(rep, m), want)
    got_t = A.link_impulses(torch.from_numpy(rep), m)
    assert isinstance(got_t, torch.Tensor) and np.array_equal(got_t.numpy(), want)
    np.testing.assert_array_equal(A.link_impulses(rep[1, 2], m), want[1, 2])
    with pytest.raises(AssertionError):
        A.link_impulses(rep[..., :6, :], m)


def test_cpp_example_compiles_and_fails_loudly_without_a_gpu(tmp_path):
    """MobyHipArticulatedBody.h's with_report / step_report: the example builds; without a device it reports the error (no fallback), with one it
    runs to its end"""
    import torch
    cpp = os.path.join(ROOT, "moby_amd", "cpp")
    exe = str(tmp_path / "example_artic_report")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-Wall", os.path.join(cpp, "example_artic_report.cpp"), "-L" + os.path.join(ROOT, "moby_amd"), "-lmoby_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "moby_amd"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, timeout=120)
    if torch.cuda.is_available():
        assert p.returncode == 0 and b"first impact in step" in p.stdout, p.stdout
    else:
        assert p.returncode == 1 and b"no HIP device" in p.stdout, p.stdout
