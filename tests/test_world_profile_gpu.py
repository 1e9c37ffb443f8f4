"""The stamped code objects of the many-worlds kernel (mh_world_{small,wheel,large}_prof.hip: separate compilations with the phase profiler's stamps
compiled in), which mh_world_batch_profile launches for an unforced batch: a profile launch must step the worlds exactly as the production object does --
state and complete aux records byte for byte -- and hand back a coherent cycle vector.  The builds without a stamped object (box-sphere, statics) go
through the production kernel: the reference's results, every cycle count exactly zero."""
import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import scene as S
from moby_amd.synth import world_uniforms
from moby_amd.world import WorldBatchDevice
from tests.world_ref import assert_aux_equal

pytestmark = pytest.mark.gpu

PH_LCP = 7            # mh_world_wave.inc: PH_BROAD_CA, PH_INTEGRATE, PH_FWDDYN, PH_CONTACTS, PH_ISLANDS, PH_PDATA, PH_MBUILD, PH_LCP, PH_APPLY, PH_STAB


def _stack():
    return S.sphere_stack_scene(), S.sphere_stack_state(8), 0.01, 40


def _wheel():
    rates = [0.24 if w == 0 else 0.2 + 0.4 * world_uniforms(w, 1)[0] for w in range(4)]
    return S.rimless_wheel_scene(), S.rimless_wheel_state(rates), 1e-3, 300


def _mixed():
    from tests.test_world_gpu import _mixed_scene
    sts = []
    for w in range(4):                                       # the states of test_mixed_spheres_and_box_bit_exact
        u = world_uniforms(w, 12)
        st = np.zeros((3, 13)); st[:, 6] = 1.0
        st[0, :3] = (0.0, 0.5 + 0.05 * u[0], 0.0); st[1, :3] = (0.1 * u[1], 1.45 + 0.2 * u[2], 0.05 * u[3])
        st[2, :3] = (2.0, 0.45 + 0.3 * u[4], 0.0)
        q = np.array([u[5] - 0.5, u[6] - 0.5, u[7] - 0.5, 1.0]); st[2, 3:7] = q / np.linalg.norm(q)
        st[0, 7:10] = (0.3 * u[8], 0.0, 0.0); st[2, 10:13] = (u[9], 2 * u[10], u[11])
        sts.append(st.ravel())
    return _mixed_scene(), np.array(sts), 1e-3, 150       # (150 steps: every world has solved LCPs; the box's conservative advancement gets slow after that)


BUILDS = {"small": _stack, "wheel": _wheel, "large": _mixed}


def profile(dev, dt, nsteps):
    """one profile launch -> the cycle vector (PHC + 4 entries) and PHC"""
    lib = _lib.load()
    phc = lib.mh_world_profile_phase_count()
    cyc = np.full(phc + 4, -1.0)
    _lib.check(lib.mh_world_batch_profile(dev.handle, float(dt), int(nsteps), cyc.ctypes.data, phc + 4))
    return cyc, phc


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_profile_object_steps_the_worlds_as_the_production_object(build):
    sc, st0, dt, nsteps = BUILDS[build]()
    half = build == "small"                                   # 20 steps stamped, then 20 by the production object == 40 by the production object
    devs = [WorldBatchDevice(sc, st0) for _ in range(3 if half else 2)]
    try:
        devs[0].step(dt, nsteps)
        st, aux = devs[0].download()
        cyc, phc = profile(devs[1], dt, nsteps)
        st_p, aux_p = devs[1].download()
        if half:
            cyc_h, _ = profile(devs[2], dt, nsteps // 2)
            devs[2].step(dt, nsteps - nsteps // 2)
            st_h, aux_h = devs[2].download()
    finally:
        for d in devs:
            d.close()
    print(build, "cycles", cyc)
    assert (aux["steps"] == nsteps).all() and (aux["status"] & ~S.MH_WORLD_IMPACT_TOL == 0).all() and (aux["lcp_solves"] > 0).all()
    np.testing.assert_array_equal(st_p, st)
    assert_aux_equal(aux_p, aux)
    assert aux_p.tobytes() == aux.tobytes()
    if half:
        np.testing.assert_array_equal(st_h, st)
        assert_aux_equal(aux_h, aux)
        assert aux_h.tobytes() == aux.tobytes()
        assert np.isfinite(cyc_h).all() and (cyc_h >= 0).all() and 0 < cyc_h[:10].sum()
    # the cycle vector
    assert phc >= 10 and np.isfinite(cyc).all() and (cyc >= 0).all()
    total = cyc[:10].sum()
    assert total > 0
    if (aux["lcp_solves"] > 0).any():
        assert cyc[PH_LCP] > 0
    slowest, fastest, mean, p99 = cyc[phc], cyc[phc + 1], cyc[phc + 2], cyc[phc + 3]
    assert slowest >= p99 >= fastest > 0
    assert fastest <= mean <= slowest
    assert abs(mean - total) <= 1e-9 * total                 # both are means over the worlds of the same integers


def _no_stamped_object(case, st_r, aux_r, statics=None):
    dev = WorldBatchDevice(case["scene"], case["state"], statics=statics)
    try:
        cyc, phc = profile(dev, case["dt"], case["nsteps"])
        st, aux = dev.download()
    finally:
        dev.close()
    np.testing.assert_array_equal(st, st_r)
    assert_aux_equal(aux, aux_r)
    assert (cyc == 0.0).all(), cyc


def test_box_sphere_build_has_no_stamped_object():
    """the "face" batch (box-sphere row of the build table): the production kernel steps the worlds, every cycle count is exactly zero"""
    from tests.world_boxsphere_ref import reference_run
    case, st_r, aux_r, _, _ = reference_run("face")
    _no_stamped_object(case, st_r, aux_r)


def test_statics_build_has_no_stamped_object():
    """the "corner" batch (statics row of the build table): likewise"""
    from tests.world_statics_ref import reference_run
    case, st_r, aux_r, _, _ = reference_run("corner")
    _no_stamped_object(case, st_r, aux_r, statics=case["statics"])
