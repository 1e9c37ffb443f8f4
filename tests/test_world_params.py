"""Per-world parameters of the many-worlds stepper (include/moby_hip.h, "Per-world parameters") without a GPU: the layout of the record, the record that
reproduces the scene, the refusals (they run before the device is looked for) and the per-world reference loop of tests/world_params_ref.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import scene as S
from tests import world_params_ref as P
from tests import world_statics_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MH_ERR_INVALID_ARG = -1


def _create(sc, stt, params, B):
    h = ctypes.c_void_p()
    rc = _lib.load().mh_world_batch_create_params(ctypes.addressof(sc), None if stt is None else ctypes.addressof(stt),
                                                  None if params is None else params.ctypes.data, B, ctypes.byref(h))
    msg = _lib.load().mh_last_error().decode()
    if h:
        _lib.load().mh_world_batch_destroy(h)
    return rc, msg


def test_ctypes_mirror_has_the_c_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "moby_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d\\n", sizeof(mh_world_params), offsetof(mh_world_params, plane_R), offsetof(mh_world_params, cp_epsilon),\n'
                   '  offsetof(mh_world_params, st_dim), MH_WORLD_PARAMS); return 0; }\n')
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    T = S.mh_world_params
    assert got == [ctypes.sizeof(T), T.plane_R.offset, T.cp_epsilon.offset, T.st_dim.offset, 1]
    assert got[0] == 2680 == 8 * S.PARAMS_DOUBLES == S.PARAMS_DTYPE.itemsize
    D = S.PARAMS_DTYPE.fields
    assert [D[f][1] for f in ("plane_R", "cp_epsilon", "st_dim")] == got[1:4]
    assert all(D[f][0].base == np.float64 for f in D)                     # doubles only: nothing in the record can become an index


@pytest.mark.parametrize("with_statics", [True, False])
def test_record_of_the_scene_byte_for_byte(with_statics):
    """mh_world_params_from_scene and scene.make_params agree byte for byte, and writing the record back gives the scene"""
    sc, stt = W.mixed_scene_and_statics()
    if not with_statics:
        stt = None
    rec = S.mh_world_params()
    _lib.load().mh_world_params_from_scene(ctypes.addressof(sc), None if stt is None else ctypes.addressof(stt), ctypes.addressof(rec))
    p = S.make_params(sc, stt, 3)
    for w in range(3):
        assert p[w].tobytes() == bytes(rec)
    assert (p["st_dim"][0, 1] > 0).all() == with_statics and p["cp_mu_coulomb"][0, S.pair_index(0, 1, 6)] == 0.35
    s2, t2 = P.world_scene(sc, stt, p, 2)
    assert bytes(s2) == bytes(sc) and (stt is None or bytes(t2) == bytes(stt))


def _bad(field, w, idx, value):
    sc, stt = W.mixed_scene_and_statics()
    p = S.make_params(sc, stt, 4)
    p[field][(w,) + idx] = value
    return _create(sc, stt, p, 4)


@pytest.mark.parametrize("field,idx,value,word", [
    ("mass", (1,), 0.0, "mass[1]"), ("mass", (2,), float("nan"), "mass[2]"), ("inertia", (0, 2), -1.0, "inertia[0]"),
    ("geom_dim", (0, 0), 0.0, "radius"), ("geom_dim", (1, 2), -0.5, "box edge"), ("geom_dim", (1, 1), float("nan"), "box edge"),
    ("gravity", (1,), float("inf"), "gravity"), ("plane_R", (4,), float("nan"), "plane_R"), ("plane_o", (0,), float("inf"), "plane_o"),
    ("cp_epsilon", (14,), float("nan"), "cp_epsilon[14]"), ("cp_mu_coulomb", (3,), float("inf"), "cp_mu_coulomb[3]"),
    ("cp_mu_viscous", (0,), float("nan"), "cp_mu_viscous[0]"), ("cp_compliance", (7,), float("nan"), "cp_compliance[7]"),
    ("st_R", (0, 8), float("nan"), "st_R[0]"), ("st_o", (1, 2), float("inf"), "st_o[1]"), ("st_dim", (1, 0), 0.0, "st_dim[1]"),
    ("st_dim", (1, 1), float("inf"), "st_dim[1]")])
@pytest.mark.parametrize("w", [0, 3])
def test_refusals_name_the_world_and_the_field(field, idx, value, word, w):
    rc, msg = _bad(field, w, idx, value)
    assert rc == MH_ERR_INVALID_ARG and ("world %d:" % w) in msg and word in msg, msg


def test_values_the_topology_does_not_use_are_not_looked_at():
    """bodies above nb, pair slots above C(ntot, 2), statics above n, a plane's st_dim, a spokes body's geom_dim and the ground frame of a scene without
    ground may hold anything; the records pass (without a device the entry then fails with MH_ERR_NO_DEVICE, with one it creates the batch)"""
    sc, stt = W.mixed_scene_and_statics()
    p = S.make_params(sc, stt, 2)
    p["mass"][1, 3:] = -1.0; p["geom_dim"][1, 3:] = np.nan; p["cp_epsilon"][1, 15:] = np.nan; p["st_R"][1, 2:] = np.nan; p["st_dim"][1, 0] = -1.0
    assert _create(sc, stt, p, 2)[0] != MH_ERR_INVALID_ARG
    wheel = S.rimless_wheel_scene()
    p = S.make_params(wheel, None, 2)
    p["geom_dim"][1, 0] = np.nan; p["st_R"][:] = np.nan
    rc, msg = _create(wheel, None, p, 2)
    assert rc != MH_ERR_INVALID_ARG, msg
    sc, stt, _ = W.corner_batch(2)
    p = S.make_params(sc, stt, 2)
    p["plane_R"][1] = np.nan
    assert sc.has_ground == 0 and _create(sc, stt, p, 2)[0] != MH_ERR_INVALID_ARG


def test_topology_refusals_stay():
    """box-box, spokes beside statics and the sizes are refused as mh_world_batch_create_statics refuses them, before any record is looked at"""
    lib = _lib.load()
    cases = []
    sc = W.scene([("box", (1.0, 1.0, 1.0), 1.0)], 1)
    cases.append((sc, S.make_statics([dict(box=(1.0, 1.0, 1.0), o=(0.0, -2.0, 0.0))]), "box-box"))
    cases.append((S.rimless_wheel_scene(), S.make_statics([dict(plane=True, R=W.R_UP)]), "spokes"))
    bad = S.sphere_stack_scene(); bad.nb = 0
    cases.append((bad, None, "nb = 0"))
    for sc, stt, word in cases:
        p = S.make_params(sc, stt, 2)
        p["mass"][:] = -1.0                                              # (a bad record as well: the topology's message wins)
        rc, msg = _create(sc, stt, p, 2)
        h = ctypes.c_void_p()
        rc0 = lib.mh_world_batch_create_statics(ctypes.addressof(sc), None if stt is None else ctypes.addressof(stt), 2, ctypes.byref(h))
        assert (rc, msg) == (rc0, lib.mh_last_error().decode()) and rc == MH_ERR_INVALID_ARG and word in msg
    sc, stt = W.mixed_scene_and_statics()
    assert _create(sc, stt, S.make_params(sc, stt, 1), 0)[0] == MH_ERR_INVALID_ARG


def test_no_params_is_the_statics_entry():
    """params == NULL is exactly mh_world_batch_create_statics: same return code and message, with a device or without one"""
    lib = _lib.load()
    sc, stt = W.mixed_scene_and_statics()
    for s, t in ((sc, stt), (S.sphere_stack_scene(), None)):
        h = ctypes.c_void_p()
        rc0 = lib.mh_world_batch_create_statics(ctypes.addressof(s), None if t is None else ctypes.addressof(t), 2, ctypes.byref(h))
        m0 = lib.mh_last_error().decode() if rc0 else ""
        if h:
            lib.mh_world_batch_destroy(h)
        rc, msg = _create(s, t, None, 2)
        assert rc == rc0 and (rc == 0 or msg == m0)
        if lib.mh_device_count() <= 0:
            assert rc == _lib.MH_ERR_NO_DEVICE and "no HIP device" in msg


def test_set_params_refuses_a_null_batch():
    lib = _lib.load()
    p = S.make_params(S.sphere_stack_scene(), None, 1)
    assert lib.mh_world_batch_set_params(None, p.ctypes.data, 0, 1) == MH_ERR_INVALID_ARG
    assert lib.mh_world_batch_set_params_dev(None, None, p.ctypes.data, 0, 1) == MH_ERR_INVALID_ARG
    assert lib.mh_debug_set(17, 2) == MH_ERR_INVALID_ARG and lib.mh_debug_set(17, 0) == 0


def test_python_side_checks_the_records():
    from moby_amd.world import WorldBatch
    sc, stt, st = W.mixed_batch(4)
    with pytest.raises(ValueError):
        WorldBatch(sc, st, statics=stt, params=S.make_params(sc, stt, 3))            # three records for four worlds
    with pytest.raises(ValueError):
        WorldBatch(sc, st, statics=stt, params=np.zeros((4, S.PARAMS_DOUBLES)))      # not the record type


def test_reference_per_world_with_the_scene_in_every_record_is_the_shared_run():
    """the loop of tests/world_params_ref.py over records equal to the scene equals the reference run once with the shared scene (the `mixed` case)"""
    c, st_r, aux_r, traj_r, _ = W.reference_run("mixed")
    p = S.make_params(c["scene"], c["statics"], c["state"].shape[0])
    st, aux, traj = P.run_ref_params(c["scene"], c["statics"], p, c["state"], c["dt"], c["nsteps"], want_traj=True)
    np.testing.assert_array_equal(st, st_r)
    np.testing.assert_array_equal(traj, traj_r)
    assert aux.tobytes() == aux_r.tobytes()


def test_varied_batch_conditions_hold_on_the_reference():
    """no fatal bit, LCPs solved in every world, mini-steps bounded, worlds 1-7 all differ from the shared-scene run (asserted by varied_run); the
    varied values are where the recipe puts them"""
    c, st, aux, _ = P.varied_run()
    p, sc = c["params"], c["scene"]
    print("varied batch: mini-steps per world", aux["mini_steps"], "status", aux["status"], "LCPs", aux["lcp_solves"])
    assert p[0].tobytes() == S.make_params(sc, c["statics"], 1)[0].tobytes()
    for w in range(1, 8):
        assert (p["geom_dim"][w, :3] <= p["geom_dim"][0, :3]).all() and (p["mass"][w, :3] != p["mass"][0, :3]).all()
        assert (p["cp_mu_coulomb"][w, :15] != p["cp_mu_coulomb"][0, :15]).all() and (p["cp_epsilon"][w, :15] <= 1.0).all()
        assert not np.array_equal(p["st_o"][w, :2], p["st_o"][0, :2]) and p["st_dim"][w, 1, 1] == p["st_dim"][0, 1, 1]
    _, st_f, aux_f, _ = P.varied_run(forced=True)
    assert not np.array_equal(st_f, st)


@pytest.mark.parametrize("name", ["plane8", "ring"])
def test_last_slots_carry_values_of_their_own(name):
    """body lane 7 and pair slot 35 (plane8), static slot 7 (ring) differ from the scene's in some world, and the reference runs clean on them"""
    c = P.slots_case(name)
    p = c["params"]
    if name == "plane8":
        assert c["scene"].nb == 8 and S.pair_index(7, 8, 9) == 35
        assert (p["geom_dim"][1:, 7, 0] != p["geom_dim"][0, 7, 0]).any() and (p["mass"][1:, 7] != p["mass"][0, 7]).any()
        assert (p["cp_mu_coulomb"][1:, 35] != p["cp_mu_coulomb"][0, 35]).any() and (p["st_o"][1:, 0, 1] != p["st_o"][0, 0, 1]).any()
    else:
        assert c["scene"].nb == 1 and c["statics"].n == 8
        assert (p["st_dim"][1:, 7] != p["st_dim"][0, 7]).any() and (p["st_o"][1:, 7] != p["st_o"][0, 7]).any()
    st, aux, _ = P.run_ref_params(c["scene"], c["statics"], p, c["state"], c["dt"], c["nsteps"])
    P.check_conditions(aux, c["nsteps"])
    st_s = W.reference_run(name)[1]
    np.testing.assert_array_equal(st[0], st_s[0])
    assert sum(not np.array_equal(st[w], st_s[w]) for w in range(1, st.shape[0])) >= st.shape[0] // 2
