"""Static planes and boxes among the free bodies of the many-worlds stepper (include/moby_hip.h, "Static bodies") without a GPU: the reference the
kernels are held to (tests/native/world_ref.cpp, a restatement of what several statics change in oracle::World) pinned to the oracle -- the
scene's ground, and the same plane handed over as a static, both ARE oracle_world_step_batch --, to the box geometry written out by hand on dyadic
inputs and to the articulated reference's static box; a mirror property of two opposed walls; the refusals of the new entry; the ctypes mirror; the
exported symbols; the scene reader.  All comparisons are bit for bit.  The reference's ctypes face lives in tests/world_ref.py, the scenes shared with the
GPU tests in tests/world_statics_ref.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import io as mio
from moby_amd import scene as S
from tests.world_ref import assert_aux_equal, run_ref
from tests import world_statics_ref as W
# the hand-written values of the box-sphere geometry (box frame, half lengths (1, 0.5, 0.75), dyadic throughout): the same tables, other box poses
from tests.test_world_boxsphere import CONTACTS, DIMS, DISTS

ROOT = W.ROOT
ELLIPSE_XML = os.path.join(os.environ.get("MOBY_REFERENCE", "/root/reference"), "example", "ellipse", "ellipse2D.xml")   # the reference tree, where there is one


@pytest.fixture(scope="session")
def ref():
    return W.reference()


def ground_as_static(sc):
    """the same scene with has_ground = 0 and its plane as static 0: the pair slots do not move (the plane is body nb either way)"""
    s2 = S.mh_scene.from_buffer_copy(bytes(sc))
    s2.has_ground = 0
    return s2, S.make_statics([dict(plane=True, R=np.array(sc.plane_R[:]).reshape(3, 3), o=tuple(sc.plane_o[:]))])


# ---- 1. pinned to the oracle -------------------------------------------------------------------------------------------------------------------
def _tumbling_box():
    sc = S.box_scene(dims=(1.0, 0.6, 0.8), epsilon=0.3, mu_coulomb=0.4, nk=4, ground_rpy=(0.1, 0.0, -0.05))
    st = np.concatenate([S.box_state(pos=(0.0, 0.8 + 0.01 * w, 0.0), quat=tuple(np.array([0.3, 0.1, -0.2, 0.9]) / np.linalg.norm([0.3, 0.1, -0.2, 0.9])),
                                     v=(0.3, -1.0, 0.1), w=(1.0, -2.0, 0.5 + 0.1 * w)).reshape(1, -1) for w in range(4)])
    return sc, st, 0.005


def _noslip_ball():
    sc = S.make_scene([0.5], [1.0], (0.0, -9.81, 0.0), ground_rpy=(0.0, 0.0, 0.0), params={(0, 1): dict(epsilon=0.0, mu_coulomb=100.0)})
    sc.lcp_n_max = 64
    st = np.zeros((4, 13)); st[:, 6] = 1.0
    for w in range(4):
        st[w, 1] = 0.5 + 1e-3 * w; st[w, 7] = 1.0 + 0.1 * w; st[w, 8] = -0.5
    return sc, st, 0.005


PIN = {
    "sphere_stack": lambda: (S.sphere_stack_scene(), S.sphere_stack_state(4), 0.01),          # stabiliser on (10 iterations)
    "tumbling_box": _tumbling_box,
    "noslip_ball": _noslip_ball,
}


@pytest.fixture(scope="session")
def pinned(oracle):
    out = {}
    for name, make in PIN.items():
        sc, st0, dt = make()
        st_o, aux_o = st0.copy(), S.new_aux(st0.shape[0])
        oracle.world_step_batch(sc, st_o, aux_o, dt, 40)
        st_o.setflags(write=False)
        out[name] = (sc, st0, dt, st_o, aux_o)
    return out


@pytest.mark.parametrize("as_static", [False, True])
@pytest.mark.parametrize("name", sorted(PIN))
def test_reference_is_the_oracle(ref, pinned, name, as_static):
    """4 worlds x 40 steps: the scene's own ground, and the same plane as a static of a ground-less scene, equal oracle_world_step_batch bit for bit"""
    sc, st0, dt, st_o, aux_o = pinned[name]
    assert (aux_o["lcp_solves"] > 0).all()
    if name == "sphere_stack":
        assert aux_o["stab_iters"].sum() > 0
    sc2, stt = ground_as_static(sc) if as_static else (sc, None)
    st_r, aux_r = st0.copy(), S.new_aux(st0.shape[0])
    ref.step(sc2, st_r, aux_r, dt, 40, statics=stt)
    np.testing.assert_array_equal(st_r, st_o)
    assert_aux_equal(aux_r, aux_o)
    assert aux_r.tobytes() == aux_o.tobytes()


@pytest.mark.parametrize("name", ["face", "full"])
def test_no_statics_is_an_empty_record(name):
    """statics = None steps exactly as an empty mh_world_statics (n = 0) on box-sphere batches: state, trajectory, census and whole aux records"""
    from tests.world_boxsphere_ref import gpu_cases
    c = gpu_cases()[name]
    empty = S.mh_world_statics()
    assert empty.n == 0
    st_n, aux_n, r_n = run_ref(c["scene"], c["state"], c["dt"], c["nsteps"], want_traj=True, want_census=True)
    st_e, aux_e, r_e = run_ref(c["scene"], c["state"], c["dt"], c["nsteps"], statics=empty, want_traj=True, want_census=True)
    assert (aux_n["lcp_solves"] > 0).all() and r_n.census[:, :, :W.PENETRATING + 1].sum() > 0
    np.testing.assert_array_equal(st_e, st_n)
    np.testing.assert_array_equal(r_e.traj, r_n.traj)
    np.testing.assert_array_equal(r_e.census, r_n.census)
    assert aux_e.tobytes() == aux_n.tobytes()


# ---- 2. static-box geometry ----------------------------------------------------------------------------------------------------------------------
# box poses whose rotation has entries in {0, +-1} and whose centre is dyadic: every product and sum of the change of frame is exact
POSES = [(np.zeros(3), np.eye(3)),
         (np.array([0.5, -0.25, 2.0]), np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])),     # a quarter turn about z
         (np.array([-1.5, 0.75, 0.125]), np.array([[0.0, 0.0, 1.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0]]))]   # a half turn about (1, 0, 1) / sqrt 2


def to_world(P, v, point=True):
    return (P[0] if point else 0.0) + P[1] @ np.array(v)


@pytest.mark.parametrize("pose", range(len(POSES)))
@pytest.mark.parametrize("name", sorted(CONTACTS))
def test_static_box_contact_equals_the_hand_written_values(ref, name, pose):
    """face, edge and vertex regions, touching, separated and penetrating"""
    P = POSES[pose]
    c, radius, TOL, (has, dist, point, normal, region) = CONTACTS[name]
    got = ref.box_contact(P[0], P[1], DIMS, to_world(P, c), radius, TOL)
    assert got["has"] == has and got["region"] == region
    assert got["dist"] == dist
    if has:
        np.testing.assert_array_equal(got["point"], to_world(P, point))
        np.testing.assert_array_equal(got["normal"], to_world(P, normal, point=False))       # (NaN == NaN for assert_array_equal)


@pytest.mark.parametrize("pose", range(len(POSES)))
@pytest.mark.parametrize("name", sorted(DISTS))
def test_static_box_signed_distance_equals_the_hand_written_values(ref, name, pose):
    P = POSES[pose]
    c, radius, (dist, pbox, psph) = DISTS[name]
    d, pa, pb = ref.box_dist(P[0], P[1], DIMS, to_world(P, c), radius)
    assert d == dist
    np.testing.assert_array_equal(pa, to_world(P, pbox))
    np.testing.assert_array_equal(pb, to_world(P, psph))


def test_static_box_through_the_pair_probe(ref):
    """the stepper's view of a (sphere, static box) pair: the box is contact_geom1 under its static index, the first signed-distance point is the
    sphere's, and the pair of two statics is never kept by the broad phase"""
    P = POSES[1]
    sc = W.scene([("sphere", 0.5, 1.0)], 2)
    stt = S.make_statics([dict(box=DIMS, R=P[1], o=tuple(P[0])), dict(plane=True, R=W.R_UP, o=(0.0, -10.0, 0.0))])
    c = CONTACTS["edge_separated"][0]
    st = np.zeros(13); st[:3] = to_world(P, c); st[6] = 1.0
    got = ref.pair(sc, st, 0, 0.25, statics=stt)
    want = ref.box_contact(P[0], P[1], DIMS, st[:3], 0.5, 0.25)
    assert (got["a"], got["b"], got["ncontacts"], got["g1"], got["g2"], got["kept"]) == (0, 1, 1, 1, 0, 1)
    assert got["cdist"] == want["dist"]
    np.testing.assert_array_equal(got["point"], want["point"]); np.testing.assert_array_equal(got["normal"], want["normal"])
    d, pbox, psph = ref.box_dist(P[0], P[1], DIMS, st[:3], 0.5)
    assert got["dist"] == d
    np.testing.assert_array_equal(got["pa"], psph); np.testing.assert_array_equal(got["pb"], pbox)
    assert ref.pair(sc, st, 2, 0.25, statics=stt)["kept"] == 0                     # (static box, static plane)
    far = st.copy(); far[:3] = (100.0, 100.0, 100.0)
    assert ref.pair(sc, far, 0, 0.25, statics=stt)["kept"] == 0 and ref.pair(sc, far, 1, 0.25, statics=stt)["kept"] == 1   # a box's bound is finite, a plane's is not


def test_static_box_equals_the_articulated_reference(ref):
    """tests/native/artic_boxsphere_ref.cpp with a static axis-aligned box at the origin and the sphere on three sliders with zero offsets (q = its
    centre): the same contact and the same signed distance, bit for bit, on every case of the tables"""
    from moby_amd import artic as A
    from tests import artic_boxsphere_ref as BS
    from tests import artic_pair_ref as APR
    aref = BS.build_boxsphere_ref()

    def model(radius):
        links = [dict(parent=k - 1, type=A.MH_JOINT_PRISMATIC, R0=np.eye(3), x0=(0.0, 0.0, 0.0), axis=np.eye(3)[k], com=(0.0, 0.0, 0.0),
                      inertia=np.eye(3) * (0.4 if k == 2 else 0.0), mass=1.0 if k == 2 else 0.0) for k in range(3)]
        m = A.model_from_links(links, gravity=(0.0, 0.0, 0.0))
        A.add_spheres(m, [(2, (0.0, 0.0, 0.0), radius)], plane_normal=APR.UP, plane_point=(0.0, -50.0, 0.0))
        A.add_boxes(m, [(-1, (0.0, 0.0, 0.0), np.eye(3), DIMS)], plane_normal=APR.UP, plane_point=(0.0, -50.0, 0.0))
        A.add_box_sphere_pairs(m, [(0, 0)], no_plane=(0,))
        return m

    for name, (c, radius, TOL, _) in sorted(CONTACTS.items()):
        got = ref.box_contact(np.zeros(3), np.eye(3), DIMS, c, radius, TOL)
        has, pt, nn, dist, region = aref.contact(model(radius), np.array(c), 0, TOL)
        assert (int(has), region) == (got["has"], got["region"]), name
        assert dist == got["dist"], name
        if has:
            np.testing.assert_array_equal(pt, got["point"], err_msg=name)
            np.testing.assert_array_equal(nn, got["normal"], err_msg=name)
    for name, (c, radius, _) in sorted(DISTS.items()):
        assert aref.regions(model(radius), np.array(c)[None, :])[1][0, 0] == ref.box_dist(np.zeros(3), np.eye(3), DIMS, c, radius)[0], name


# ---- 3. the mirror property ----------------------------------------------------------------------------------------------------------------------
def test_two_opposed_walls_mirror(ref):
    """a frictionless ball, epsilon = 1, no gravity, between the walls x = -1 (normal +x) and x = +1 (normal -x), rotations with entries in {0, +-1}:
    started with (x, vx) and with (-x, -vx) the two trajectories are mirror images in x bit for bit, and |v| is what it was after every bounce"""
    sc = W.scene([("sphere", 0.25, 1.0)], 2, gravity=(0.0, 0.0, 0.0), epsilon=1.0, mu_coulomb=0.0, cstab=0)
    stt = S.make_statics([dict(plane=True, R=W.R_POS_X, o=(-1.0, 0.0, 0.0)), dict(plane=True, R=W.R_NEG_X, o=(1.0, 0.0, 0.0))])
    st = W.sphere_state(2, 1)
    W.set_body(st, 0, 0, (0.125, 0.5, -0.25), v=(3.0, 0.0, 0.0))
    W.set_body(st, 1, 0, (-0.125, 0.5, -0.25), v=(-3.0, 0.0, 0.0))
    s, aux, (traj, *_) = run_ref(sc, st.reshape(2, -1), 0.01, 120, statics=stt, want_traj=True)
    assert (aux["status"] & W.FATAL == 0).all() and (aux["lcp_solves"] >= 2).all()      # 3.6 m at 0.75 m between the turning points: several bounces
    mirror = traj[1].copy(); mirror[..., 0] = -mirror[..., 0]
    np.testing.assert_array_equal(traj[0], mirror)
    assert traj[0][:, 0, 0].max() <= 0.75 + 1e-6 and traj[0][:, 0, 0].min() >= -0.75 - 1e-6
    assert abs(s.reshape(2, 13)[0, 7]) == 3.0 and s.reshape(2, 13)[0, 7] == -s.reshape(2, 13)[1, 7]
    np.testing.assert_array_equal(s.reshape(2, 13)[:, 8:13], 0.0)


# ---- 3b. the mixed scene as an input: a ground AND statics, parameters per pair slot ------------------------------------------------------------
def test_mixed_scene_is_built_as_stated():
    sc, stt, st = (W.gpu_cases()["mixed"][k] for k in ("scene", "statics", "state"))
    assert (sc.nb, sc.has_ground, stt.n, st.shape) == (3, 1, 2, (8, 39)) and list(stt.type[:2]) == [S.MH_STATIC_PLANE, S.MH_STATIC_BOX]
    assert [sc.geom_type[b] for b in range(3)] == [S.MH_GEOM_SPHERE, S.MH_GEOM_BOX, S.MH_GEOM_SPHERE]
    # every frame is a general rotation (at most one entry in {0, +-1}); every origin is off the world's
    for R in (np.array(sc.plane_R[:]), np.array(stt.R[0][:]), np.array(stt.R[1][:])):
        assert (~np.isin(np.abs(R), (0.0, 1.0))).sum() >= 8 and np.allclose(R.reshape(3, 3) @ R.reshape(3, 3).T, np.eye(3), atol=1e-15)
    assert any(sc.plane_o[:]) and all(stt.o[0][:]) and any(stt.o[1][:])
    # 15 slots over ntot = 6; the box body / static box pair and sphere 0 / wall are disabled, nothing else; the parameters of no two slots agree
    en = {(i, j): sc.pair_enabled[S.pair_index(i, j, 6)] for i in range(6) for j in range(i + 1, 6)}
    assert len(en) == 15 and sorted(k for k, v in en.items() if not v) == sorted(W.MIXED_DISABLED) == [(0, W.MIXED_WALL), (1, W.MIXED_SBOX)]
    triples = [(sc.cp_epsilon[p], sc.cp_mu_coulomb[p], sc.cp_nk[p]) for p in range(15)]
    assert len(set(triples)) == 15 and {t[2] for t in triples} == {4, 8} and sum(sc.cp_mu_viscous[p] > 0 for p in range(15)) >= 4
    assert len({t[0] for t in triples}) == 15 and len({t[1] for t in triples}) == 15


def test_mixed_scene_conditions_hold_on_the_reference(ref):
    """reference_run asserts them (check_mixed_conditions): no fatal bit, LCPs solved and the stabiliser run, the mini-step cap, kept contacts of the five
    pair kinds in two worlds each under parameters of their own, the ball through the wall it does not collide with"""
    c, st, aux, _, _ = W.reference_run("mixed")
    assert (aux["mini_steps"] <= 50 * c["nsteps"]).all() and (aux["status"] & W.FATAL == 0).all()
    c, st_f, aux_f, _, _ = W.reference_run("mixed_forces")
    assert not np.array_equal(st_f, st)


@pytest.mark.parametrize("name", ["mixed", "mixed_forces"])
def test_mixed_scene_equals_its_ground_as_static_twin_on_the_reference(ref, name):
    """has_ground = 0, the ground static 0, the statics one slot up: bit-equal state, records and trajectory"""
    c, st, aux, traj, _ = W.reference_run(name)
    sc2, stt2 = W.ground_to_static(c["scene"], c["statics"])
    assert (sc2.has_ground, stt2.n) == (0, 3) and bytes(sc2)[8:] == bytes(c["scene"])[8:]
    st2, aux2, (traj2, *_) = run_ref(sc2, c["state"], c["dt"], c["nsteps"], statics=stt2, want_traj=True, forces=c.get("forces"), wrench=c.get("wrench"))
    np.testing.assert_array_equal(traj2, traj)
    np.testing.assert_array_equal(st2, st)
    assert aux2.tobytes() == aux.tobytes()


# ---- 4. argument validation (no GPU: every refusal comes before the device is asked for) ------------------------------------------------------
def _create(sc, stt, B=2):
    h = ctypes.c_void_p()
    rc = _lib.load().mh_world_batch_create_statics(ctypes.addressof(sc), None if stt is None else ctypes.addressof(stt), B, ctypes.byref(h))
    msg = _lib.load().mh_last_error().decode()
    if h:
        _lib.load().mh_world_batch_destroy(h)
    return rc, msg


MH_ERR_INVALID_ARG = -1


def test_refusals():
    lib = _lib.load()
    plane = dict(plane=True, R=W.R_UP)
    # box body against a static box, enabled: box-box
    sc = W.scene([("box", (1.0, 1.0, 1.0), 1.0)], 1)
    stt = S.make_statics([dict(box=(1.0, 1.0, 1.0), o=(0.0, -2.0, 0.0))])
    rc, msg = _create(sc, stt)
    assert rc == MH_ERR_INVALID_ARG and "box-box" in msg and "static 0" in msg
    # a spokes body beside statics
    sc = S.rimless_wheel_scene()
    rc, msg = _create(sc, S.make_statics([plane]))
    assert rc == MH_ERR_INVALID_ARG and "spokes" in msg
    # a box with a non-positive edge
    sc = W.scene([("sphere", 0.25, 1.0)], 1)
    for dims in ((1.0, 0.0, 1.0), (1.0, 1.0, -2.0)):
        rc, msg = _create(sc, S.make_statics([dict(box=dims)]))
        assert rc == MH_ERR_INVALID_ARG and "edge lengths" in msg
    # an unknown type
    stt = S.make_statics([plane]); stt.type[0] = 7
    rc, msg = _create(sc, stt)
    assert rc == MH_ERR_INVALID_ARG and "type 7" in msg
    # counts above the cap
    stt = S.make_statics([plane]); stt.n = S.MH_MAX_STATICS + 1
    rc, msg = _create(sc, stt)
    assert rc == MH_ERR_INVALID_ARG and "outside [0, 8]" in msg
    stt.n = -1
    assert _create(sc, stt)[0] == MH_ERR_INVALID_ARG
    assert lib.mh_version() == 102


@pytest.mark.parametrize("nb,ground,n", [(1, 1, 8), (8, 1, 1), (2, 0, 8), (5, 1, 4), (8, 0, 2)])
def test_cap_refused_above_nine(nb, ground, n):
    """nb + has_ground + n = 10: one more than the pair arrays hold"""
    sc = S.make_scene([0.25] * nb, [1.0] * nb, (0.0, -9.81, 0.0), ground_rpy=(0.0, 0.0, 0.0) if ground else None)
    rc, msg = _create(sc, S.make_statics([dict(plane=True, R=W.R_UP)] * n))
    assert nb + ground + n == 10 and rc == MH_ERR_INVALID_ARG and "exceeds 9" in msg


@pytest.mark.parametrize("nb,ground,n", [(1, 0, 8), (8, 0, 1), (1, 1, 7), (4, 1, 4), (7, 1, 1)])
def test_cap_accepted_at_nine(nb, ground, n):
    """nb + has_ground + n = 9 passes every check: without a device the entry fails later, with MH_ERR_NO_DEVICE; with one it creates the batch"""
    sc = W.scene([("sphere", 0.25, 1.0)] * nb, n, ground=bool(ground))
    rc, msg = _create(sc, S.make_statics([dict(plane=True, R=W.R_UP)] * n))
    assert nb + ground + n == 9 and rc != MH_ERR_INVALID_ARG, msg


def test_no_statics_is_the_old_entry():
    """statics == NULL and n == 0 validate exactly as mh_world_batch_create does: same return codes, same messages"""
    lib = _lib.load()
    empty = S.mh_world_statics()
    good = S.sphere_stack_scene()
    bad = S.sphere_stack_scene(); bad.nb = 0
    bad2 = S.box_scene(); bad2.nb = 2; bad2.geom_type[1] = S.MH_GEOM_BOX
    for k in range(3):
        bad2.geom_dim[1][k] = 1.0; bad2.inertia[1][k] = 1.0
    bad2.mass[1] = 1.0
    for sc in (good, bad, bad2):
        h = ctypes.c_void_p()
        rc0 = lib.mh_world_batch_create(ctypes.addressof(sc), 2, ctypes.byref(h)); m0 = lib.mh_last_error().decode()
        if h:
            lib.mh_world_batch_destroy(h)
        for stt in (None, empty):
            rc, msg = _create(sc, stt)
            assert (rc, msg) == (rc0, m0)
    assert _create(bad, None)[0] == MH_ERR_INVALID_ARG and "box-box" in _create(bad2, empty)[1]
    # garbage in the unused entries of an empty record is never looked at
    junk = S.mh_world_statics(); junk.type[0] = 99; junk.dim[0][0] = -1.0
    assert _create(good, junk)[0] == _create(good, None)[0]


# ---- 5. the mirror of the struct, the symbols ----------------------------------------------------------------------------------------------------
def test_ctypes_mirror_has_the_c_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "moby_hip.h"\n#include "moby_hip_io_statics.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(mh_world_statics), offsetof(mh_world_statics, type), offsetof(mh_world_statics, R),\n'
                   '  offsetof(mh_world_statics, o), offsetof(mh_world_statics, dim), MH_MAX_STATICS, MH_STATIC_PLANE, MH_STATIC_BOX, MH_WORLD_STATICS, MH_VERSION); return 0; }\n')
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    T = S.mh_world_statics
    assert got == [ctypes.sizeof(T), T.type.offset, T.R.offset, T.o.offset, T.dim.offset, S.MH_MAX_STATICS, S.MH_STATIC_PLANE, S.MH_STATIC_BOX, 1, 102]
    assert S.MH_MAX_STATICS * (S.MH_MAX_STATICS + 1) // 2 == S.MH_MAX_PAIRS       # C(9, 2): one body and eight statics fill the pair arrays


def test_symbols_are_exported():
    lib = _lib.load()
    for name in ("mh_world_batch_create_statics", "mh_world_step_batch_statics"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert hasattr(mio.load(), "mh_io_load_xml_statics")
    hdr = open(os.path.join(ROOT, "include", "moby_hip_io_statics.h")).read()
    assert "int mh_io_load_xml_statics(const char* path, mh_io_scene* out, mh_world_forces* forces, mh_world_statics* statics);" in hdr


# ---- 6. the reader -------------------------------------------------------------------------------------------------------------------------------
def test_scene_file_loads():
    sc, st, ids, dt, forces, stt = mio.load_xml_statics(W.SCENE_XML)
    assert (sc.nb, sc.has_ground, stt.n, dt, forces.terms) == (1, 0, 3, 0.001, 0)
    assert ids == ["ball", "ground", "table", "wall"]
    assert list(stt.type[:3]) == [S.MH_STATIC_PLANE, S.MH_STATIC_BOX, S.MH_STATIC_PLANE]
    np.testing.assert_array_equal(np.array(stt.R[0][:]).reshape(3, 3), np.eye(3))
    np.testing.assert_array_equal(np.array(stt.R[1][:]).reshape(3, 3), S.rpy_to_R(0.0, 0.5, 0.0))
    np.testing.assert_array_equal(np.array(stt.R[2][:]).reshape(3, 3), S.rpy_to_R(0.0, 0.0, -1.5707963267949))
    assert np.array(stt.R[2][:]).reshape(3, 3)[:, 1] @ np.array([1.0, 0.0, 0.0]) == 1.0            # the wall's normal is +x
    assert list(stt.o[1][:]) == [1.0, 0.25, 0.0] and list(stt.dim[1][:]) == [1.0, 0.5, 1.0] and list(stt.o[2][:]) == [0.0, 0.0, 0.0]
    np.testing.assert_array_equal(st[0, :3], (0.9, 0.752, 0.05)); np.testing.assert_array_equal(st[0, 7:10], (-1.0, -1.0, 0.0))
    # the triangular slots over ntot = 4: (ball, ground) 0, (ball, table) 1, (ball, wall) 2, (ground, table) 3, ...
    assert [sc.cp_epsilon[p] for p in range(3)] == [0.1, 0.2, 0.6] and [sc.cp_nk[p] for p in range(3)] == [8, 4, 16]
    assert [sc.cp_mu_coulomb[p] for p in range(3)] == [0.5, 0.4, 0.1]
    assert [sc.pair_enabled[p] for p in range(6)] == [1, 1, 1, 0, 1, 1]
    assert S.pair_index(1, 2, 4) == 3


def test_old_loaders_refuse_the_scene_file():
    for load in (mio.load_xml, mio.load_xml_forces):
        with pytest.raises(mio.SceneError, match="more than one disabled body"):
            load(W.SCENE_XML)


def _variant(tmp_path, old, new):
    txt = open(W.SCENE_XML).read()
    assert old in txt
    p = tmp_path / "scene.xml"
    p.write_text(txt.replace(old, new))
    return str(p)


def test_reader_refusals(tmp_path):
    # a posed box primitive
    with pytest.raises(mio.SceneError, match="box primitive table-shape has a pose of its own"):
        mio.load_xml_statics(_variant(tmp_path, '<Box xlen="1"', '<Box rpy="0 0.1 0" xlen="1"'))
    # both rotations on a plane
    with pytest.raises(mio.SceneError, match="pose on both the body and the plane primitive"):
        mio.load_xml_statics(_variant(tmp_path, '<RigidBody id="wall" enabled="false">', '<RigidBody id="wall" enabled="false" rpy="0.1 0 0">'))
    # any other primitive on a disabled body, by name
    with pytest.raises(mio.SceneError, match="disabled body table carries a Sphere"):
        mio.load_xml_statics(_variant(tmp_path, '<RigidBody id="table" enabled="false" position="1 0.25 0" rpy="0 0.5 0"><CollisionGeometry primitive-id="table-shape"/>',
                                      '<RigidBody id="table" enabled="false"><CollisionGeometry primitive-id="ball-shape"/>'))
    # more bodies than the pair arrays hold
    many = "".join('<RigidBody id="w%d" enabled="false"><CollisionGeometry primitive-id="floor"/></RigidBody>' % k for k in range(6))
    dyn = "".join('<DynamicBody dynamic-body-id="w%d"/>' % k for k in range(6))
    txt = open(W.SCENE_XML).read().replace('<TimeSteppingSimulator constraint', many + '<TimeSteppingSimulator constraint').replace('<RecurrentForce', dyn + '<RecurrentForce')
    p = tmp_path / "many.xml"; p.write_text(txt)
    with pytest.raises(mio.SceneError, match="1 enabled and 9 disabled bodies"):
        mio.load_xml_statics(str(p))


def test_plane_pose_rules(tmp_path):
    """a plane posed through its body instead of its primitive lands in the same record"""
    a = mio.load_xml_statics(W.SCENE_XML)[5]
    b = mio.load_xml_statics(_variant(tmp_path, '<RigidBody id="wall" enabled="false">', '<RigidBody id="wall" enabled="false" position="0.5 0 0">'))[5]
    assert list(b.o[2][:]) == [0.5, 0.0, 0.0] and list(b.R[2][:]) == list(a.R[2][:])


@pytest.mark.skipif(not os.path.exists(ELLIPSE_XML), reason="no reference tree here")
def test_reference_scene_with_three_planes(tmp_path):
    """example/ellipse/ellipse2D.xml: a ground and two wall planes, all disabled bodies.  Its collision plugin (an ellipse against planes) is not built
    and stays refused; with the plugin attribute taken out -- the body's <Sphere> then collides as the sphere it is -- the three planes load."""
    with pytest.raises(mio.SceneError, match="collision detection plugin"):
        mio.load_xml_statics(ELLIPSE_XML)
    txt = open(ELLIPSE_XML).read()
    assert 'collision-detection-plugin="coldet"' in txt
    p = tmp_path / "ellipse2D.xml"
    p.write_text(txt.replace('collision-detection-plugin="coldet"', ""))
    sc, st, ids, dt, forces, stt = mio.load_xml_statics(str(p))
    assert ids == ["ellipse", "ground", "wall_neg", "wall_pos"] and (sc.nb, sc.has_ground, stt.n) == (1, 0, 3)
    assert list(stt.type[:3]) == [S.MH_STATIC_PLANE] * 3
    np.testing.assert_array_equal(np.array(stt.R[0][:]).reshape(3, 3), np.eye(3))
    np.testing.assert_array_equal(np.array(stt.R[1][:]).reshape(3, 3), S.rpy_to_R(-1.5707963267949, 0.0, 0.0))
    np.testing.assert_array_equal(np.array(stt.R[2][:]).reshape(3, 3), S.rpy_to_R(1.5707963267949, 0.0, 0.0))
    assert list(stt.o[1][:]) == [0.0, 0.0, 1.0] and list(stt.o[2][:]) == [0.0, 0.0, -1.0]
    # the walls face each other across the body: normals -z at z = +1 and +z at z = -1
    assert np.array(stt.R[1][:]).reshape(3, 3)[2, 1] == -1.0 and np.array(stt.R[2][:]).reshape(3, 3)[2, 1] == 1.0
    assert [sc.cp_mu_coulomb[p] for p in range(3)] == [1.0, 0.1, 0.1] and [sc.cp_nk[p] for p in range(3)] == [16, 16, 16]
    assert sc.cstab_max_iterations == 50 and sc.min_step_size == 1e-4
