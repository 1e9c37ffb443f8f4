"""Static planes and boxes among the free bodies of the many-worlds stepper (include/moby_hip.h, "Static bodies"; mh_world_large_st*.hip) against
tests/native/world_ref.cpp, bit for bit: states, trajectories and complete aux records, no tolerance anywhere.  The batches and their
reference results live in tests/world_statics_ref.py (computed once per process); worlds differ through world_uniforms."""
import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import io as mio
from moby_amd import scene as S
from moby_amd.synth import world_uniforms
from moby_amd.world import WorldBatch, WorldBatchDevice
from tests.world_ref import assert_aux_equal, reference
from tests import world_statics_ref as W
from tests.world_statics_ref import EDGE, FACE, PENETRATING, VERTEX, gpu_cases, reference_run

pytestmark = pytest.mark.gpu


def run_host(case, want_traj=True):
    """the case through the host convenience entry (one launch): -> (state, aux, trajectory)"""
    wb = WorldBatch(case["scene"], case["state"].copy(), forces=case.get("forces"), statics=case["statics"])
    traj = wb.step(case["dt"], case["nsteps"], want_traj=want_traj, wrench=case.get("wrench"))
    return wb.state, wb.aux, traj


def check_case(name):
    case, st_r, aux_r, traj_r, census = reference_run(name)
    st, aux, traj = run_host(case)
    np.testing.assert_array_equal(traj, traj_r)
    np.testing.assert_array_equal(st, st_r)
    assert_aux_equal(aux, aux_r)
    return st, aux, census


def test_one_static_plane_under_eight_bodies():
    """(1) nb = 8, no scene ground, one static plane: the pair (7, plane) is slot 35, the last one.  Equals the reference, and the result of the existing
    ground path (the same plane as the scene's own ground) from this process"""
    sc = gpu_cases()["plane8"]["scene"]
    assert (sc.nb, sc.has_ground, gpu_cases()["plane8"]["statics"].n) == (8, 0, 1) and S.pair_index(7, 8, 9) == S.MH_MAX_PAIRS - 1
    st, aux, _ = check_case("plane8")
    g = gpu_cases()["plane8_ground"]
    assert g["scene"].has_ground == 1 and g["statics"] is None
    st_g, aux_g, traj_g = run_host(g)
    np.testing.assert_array_equal(st, st_g)
    assert_aux_equal(aux, aux_g)
    np.testing.assert_array_equal(traj_g, reference_run("plane8")[3])
    assert aux_g["stab_iters"].sum() > 0 and (aux_g["lcp_solves"] > 100).all()


def test_eight_statics_around_one_body():
    """(2) nb = 1, n = 8: four planes and four boxes around one ball; 28 of the 36 pair lanes are static-static and never kept"""
    case = gpu_cases()["ring"]
    assert (case["scene"].nb, case["statics"].n) == (1, 8) and sorted(case["statics"].type[:8]) == [0, 0, 0, 0, 1, 1, 1, 1]
    _, aux, census = check_case("ring")
    assert census[:, :, FACE].sum() > 0 and (aux["lcp_solves"] >= 2).all()


def test_ball_in_a_corner():
    """(3) one ball touching floor, wall and a turned static box at once: three contacts in one island; the stabiliser runs with rows of both kinds
    (worlds start a fraction of a micrometre inside or outside each of the three)"""
    case = gpu_cases()["corner"]
    for w in range(case["state"].shape[0]):
        got = [reference().pair(case["scene"], case["state"][w], p, 1e-6, statics=case["statics"]) for p in range(3)]
        assert [g["b"] for g in got] == [1, 2, 3]
    d = np.array([[reference().pair(case["scene"], case["state"][w], p, 1e-6, statics=case["statics"])["dist"] for p in range(3)] for w in range(case["state"].shape[0])])
    assert (np.abs(d) < 1e-6).all() and (d < 0).any() and (d > 1.5e-8).any()
    _, aux, _ = check_case("corner")
    assert (aux["stab_iters"] > 0).all() and (aux["lcp_rows"] >= 3 * 20).all()


def test_face_edge_and_vertex_regions_of_a_turned_box():
    """(4) balls meeting a static box turned about two axes in its face (worlds 0-3), edge (4-7) and vertex (8-11) regions, by the reference's census"""
    assert not np.array_equal(W.REGION_R, np.eye(3))
    _, _, census = check_case("regions")
    assert (census[:4, :, FACE].sum(axis=1) > 0).all() and (census[4:8, :, EDGE].sum(axis=1) > 0).all() and (census[8:, :, VERTEX].sum(axis=1) > 0).all()
    assert census[:, :, PENETRATING].sum() > 0


def test_box_body_against_floor_and_wall():
    """(5) a box body flat on the floor and flush against the wall: eight vertex contacts in one island, LCPs of 64 rows"""
    _, aux, _ = check_case("box_corner")
    assert (aux["lcp_rows"] // aux["lcp_solves"] >= 56).all()


def test_capacity_is_flagged_in_the_step_of_the_reference():
    """(5, capacity) the same box with a ball landing on top: a ninth contact in the island, 72 LCP rows / 27 Jacobian rows, beyond the solver and
    beyond the image.  Every world must be flagged MH_WORLD_UNSUPPORTED in the step the reference flags it -- never approximated"""
    case = gpu_cases()["box_corner_capacity"]
    B = case["state"].shape[0]
    st, aux = case["state"].copy(), S.new_aux(B)
    got, want = np.full(B, -1), np.full(B, -1)
    dev = WorldBatchDevice(case["scene"], case["state"], statics=case["statics"])
    try:
        for s in range(case["nsteps"]):                            # one step per launch, until both sides have flagged every world
            dev.step(case["dt"], 1)
            reference().step(case["scene"], st, aux, case["dt"], 1, statics=case["statics"])
            st_g, aux_g = dev.download()
            got[(got < 0) & ((aux_g["status"] & S.MH_WORLD_UNSUPPORTED) != 0)] = s
            want[(want < 0) & ((aux["status"] & S.MH_WORLD_UNSUPPORTED) != 0)] = s
            if (got >= 0).any() or (want >= 0).any():
                break
            np.testing.assert_array_equal(st_g, st)                # until then: the usual equality
            assert_aux_equal(aux_g, aux)
    finally:
        dev.close()
    print("first flagged step: kernel", got, "reference", want)
    assert (want >= 0).all()
    np.testing.assert_array_equal(got, want)


def test_noslip_model_on_a_static_box():
    """(6) mu-coulomb = 100: the no-slip model for a ball landing on the top of a turned static box"""
    _, aux, census = check_case("noslip_table")
    assert census[:, :, FACE].sum() > 0


def test_with_forces():
    """(7) the forced statics object (mh_world_large_st_forces.hip): Stokes drag and damping stored, a wrench row per step"""
    case = gpu_cases()["forces"]
    assert case["forces"].terms == 3 and case["wrench"].shape[0] == case["nsteps"]
    check_case("forces")


def test_launch_variants():
    """(8) the corner case in one launch with a trajectory == in four launches == through step_ids on a shuffled id list"""
    import torch
    case, st_r, aux_r, _, _ = reference_run("corner")
    dev = WorldBatchDevice(case["scene"], case["state"], statics=case["statics"])
    try:
        for _ in range(4):
            dev.step(case["dt"], case["nsteps"] // 4)
        st, aux = dev.download()
    finally:
        dev.close()
    np.testing.assert_array_equal(st, st_r)
    assert_aux_equal(aux, aux_r)
    dev = WorldBatchDevice(case["scene"], case["state"], statics=case["statics"])
    try:
        ids = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4], dtype=torch.int32, device="cuda")
        dev.step_ids(case["dt"], case["nsteps"], ids.data_ptr(), 8)
        st, aux = dev.download()
    finally:
        dev.close()
    np.testing.assert_array_equal(st, st_r)
    assert_aux_equal(aux, aux_r)


def test_mixed_scene_with_ground_and_statics():
    """(12) has_ground = 1 AND n = 2: the statics sit one slot up in the kernel's cache (the ground in slot 0).  A tilted ground off the origin, a plane
    turned about two axes off the origin, a static box turned about two axes, a sphere, a box body and a second sphere; 15 pair slots with parameters
    of their own, two of them disabled (the conditions on this input: tests/world_statics_ref.py check_mixed_conditions, asserted by reference_run)"""
    case = gpu_cases()["mixed"]
    sc = case["scene"]
    assert (sc.nb, sc.has_ground, case["statics"].n) == (3, 1, 2)
    _, aux, _ = check_case("mixed")
    assert (aux["stab_iters"] > 0).any()


def test_mixed_scene_equals_its_ground_as_static_twin():
    """(13) the same scene with has_ground = 0, its ground handed over as static 0 and the two statics one slot up: bodies and pair slots are where they
    were, so state, aux and trajectory are bit-equal -- a comparison of the device with itself, no reference in it"""
    case = gpu_cases()["mixed"]
    sc2, stt2 = W.ground_to_static(case["scene"], case["statics"])
    assert (sc2.has_ground, stt2.n) == (0, 3) and list(stt2.type[:3]) == [S.MH_STATIC_PLANE, S.MH_STATIC_PLANE, S.MH_STATIC_BOX]
    st, aux, traj = run_host(case)
    st2, aux2, traj2 = run_host(dict(case, scene=sc2, statics=stt2))
    np.testing.assert_array_equal(traj2, traj)
    np.testing.assert_array_equal(st2, st)
    assert_aux_equal(aux2, aux)
    assert aux2.tobytes() == aux.tobytes()
    # the ball shot at the wall its pair with is disabled has left through it
    r = W.MIXED_BODIES[0][1]
    for w in W.MIXED_THROUGH:
        assert W.plane_height(W.MIXED_WALL_R, W.MIXED_WALL_O, st[w, 0:3]) < -r < r < W.plane_height(W.MIXED_WALL_R, W.MIXED_WALL_O, case["state"][w, 0:3])


def test_mixed_scene_with_forces():
    """(14) the mixed scene through the forced statics object: Stokes drag and damping on all three bodies, a wrench row per step"""
    case = gpu_cases()["mixed_forces"]
    assert case["forces"].terms == 3 and case["wrench"].shape == (case["nsteps"], 8, 3, 6)
    assert all(case["forces"].stokes_b[b] > 0 and case["forces"].damp_kl[b] > 0 for b in range(3))
    st, _, _ = check_case("mixed_forces")
    assert not np.array_equal(st, reference_run("mixed")[1])


def test_mixed_scene_launch_variants():
    """(15) the mixed scene in three launches == in one launch == through step_ids on a shuffled id list"""
    import torch
    case, st_r, aux_r, _, _ = reference_run("mixed")
    st1, aux1, _ = run_host(case, want_traj=False)
    dev = WorldBatchDevice(case["scene"], case["state"], statics=case["statics"])
    try:
        for _ in range(3):
            dev.step(case["dt"], case["nsteps"] // 3)
        st, aux = dev.download()
    finally:
        dev.close()
    np.testing.assert_array_equal(st, st1)
    assert_aux_equal(aux, aux1)
    dev = WorldBatchDevice(case["scene"], case["state"], statics=case["statics"])
    try:
        ids = torch.tensor([6, 1, 4, 7, 0, 3, 5, 2], dtype=torch.int32, device="cuda")
        dev.step_ids(case["dt"], case["nsteps"], ids.data_ptr(), 8)
        st, aux = dev.download()
    finally:
        dev.close()
    np.testing.assert_array_equal(st, st1)
    assert_aux_equal(aux, aux1)
    np.testing.assert_array_equal(st, st_r)
    assert_aux_equal(aux, aux_r)


def test_key_16_changes_no_result():
    """(9) a ground-only scene with an enabled box-sphere pair through mh_world_large_bsp (key 16 = 0) and through mh_world_large_st (key 16 = 1):
    bit-equal, and equal to the reference"""
    from tests.world_boxsphere_ref import face_batch
    sc, st0 = face_batch(8)
    st_r, aux_r = st0.copy(), S.new_aux(8)
    reference().step(sc, st_r, aux_r, 1e-3, 30)
    lib = _lib.load()
    out = []
    try:
        for key in (0, 1):
            _lib.check(lib.mh_debug_set(16, key))
            dev = WorldBatchDevice(sc, st0)
            try:
                assert dev.occupancy() >= 1
                dev.step(1e-3, 30)
                out.append(dev.download())
            finally:
                dev.close()
    finally:
        _lib.check(lib.mh_debug_set(16, 0))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    assert out[0][1].tobytes() == out[1][1].tobytes()
    for st, aux in out:
        np.testing.assert_array_equal(st, st_r)
        assert_aux_equal(aux, aux_r)


def test_occupancy_equals_the_ground_only_twin():
    """(10) resident workgroups per CU of a statics batch = those of the same scene with the plane as its ground, plain and with forces stored"""
    a, g = gpu_cases()["plane8"], gpu_cases()["plane8_ground"]
    da = WorldBatchDevice(a["scene"], a["state"], statics=a["statics"])
    dg = WorldBatchDevice(g["scene"], g["state"])
    try:
        occ = (da.occupancy(), dg.occupancy())
        f = S.make_forces(8, stokes=(0.1, 0.1))
        da.set_forces(f); dg.set_forces(f)
        occ_f = (da.occupancy(), dg.occupancy())
    finally:
        da.close(); dg.close()
    print("occupancy statics / ground twin:", occ, "with forces:", occ_f)
    assert occ[0] == occ[1] >= 1 and occ_f[0] == occ_f[1] >= 1


def test_scene_file():
    """(11) tests/scenes/ball_in_corner.xml through the loader and WorldBatch(statics=), four worlds a little apart, equals the reference"""
    sc, st0, ids, dt, forces, stt = mio.load_xml_statics(W.SCENE_XML)
    assert ids == ["ball", "ground", "table", "wall"] and dt == 1e-3 and forces.terms == 0
    st0 = np.repeat(st0, 4, axis=0)
    for w in range(4):
        u = world_uniforms(1100 + w, 2)
        st0[w, 0] += 0.05 * (u[0] - 0.5); st0[w, 1] += 1e-3 * u[1]
    st_r, aux_r = st0.copy(), S.new_aux(4)
    traj_r, census = reference().step(sc, st_r, aux_r, dt, 30, statics=stt, want_traj=True, want_census=True)[:2]
    assert ((aux_r["status"] & ~S.MH_WORLD_IMPACT_TOL) == 0).all() and (aux_r["lcp_solves"] > 0).all() and census[:, :, :PENETRATING].sum() > 0
    wb = WorldBatch(sc, st0.copy(), statics=stt)
    traj = wb.step(dt, 30, want_traj=True)
    np.testing.assert_array_equal(traj, traj_r)
    np.testing.assert_array_equal(wb.state, st_r)
    assert_aux_equal(wb.aux, aux_r)
