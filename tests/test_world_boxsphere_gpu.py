"""Box-sphere contacts between free bodies in the many-worlds stepper (include/moby_hip.h, "Box-sphere pairs"; mh_world_large_bsp*.hip) against
tests/native/world_ref.cpp, bit for bit: states, trajectories and complete aux records, no tolerance anywhere.  The batches and their
reference results live in tests/world_boxsphere_ref.py (computed once per process); the conditions on the inputs are asserted there and here."""

import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import io as mio
from moby_amd import scene as S
from moby_amd.world import WorldBatch, WorldBatchDevice
from tests.world_ref import assert_aux_equal, reference
from tests.world_boxsphere_ref import (EDGE, FACE, PENETRATING, SCENE_XML, VERTEX, centre_inside_box, gpu_cases, reference_run)

pytestmark = pytest.mark.gpu


def run_host(case, want_traj=True):
    """the case through the host convenience entry (one launch): -> (state, aux, trajectory)"""
    wb = WorldBatch(case["scene"], case["state"].copy(), forces=case.get("forces"))
    traj = wb.step(case["dt"], case["nsteps"], want_traj=want_traj, wrench=case.get("wrench"))
    return wb.state, wb.aux, traj


def check_case(name):
    case, st_r, aux_r, traj_r, census = reference_run(name)
    assert not centre_inside_box(case["scene"], case["state"])
    st, aux, traj = run_host(case)
    np.testing.assert_array_equal(traj, traj_r)
    np.testing.assert_array_equal(st, st_r)
    assert_aux_equal(aux, aux_r)
    return census


def test_face_region():
    """(a) 1 box + 1 sphere + plane, 8 worlds: the sphere lands on the top face of the resting box (mu 0.4, epsilon 0.2, NK 4, 30 steps of 1e-3)"""
    census = check_case("face")
    assert census[:, :, FACE].sum() > 0


def test_edge_and_vertex_regions():
    """(b) the box floating under a random quaternion, the sphere aimed at an edge (4 worlds) and at a vertex (4 worlds); over (a) + (b) the census shows
    face, edge, vertex and penetrating contacts"""
    census = check_case("edge_vertex")
    assert census[:4, :, EDGE].sum() > 0 and census[4:, :, VERTEX].sum() > 0
    total = census.sum(axis=(0, 1)) + reference_run("face")[4].sum(axis=(0, 1))
    assert (total[[FACE, EDGE, VERTEX, PENETRATING]] > 0).all(), total


def test_sphere_as_lower_id():
    """(c) sphere = body 0, box = body 1: the contact is still created as (box, sphere), the signed-distance points stay with their bodies"""
    check_case("id_order")


def test_full_image():
    """(d) MH_MAX_BODIES bodies, 4 boxes and 4 spheres with all 16 box-sphere pairs, the sphere pairs and every ground pair enabled; one island spans box
    vertex contacts, a box-sphere contact and a sphere-sphere contact"""
    case = gpu_cases()["full"]
    sc = case["scene"]
    assert sc.nb == S.MH_MAX_BODIES
    kinds = [sc.geom_type[b] for b in range(sc.nb)]
    en = {(i, j): sc.pair_enabled[S.pair_index(i, j, sc.nb + 1)] for i in range(sc.nb + 1) for j in range(i + 1, sc.nb + 1)}
    assert sum(en[i, j] for i in range(8) for j in range(i + 1, 8) if {kinds[i], kinds[j]} == {S.MH_GEOM_BOX, S.MH_GEOM_SPHERE}) == 16
    assert sum(en[i, j] for i in range(8) for j in range(i + 1, 8) if kinds[i] == kinds[j] == S.MH_GEOM_BOX) == 0
    assert all(en[i, 8] for i in range(8)) and all(en[i, j] for i in range(8) for j in range(i + 1, 8) if kinds[i] == kinds[j] == S.MH_GEOM_SPHERE)
    check_case("full")


def test_full_image_with_parameters_per_pair():
    """(d, parameters) the same eight bodies with (epsilon, mu-coulomb, NK in {4, 8}) of its own in every pair slot, two sphere-sphere pairs and a
    sphere-ground pair disabled: a cp_* or pair_enabled read at another triangular index gives another result (the conditions on this input:
    tests/world_boxsphere_ref.py check_full_params_conditions, asserted by reference_run)"""
    check_case("full_params")


def test_full_image_with_parameters_per_pair_through_the_statics_build():
    """(d, parameters, key 16) the same batch through mh_world_large_st: its triangular indices run over nb + has_ground + n with n = 0"""
    lib = _lib.load()
    try:
        _lib.check(lib.mh_debug_set(16, 1))
        check_case("full_params")
    finally:
        _lib.check(lib.mh_debug_set(16, 0))


def test_noslip_model():
    """(e) mu-coulomb = 100 on every pair: the no-slip model over an island of box vertex contacts and a box-sphere contact"""
    check_case("noslip")


def test_noslip_capacity_flagged_like_the_reference():
    """(e, capacity) two boxes flat on the plane and a ball landing on the seam between them, mu-coulomb = 100: one no-slip island of ten contacts.  Every
    world must be flagged MH_WORLD_UNSUPPORTED at the same step as the reference -- never approximated.  (The kernel's no-slip island holds 6 contacts
    (MHW_NS_MAXC) and flags the island itself; the reference's handler holds MH_NOSLIP_MAX = 16 and flags the restitution pass it cannot restate
    (oracle/world.hpp, apply_no_slip_model_to_island): both flags rise in the step of the ball's impact.)"""
    case, _, aux_r, _, _ = reference_run("noslip_capacity")
    assert ((aux_r["status"] & S.MH_WORLD_UNSUPPORTED) != 0).all()
    B = case["state"].shape[0]

    st, aux = case["state"].copy(), S.new_aux(B)
    got, want = np.full(B, -1), np.full(B, -1)
    dev = WorldBatchDevice(case["scene"], case["state"])
    try:
        for s in range(case["nsteps"]):                            # one step per launch, until both sides have flagged every world
            dev.step(case["dt"], 1)
            reference().step(case["scene"], st, aux, case["dt"], 1)
            got[(got < 0) & ((dev.download()[1]["status"] & S.MH_WORLD_UNSUPPORTED) != 0)] = s
            want[(want < 0) & ((aux["status"] & S.MH_WORLD_UNSUPPORTED) != 0)] = s
            if (got >= 0).all() and (want >= 0).all():
                break
    finally:
        dev.close()
    print("first flagged step: kernel", got, "reference", want)
    assert (want >= 0).all()
    np.testing.assert_array_equal(got, want)


def test_stabiliser_rows():
    """(f) a sphere 1e-4 inside the top face (dist < 0: the contact function's own row) and a second sphere hovering 1e-3 above it (the synthetic row of a
    separated pair); cstab_max_iterations = 10"""
    case, _, aux_r, _, _ = reference_run("stab")
    assert case["scene"].cstab_max_iterations == 10 and (aux_r["stab_iters"] > 0).all()
    check_case("stab")


def test_with_forces():
    """(g) case (a) with Stokes drag stored and one wrench row on the box: the forced box-sphere object (mh_world_large_bsp_forces.hip)"""
    check_case("face_forces")


def test_launch_variants():
    """(h) case (a) in one launch == in three launches == through step_ids on a shuffled id list"""
    import torch
    case, st_r, aux_r, _, _ = reference_run("face")
    dev = WorldBatchDevice(case["scene"], case["state"])
    try:
        for _ in range(3):
            dev.step(case["dt"], case["nsteps"] // 3)
        st, aux = dev.download()
    finally:
        dev.close()
    np.testing.assert_array_equal(st, st_r)
    assert_aux_equal(aux, aux_r)
    dev = WorldBatchDevice(case["scene"], case["state"])
    try:
        ids = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4], dtype=torch.int32, device="cuda")
        dev.step_ids(case["dt"], case["nsteps"], ids.data_ptr(), 8)
        st, aux = dev.download()
    finally:
        dev.close()
    np.testing.assert_array_equal(st, st_r)
    assert_aux_equal(aux, aux_r)


def test_ab_switch_changes_no_result():
    """(i) a mixed scene with the box-sphere pairs disabled under mh_debug_set(15, 1) (the box-sphere objects) equals the plain large kernels, which equal
    the reference; occupancy() >= 1 for both"""
    case, st_r, aux_r, traj_r, _ = reference_run("disabled")
    lib = _lib.load()
    out = []
    try:
        for key in (0, 1):
            _lib.check(lib.mh_debug_set(15, key))
            dev = WorldBatchDevice(case["scene"], case["state"])
            try:
                assert dev.occupancy() >= 1
                dev.step(case["dt"], case["nsteps"])
                out.append(dev.download())
            finally:
                dev.close()
    finally:
        _lib.check(lib.mh_debug_set(15, 0))
    for st, aux in out:
        np.testing.assert_array_equal(st, st_r)
        assert_aux_equal(aux, aux_r)


def test_scene_file():
    """(j) tests/scenes/ball_on_crate.xml through the loader and WorldBatch equals the reference"""
    sc, st0, ids, dt = mio.load_xml(SCENE_XML)
    assert ids == ["ball", "crate", "ground"] and dt == 1e-3
    assert not centre_inside_box(sc, st0)
    st_r, aux_r = st0.copy(), S.new_aux(1)
    traj_r, census = reference().step(sc, st_r, aux_r, dt, 30, want_traj=True, want_census=True)[:2]
    assert (aux_r["status"] & ~S.MH_WORLD_IMPACT_TOL) == 0 and aux_r["lcp_solves"][0] > 0 and census[:, :, FACE].sum() > 0
    wb = WorldBatch(sc, st0.copy())
    traj = wb.step(dt, 30, want_traj=True)
    np.testing.assert_array_equal(traj, traj_r)
    np.testing.assert_array_equal(wb.state, st_r)
    assert_aux_equal(wb.aux, aux_r)
