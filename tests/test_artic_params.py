"""Per-world parameters of the articulated stepper (include/moby_hip_artic.h, "Per-world parameters") without a GPU: the layout of the record, the
record that reproduces the model, the refusals (they run before the device is looked for), and the coverage of the GPU cases of
tests/artic_params_ref.py, proven on the reference alone so that tests/test_artic_params_gpu.py cannot pass vacuously."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import artic as A
from moby_amd import scene as S
from tests import artic_boxsphere_ref as BS
from tests import artic_params_ref as P
from tests import artic_report_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MH_ERR_INVALID_ARG = -1


@pytest.fixture(scope="module")
def ref():
    return R.build_report_ref()


def _create(m, params, B, flags=0):
    h = ctypes.c_void_p()
    rc = _lib.load().mh_artic_batch_create_params(ctypes.byref(m), None if params is None else params.ctypes.data, B, flags, ctypes.byref(h))
    msg = _lib.load().mh_last_error().decode()
    if h:
        _lib.load().mh_artic_batch_destroy(h)
    return rc, msg


def test_mirrors_have_the_c_layout(tmp_path):
    names = A.PARAMS_DTYPE.names
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "moby_hip_artic.h"\nint main(void) {\n  printf("%zu %d %d\\n", sizeof(mh_artic_params), MH_ARTIC_PARAMS, MH_ARTIC_CREATE_REPORT);\n'
                   + "".join('  printf("%%zu %%zu\\n", offsetof(mh_artic_params, %s), sizeof(((mh_artic_params*)0)->%s));\n' % (f, f) for f in names) + "  return 0; }\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [[int(x) for x in ln.split()] for ln in subprocess.check_output([exe]).decode().splitlines()]
    T = A.mh_artic_params
    assert got[0] == [ctypes.sizeof(T), 1, A.MH_ARTIC_CREATE_REPORT]
    assert got[0][0] == A.PARAMS_DTYPE.itemsize == 8 * A.PARAMS_DOUBLES
    assert [f for f, _ in T._fields_] == list(names)                      # the header's fields, in its order, in both mirrors
    D = A.PARAMS_DTYPE.fields
    for f, (off, size) in zip(names, got[1:]):
        assert (getattr(T, f).offset, getattr(T, f).size) == (off, size), f
        assert (D[f][1], D[f][0].itemsize) == (off, size), f
    assert all(D[f][0].base == np.float64 for f in names)                 # doubles only: nothing in the record can become an index
    assert sum(size for _, size in got[1:]) == got[0][0]                  # ... and no padding between them


def test_record_of_the_model_byte_for_byte():
    """mh_artic_params_from_model and artic.make_params agree byte for byte, and writing the record back gives the model's bytes"""
    m = BS.mixed_all()[0]
    rec = A.mh_artic_params()
    _lib.load().mh_artic_params_from_model(ctypes.byref(m), ctypes.byref(rec))
    p = A.make_params(m, 3)
    for w in range(3):
        assert p[w].tobytes() == bytes(rec)
    assert p["cp_mu_coulomb"][2] == 100.0 and p["box_len"][1, 1, 0] == 0.3 and p["sphere_radius"][0, 1] == 0.08
    assert bytes(P.model_of_world(m, p, 2)) == bytes(m)
    p["mass"][1, 6] = 0.7
    m1 = P.model_of_world(m, p, 1)
    assert m1.mass[6] == 0.7 and bytes(m1) != bytes(m) and m1.nj == m.nj and list(m1.parent) == list(m.parent)


def _bad(field, w, idx, value, nB=4):
    m = BS.mixed_all()[0]
    p = A.make_params(m, nB)
    if idx is None:
        p[field][w] = value
    else:
        p[field][(w,) + idx] = value
    return _create(m, p, nB)


# mixed_all: a floating base (joints 0..5 virtual), joint 6 with finite limits, joint 7 with none, two spheres, a link box and a static box
@pytest.mark.parametrize("field,idx,value,word", [
    ("mass", (6,), -1.0, "mass"), ("mass", (6,), float("nan"), "mass"), ("mass", (7,), 0.0, "carries no mass"),
    ("axis", (6, 1), 0.5, "axis"), ("axis", (4, 0), 0.1, "axis"), ("com", (2, 1), 0.1, "floating_base"), ("trel", (3, 2), 0.2, "floating_base"),
    ("Rrel", (1, 0), 0.9, "floating_base"),
    ("lolimit", (6,), 2.0, "lower limit above the upper"), ("hilimit", (6,), float("nan"), "limit"),
    ("hilimit", (7,), 1.5, "hilimit"), ("lolimit", (7,), -1.5, "lolimit"),                      # a limit made finite where the model has none
    ("lolimit", (6,), -np.finfo(float).max, "lolimit"),                                         # ... and one removed
    ("gravity", (1,), float("inf"), "gravity"),
    ("sphere_radius", (1,), 0.0, "radius"), ("sphere_radius", (0,), float("nan"), "radius"),
    ("box_len", (0, 2), -0.1, "edge lengths"), ("box_len", (1, 0), float("inf"), "edge lengths"), ("box_R", (1, 4), 0.9, "box_R"),
    ("plane_R", (4,), 0.5, "plane_R"), ("plane_R", (1,), float("nan"), "plane_R"),
    ("cp_epsilon", None, -0.1, "contact parameters"), ("cp_epsilon", None, float("inf"), "contact parameters"),
    ("cp_mu_coulomb", None, float("nan"), "contact parameters"), ("cp_mu_coulomb", None, float("inf"), "contact parameters"),
    ("cp_mu_viscous", None, -1.0, "contact parameters"), ("cp_compliance", None, float("nan"), "contact parameters")])
@pytest.mark.parametrize("w", [0, 3])
def test_refusals_name_the_world_and_the_field(field, idx, value, word, w):
    rc, msg = _bad(field, w, idx, value)
    assert rc == MH_ERR_INVALID_ARG and msg.startswith("world %d:" % w) and word in msg, msg


def test_records_that_pass_and_what_comes_first():
    """records equal to the model, NULL records and varied records pass the checks (without a device the entry then ends with MH_ERR_NO_DEVICE, with one
    it creates the batch); the refusals of mh_artic_batch_create come first and carry no world; values the topology does not use are not looked at"""
    m = BS.mixed_all()[0]
    for p in (None, A.make_params(m, 3), P.vary(m, 3, 1, [0.5, 100.0, 0.3])):
        rc, msg = _create(m, p, 3, A.MH_ARTIC_CREATE_REPORT)
        assert rc != MH_ERR_INVALID_ARG, msg
    p = A.make_params(m, 2)
    p["sphere_radius"][1, 2:] = -1.0; p["box_len"][1, 2:] = np.nan; p["mass"][1, 8:] = -1.0
    assert _create(m, p, 2)[0] != MH_ERR_INVALID_ARG
    bad = BS.mixed_all()[0]; bad.parent[7] = 9
    rc, msg = _create(bad, None, 2)
    assert rc == MH_ERR_INVALID_ARG and msg.startswith("joint 7") and "world" not in msg
    bare = A.chain_model(3)
    rc, msg = _create(bare, None, 2, A.MH_ARTIC_CREATE_REPORT)            # the report flag makes it a report batch: a model without a slot is refused
    assert rc == MH_ERR_INVALID_ARG and "no slot" in msg
    assert _create(bare, None, 2)[0] != MH_ERR_INVALID_ARG               # ... without it the robot alone is the main use
    assert _create(m, None, 2, 6)[0] == MH_ERR_INVALID_ARG               # unknown flag bits
    pb = A.make_params(bare, 2); pb["cp_mu_coulomb"][1] = np.nan; pb["plane_R"][1] = np.nan      # no geometry: contact values are not looked at
    assert _create(bare, pb, 2)[0] != MH_ERR_INVALID_ARG
    # cp_nk is validated whatever the model's own mu (worlds below 100 may join the batch later): mh_artic_batch_create takes this model
    odd = BS.mixed_all()[0]; odd.cp_nk = 5
    rc, msg = _create(odd, None, 2)
    assert rc == MH_ERR_INVALID_ARG and "cp_nk" in msg


def test_the_setters_refuse_a_null_batch():
    lib = _lib.load()
    p = A.make_params(BS.mixed_all()[0], 1)
    assert lib.mh_artic_batch_set_params(None, p.ctypes.data, 0, 1) == MH_ERR_INVALID_ARG and "null batch" in lib.mh_last_error().decode()
    assert lib.mh_artic_batch_set_params_dev(None, None, p.ctypes.data, 0, 1) == MH_ERR_INVALID_ARG and "null batch" in lib.mh_last_error().decode()


def test_python_side_checks_the_records():
    m = BS.mixed_all()[0]
    z = np.zeros((2, m.nj))
    for bad in (np.zeros((2, A.PARAMS_DOUBLES)), A.make_params(m, 3), A.make_params(m, 2).reshape(2, 1)):
        with pytest.raises(ValueError, match="PARAMS_DTYPE"):
            A.ArticBatch(m, z, z, params=bad)


def test_the_contact_reference_steps_a_model_without_geometry_as_the_plain_oracle(oracle, ref):
    """the rule makes a params batch of the robot alone step through the contact kernels: with an empty contact list the contact reference and the
    plain oracle (oracle/artic.hpp) agree bit for bit, with and without the stabiliser, CRB and FSAB"""
    for stab, alg in ((0, A.MH_ARTIC_CRB), (10, A.MH_ARTIC_FSAB)):
        m, q0, qd0, dt = P.chain6()
        m.cstab_max_iterations = stab; m.algorithm = alg
        q, qd, aux = q0[:4].copy(), qd0[:4].copy(), S.new_aux(4)
        ref.step_report(m, q, qd, aux, dt, 100)
        qo, qdo, auxo = q0[:4].copy(), qd0[:4].copy(), S.new_aux(4)
        oracle.artic_step(m, qo, qdo, auxo, dt, 100)
        from tests.test_artic_box_gpu import same
        same((q, qd, aux), (qo, qdo, auxo), 4)
        assert (aux["lcp_solves"] > 0).any() and (stab == 0 or (aux["stab_iters"] > 0).any())
        # (the two part ways only behind MH_WORLD_UNSUPPORTED, which freezes a world in the contact step and not in the plain one; without
        #  restitution on coupled limits, as here, no world gets it)
        assert not (aux["status"] & S.MH_WORLD_UNSUPPORTED).any()


def test_equal_records_are_the_shared_run(ref):
    """the per-world loop with every record equal to the model is the reference's own batched run"""
    case = P.CASES[1]
    m, q0, qd0, dt, n, _ = P.case_model(ref, case)
    p = A.make_params(m, P.B)
    q, qd, aux = q0.copy(), qd0.copy(), S.new_aux(P.B)
    rep = P.step_worlds(ref, m, p, q, qd, aux, dt, n)
    q1, qd1, aux1 = q0.copy(), qd0.copy(), S.new_aux(P.B)
    rep1 = ref.step_report(m, q1, qd1, aux1, dt, n)
    assert np.array_equal(q, q1) and np.array_equal(qd, qd1) and aux.tobytes() == aux1.tobytes() and np.array_equal(rep, rep1)


@pytest.mark.parametrize("case", P.CASES, ids=P.case_id)
def test_gpu_cases_are_covered_on_the_reference(ref, case):
    """conditions on the reference's own runs: every world's run differs from the run of the same start state under record 0; in a mixed-mu case
    worlds on both sides of mu = 100 solve LCPs; with geometry at least one report row has a positive normal impulse"""
    m, q0, qd0, dt, n, p, out = P.reference_run(ref, case)
    last = out[-1]
    # (MH_WORLD_UNSUPPORTED -- a restitution pass that leaves a constraint approaching again -- freezes a world in the contact kernels: none here)
    assert not (last["aux"]["status"] & (S.MH_WORLD_UNSUPPORTED | S.MH_WORLD_STALLED)).any()
    p0 = p[np.zeros(P.B, dtype=int)]                                       # record 0 in every world
    q, qd, aux = q0.copy(), qd0.copy(), S.new_aux(P.B)
    Pp = P.world_pose(m, p0) if case[1] == "pose" else None
    P.step_worlds(ref, m, p0, q, qd, aux, dt, n, pose=Pp, drive=out[0]["drive"], worlds=range(1, P.B))
    for w in range(1, P.B):
        assert not np.array_equal(q[w], out[0]["q"][w]) and not np.array_equal(qd[w], out[0]["qd"][w]), "world %d steps as under record 0" % w
    assert len({p[w].tobytes() for w in range(P.B)}) == P.B
    mu = p["cp_mu_coulomb"]
    if case[4] is P.MIXED:
        assert (last["aux"]["lcp_solves"][mu >= 100.0] > 0).any() and (last["aux"]["lcp_solves"][mu < 100.0] > 0).any()
        assert (mu >= 100.0).any() and (mu < 100.0).any()
    if case[4] is not None:
        assert max((o["report"][..., 1].sum(axis=1) > 0.0).sum() for o in out) > 0, "no report row with a positive normal impulse"
    else:
        assert (last["aux"]["lcp_solves"] > 0).sum() >= P.B // 2           # the robot alone: the worlds meet their limits


def test_switched_records_change_the_second_launch(ref):
    """the setter tests' reference run: worlds 2..4 get other records between the launches and then step differently from the unswitched run; the
    others continue bit for bit"""
    case = P.CASES[1]
    a = P.reference_run(ref, case)[-1]
    b = P.reference_run(ref, case, P.switched, "switched")[-1]
    assert np.array_equal(a[0]["q"], b[0]["q"])
    for w in range(P.B):
        assert np.array_equal(a[1]["q"][w], b[1]["q"][w]) == (w not in (2, 3, 4)), w


def test_cpp_adapter_takes_records(tmp_path):
    """MobyHipArticulatedBody.h: with_params + set_params build with plain g++ against the C ABI, and the refusal of a record reaches the caller as
    an exception that names the world"""
    src = tmp_path / "pw.cpp"
    src.write_text('#include <cstdio>\n#include <vector>\n#include "MobyHipArticulatedBody.h"\n'
                   'int main() {\n  mh_artic_model m = mh_artic_model();\n  m.nj = 3; m.gravity[2] = -9.81;\n'
                   '  for (int i = 0; i < 3; i++) { m.parent[i] = i - 1; m.axis[i][1] = 1.0; m.mass[i] = 1.0; m.trel[i][2] = -0.5; m.lolimit[i] = -1.0; m.hilimit[i] = 1.0;\n'
                   '    for (int k = 0; k < 3; k++) { m.Rrel[i][4 * k] = 1.0; m.inertia[i][4 * k] = 0.01; } }\n  std::vector<mh_artic_params> p(4);\n'
                   '  for (size_t w = 0; w < p.size(); w++) { mh_artic_params_from_model(&m, &p[w]); p[w].mass[2] = 1.0 + 0.1 * (double)w; }\n  p[3].mass[1] = -1.0;\n'
                   '  std::vector<double> q(12, 0.0);\n'
                   '  try { MobyHip::BatchedArticulatedBody* r = MobyHip::BatchedArticulatedBody::with_params(m, p.data(), 4, q.data(), q.data()); r->set_params(p.data(), 0, 1); r->step(1e-3, 2); delete r; }\n'
                   '  catch (const std::exception& e) { std::printf("%s\\n", e.what()); return 3; }\n  return 0; }\n')
    exe = str(tmp_path / "pw")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "moby_amd", "cpp"), str(src), "-L" + os.path.join(ROOT, "moby_amd"),
                           "-lmoby_hip", "-Wl,-rpath," + os.path.join(ROOT, "moby_amd"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE)
    assert r.returncode == 3 and r.stdout.decode().startswith("world 3: link 1: mass"), r.stdout
