"""Episodes on the device (include/moby_hip_artic.h, "Episodes on the device") without a GPU: the coverage of the cases of tests/artic_reset_ref.py,
proven on the reference alone so that tests/test_artic_reset_gpu.py cannot pass vacuously; the fresh aux record; the refusals that need no device;
the example."""
import os
import subprocess

import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import artic as A
from moby_amd import scene as S
from tests import artic_params_ref as P
from tests import artic_report_ref as R
from tests import artic_reset_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MH_ERR_INVALID_ARG = -1


@pytest.fixture(scope="module")
def ref():
    return R.build_report_ref()


@pytest.mark.parametrize("case", E.CASES, ids=P.case_id)
def test_gpu_cases_keep_their_point(ref, case):
    """on the reference alone: every reset world ends elsewhere than in the uninterrupted two-launch run, every other world ends exactly there, every
    reset world solves an LCP after its reset (its warm starts and rand() stream matter), and the mixed case resets worlds on both sides of mu = 100"""
    m, q0, qd0, dt, n, p, pose0, out, after = E.reset_run(ref, case)
    keep = P.reference_run(ref, case)[-1]
    worlds = E.mask_of(case)[1]
    assert len(E.CASES) == 4 and len(worlds) == 3 and (worlds == (1, 3, 4) or case[0] == "floating_box_pendulum")
    for launch in range(2):
        a, b = out[launch], keep[launch]
        for w in range(E.B):
            same = (np.array_equal(a["q"][w], b["q"][w]) and np.array_equal(a["qd"][w], b["qd"][w]) and a["aux"][w].tobytes() == b["aux"][w].tobytes()
                    and np.array_equal(a["report"][w], b["report"][w]) and (a["pose"] is None or np.array_equal(a["pose"][w], b["pose"][w])))
            if launch == 0 or w not in worlds:
                assert same, (launch, w)                                   # not reset: the uninterrupted run, bit for bit
            else:
                assert not (np.array_equal(a["q"][w], b["q"][w]) and np.array_equal(a["qd"][w], b["qd"][w])), w   # (the aux record differs anyway: the clock)
    for w in worlds:
        assert after["aux"][w].tobytes() == S.new_aux(1)[0].tobytes()
        assert out[1]["aux"]["lcp_solves"][w] > 0 and out[1]["aux"]["steps"][w] == n and out[1]["aux"]["status"][w] & S.MH_WORLD_LCP_FAILED == 0, w
    if case[4] is P.MIXED:
        mu = p["cp_mu_coulomb"][list(worlds)]
        assert (mu < 100.0).any() and (mu >= 100.0).any()


def test_the_box_family_case_keeps_its_point(ref):
    """four_feet with the stabiliser on the reference alone: a model with boxes only (a plain batch of it steps through the box kernels), and every
    reset world solves LCPs and runs stabiliser iterations after its reset -- the rows the box family keeps in the batch's workspace are in use"""
    m, q0, qd0, dt, n, out = E.box_family_run(ref)
    assert m.nboxes > 0 and m.nspheres == 0 and m.npairs == 0 and m.sphere_no_plane == 0 and all(m.box_link[k] >= 0 for k in range(m.nboxes)) and m.cstab_max_iterations > 0
    for w in E.RESET_WORLDS:
        a = out[1]["aux"][w]
        assert a["steps"] == n and a["lcp_solves"] > 0 and a["stab_iters"] > 0 and a["status"] & S.MH_WORLD_LCP_FAILED == 0, w
    assert (out[0]["aux"]["stab_iters"] > 0).any() and (out[1]["aux"]["steps"][[0, 2]] == 2 * n).all()


def test_the_fresh_record_is_the_librarys():
    """S.new_aux(1), what the reference resets a world's record to, is what mh_world_aux_init(&a, 1) writes -- the record of a freshly created batch
    and of a reset world -- byte for byte"""
    a = np.full(1, 0xff, dtype=np.uint8).repeat(S.AUX_DTYPE.itemsize).view(S.AUX_DTYPE)
    _lib.load().mh_world_aux_init(a.ctypes.data, 1)
    assert a.tobytes() == S.new_aux(1).tobytes() and S.AUX_DTYPE.itemsize == 1376 and S.AUX_DTYPE.itemsize % 8 == 0


def test_refusals_that_need_no_device():
    """a null batch for all three calls (before the device is looked for); a mask that is not int32 is refused in Python with the way out"""
    lib = _lib.load()
    buf = np.zeros(64)
    p = buf.ctypes.data
    for call in (lambda: lib.mh_artic_batch_reset_dev(None, None, p, p, p, None), lambda: lib.mh_artic_batch_reset_dev(None, None, None, None, None, None),
                 lambda: lib.mh_artic_batch_status_dev(None, None, p, p), lambda: lib.mh_artic_batch_link_poses_dev(None, None, p)):
        assert call() == MH_ERR_INVALID_ARG and "null batch" in lib.mh_last_error().decode()
    import torch
    ab = object.__new__(A.ArticBatch)                                    # no handle: the mask is refused before anything is looked up
    ab.B, ab.nj, ab.handle = 6, 3, None
    for bad in (torch.zeros(6, dtype=torch.float64), torch.zeros(6, dtype=torch.bool), torch.zeros(6, dtype=torch.int64), np.zeros(6, dtype=np.int32)):
        with pytest.raises(ValueError, match="convert"):
            ab.reset(mask=bad)


def test_cpp_example_compiles_and_fails_loudly_without_a_gpu(tmp_path):
    """example_artic_reset.cpp (link_poses_dev, a kernel of its own that marks the fallen copies, reset_dev, status_dev): the example builds; without
    a device it reports the error (no fallback), with one it runs to its end -- some copies are reset, their clocks restart, every status is 0"""
    import torch
    cpp = os.path.join(ROOT, "moby_amd", "cpp")
    exe = str(tmp_path / "example_artic_reset")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-Wall", os.path.join(cpp, "example_artic_reset.cpp"), "-L" + os.path.join(ROOT, "moby_amd"),
                           "-lmoby_hip", "-Wl,-rpath," + os.path.join(ROOT, "moby_amd"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, timeout=120)
    if torch.cuda.is_available():
        assert p.returncode == 0 and b"reset, status 0, time 0.000" in p.stdout and b"goes on, status 0" in p.stdout, p.stdout
    else:
        assert p.returncode == 1 and b"no HIP device" in p.stdout, p.stdout
