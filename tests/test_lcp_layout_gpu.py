"""The documented matrix layout of mh_lcp_solve_batch[_dev] -- "problem b at M + b*strideM, leading dimension ld >= n" -- on every
kernel family, with padding that must never be read, and the optional outputs left out.

Layouts (B = 4 problems each):
  (a) ld = n + 3, strideM = ld n + 5                 what a Ravelin sub-block view hands the C++ adapter
  (b) ld = n,     strideM = n n + 1                  even n: odd problems sit 8 bytes off a 16-byte boundary -- the wave kernel takes
                                                     its double2 loads for even b and its scalar loads for odd b in ONE launch
  (c) ld = n, the first matrix one double into the buffer (through the device entry the kernel sees that misaligned base)
Each through the host entry and through the device entry (where the padded buffer is in HBM as built, is read back afterwards and must be unchanged).
The padding holds NaN in one run and 1e300 in another: norm_inf(M) is taken with `a > m ? a : m`, which a NaN does not enter but a
large number does -- NaN padding shows up where it is used as data, 1e300 where it only reaches the tolerances."""
import numpy as np
import pytest

from moby_amd import _lib
from tests import lcp_reference as R
from tests.oracle_api import DEFAULT_EXPS, FAST, FAST_REG, LEMKE, LEMKE_REG
from tests.test_lcp_gpu import TRACE_CAP

pytestmark = pytest.mark.gpu

KINDS = [FAST, FAST_REG, LEMKE, LEMKE_REG]
LEMKES = [LEMKE, LEMKE_REG]
B = 4
FIELDS = ("status", "pivots", "trace_len", "trace", "rng", "z_size")


def layouts(n):
    return {"a": dict(ld=n + 3, strideM=(n + 3) * n + 5), "b": dict(ld=n, strideM=n * n + 1), "c": dict(ld=n, strideM=n * n, base_offset=1)}


def problems(n, active, seed):
    """B known-solution problems, active sets of `active` +- a few variables"""
    Ms, qs, idxs = [], [], []
    for b in range(B):
        M, q, idx, _ = R.known_solution_problem(n, max(1, min(n - 1, active + b - 1)), seed=seed + b)
        Ms.append(M); qs.append(q); idxs.append(idx)
    return np.array(Ms), np.array(qs), idxs


def equal_results(a, b, tag):
    for f in FIELDS:
        np.testing.assert_array_equal(a[f], b[f], err_msg="%s: %s" % (tag, f))
    good = a["status"] == 1
    np.testing.assert_array_equal(a["z"][good], b["z"][good], err_msg=tag + ": z")


def equals_oracle(res, ora, tag):
    """what tests/test_lcp_gpu.py::assert_parity asserts, on a solve_layout result and oracle results computed once"""
    for b, r in enumerate(ora):
        t = "%s problem %d" % (tag, b)
        assert bool(res["status"][b]) == r["ok"], t
        assert int(res["pivots"][b]) == r["pivots"], t
        assert int(res["trace_len"][b]) == r["trace_len"], t
        L = min(r["trace_len"], TRACE_CAP)
        np.testing.assert_array_equal(res["trace"][b, :L], r["trace"][:L], err_msg=t)
        np.testing.assert_array_equal(res["rng"][b], r["rng"], err_msg=t)
        assert int(res["z_size"][b]) == r["z_size"], t
        if r["ok"]:
            np.testing.assert_array_equal(res["z"][b], r["z"], err_msg=t)


def check_layouts(oracle, kinds, M, q, idxs, z0=None, z_size=None, compact_oracle=False):
    n = q.shape[1]
    zs = np.full(B, n, dtype=np.int32) if z_size is None else np.asarray(z_size, dtype=np.int32)
    for kind in kinds:
        exps = DEFAULT_EXPS[kind]
        if compact_oracle:
            oracle.lib.oracle_dbg_lemke_compact(8)
        try:
            ora = [oracle.lcp(kind, M[b], q[b], z=None if z0 is None else z0[b], z_size=int(zs[b]), rng=oracle.rand_state(1), exps=exps, trace_cap=TRACE_CAP)
                   for b in range(B)]
        finally:
            oracle.lib.oracle_dbg_lemke_compact(0)
        assert all(r["ok"] for r in ora)
        kw = dict(z0=z0, z_size=zs, exps=exps, trace_cap=TRACE_CAP)
        compact = R.solve_layout(kind, M, q, **kw)
        equals_oracle(compact, ora, "kind %d n %d compact" % (kind, n))
        for b in range(B):
            R.assert_is_the_solution(M[b], q[b], compact["z"][b], idxs[b], tag="kind %d n %d problem %d" % (kind, n, b))
        for name, lay in layouts(n).items():
            for device in (False, True):
                for fill in (np.nan, 1e300):
                    tag = "kind %d n %d layout %s %s fill %r" % (kind, n, name, "device" if device else "host", fill)
                    res = R.solve_layout(kind, M, q, fill=fill, device=device, **lay, **kw)
                    equals_oracle(res, ora, tag)
                    equal_results(res, compact, tag)
                    if device:          # (the host entry works on a device copy of its own and never writes M back: nothing to see there)
                        assert R.same_bits(res["buffer"], res["buffer_before"]), tag + ": the matrix buffer changed"


@pytest.mark.parametrize("n", [6, 42, 64])
def test_wave_kernel(oracle, n):
    """even n: the double2 path needs ld == n, a 16-byte-aligned matrix and an even n n; (a) fails the first, odd problems of (b) and
    every problem of (c) on the device entry fail the second"""
    M, q, idxs = problems(n, n // 3, seed=10 * n)
    check_layouts(oracle, KINDS, M, q, idxs, z_size=np.zeros(B, dtype=np.int32))


def test_blk_256_threads(oracle):
    M, q, idxs = problems(100, 12, seed=100)
    try:
        _lib.check(_lib.load().mh_debug_set(2, 1))
        check_layouts(oracle, KINDS, M, q, idxs, z_size=np.zeros(B, dtype=np.int32))
    finally:
        _lib.check(_lib.load().mh_debug_set(2, 0))


def test_blkw_1024_threads_cold(oracle):
    M, q, idxs = problems(200, 12, seed=200)
    try:
        _lib.check(_lib.load().mh_debug_set(2, 2))
        check_layouts(oracle, KINDS, M, q, idxs, z_size=np.zeros(B, dtype=np.int32))
    finally:
        _lib.check(_lib.load().mh_debug_set(2, 0))


def test_blkw_register_lu_warm(oracle):
    """n = 400, a warm lcp_fast whose nonbasic block has about 100 rows: gathered from M into the registers of the sixteen waves
    (mh_lu_reg.inc) through Mat::at"""
    n = 400
    M, q, idxs = problems(n, 100, seed=400)
    z0 = np.zeros((B, n))
    for b in range(B):
        z0[b, idxs[b]] = 1.0 + 1e-3 * np.random.default_rng(b).standard_normal(len(idxs[b]))
    try:
        _lib.check(_lib.load().mh_debug_set(2, 2))
        check_layouts(oracle, [FAST, FAST_REG], M, q, idxs, z0=z0)
    finally:
        _lib.check(_lib.load().mh_debug_set(2, 0))


@pytest.mark.parametrize("geometry", [3, 4])
def test_blk1_blk2_one_and_two_waves(oracle, geometry):
    M, q, idxs = problems(130, 10, seed=130 + geometry)
    try:
        _lib.check(_lib.load().mh_debug_set(2, geometry))
        check_layouts(oracle, LEMKES, M, q, idxs, z_size=np.array([130, 0, 130, 0], dtype=np.int32))
    finally:
        _lib.check(_lib.load().mh_debug_set(2, 0))


def test_blky_four_rows_per_lane(oracle):
    M, q, idxs = problems(513, 16, seed=513)
    try:
        _lib.check(_lib.load().mh_debug_set(2, 5))
        check_layouts(oracle, LEMKES, M, q, idxs, z_size=np.array([513, 0, 513, 0], dtype=np.int32), compact_oracle=True)
    finally:
        _lib.check(_lib.load().mh_debug_set(2, 0))


def test_blkx_two_rows_per_lane(oracle):
    M, q, idxs = problems(1025, 12, seed=1025)
    check_layouts(oracle, LEMKES, M, q, idxs, z_size=np.array([1025, 0, 1025, 0], dtype=np.int32), compact_oracle=True)


@pytest.mark.parametrize("n,geometry", [(42, 0), (100, 1)])
def test_optional_outputs_left_out(n, geometry):
    """z_size_in (warm z given), z_size_out, pivots, trace, trace_len NULL in turn, then all of them: status, z and rng as in the full call"""
    M, q, idxs = problems(n, n // 4, seed=7 * n)
    z0 = np.zeros((B, n))
    for b in range(B):
        z0[b, idxs[b]] = 1.0 + 1e-3 * np.random.default_rng(b).standard_normal(len(idxs[b]))
        z0[b, (idxs[b][0] + 1) % n] += 0.5                     # one variable that does not belong: a few pivots, not none
    try:
        _lib.check(_lib.load().mh_debug_set(2, geometry))
        for kind in KINDS:
            for device in (False, True):
                kw = dict(z0=z0, exps=DEFAULT_EXPS[kind], device=device, ld=n + 3, strideM=(n + 3) * n + 5)
                full = R.solve_layout(kind, M, q, **kw)
                assert (full["status"] == 1).all()
                for b in range(B):
                    R.assert_is_the_solution(M[b], q[b], full["z"][b], idxs[b])
                for leave in [(o,) for o in R.OPTIONAL] + [R.OPTIONAL]:
                    want = tuple(o for o in R.OPTIONAL if o not in leave)
                    res = R.solve_layout(kind, M, q, want=want, **kw)
                    tag = "kind %d n %d %s without %s" % (kind, n, "device" if device else "host", leave)
                    for f in ("status", "z", "rng"):
                        np.testing.assert_array_equal(res[f], full[f], err_msg=tag + ": " + f)
                    for f in ("pivots", "trace", "trace_len", "z_size"):
                        if res[f] is not None:
                            np.testing.assert_array_equal(res[f], full[f], err_msg=tag + ": " + f)
    finally:
        _lib.check(_lib.load().mh_debug_set(2, 0))


@pytest.mark.parametrize("n", [42, 100])
def test_device_entry_on_a_side_stream(n):
    """LCPDevice.solve on a non-default torch stream, no trace: the host entry's result bit for bit"""
    import torch
    from moby_amd.lcp import LCPDevice
    M, q, idxs = problems(n, n // 4, seed=3 * n)
    zs = np.zeros(B, dtype=np.int32)
    for kind in KINDS:
        host = R.solve_layout(kind, M, q, z_size=zs, exps=DEFAULT_EXPS[kind])
        assert (host["status"] == 1).all()
        dev = LCPDevice(B)
        Md = torch.from_numpy(np.ascontiguousarray(np.transpose(M, (0, 2, 1)))).cuda()
        qd = torch.from_numpy(q).cuda(); zd = torch.zeros((B, n), dtype=torch.float64, device="cuda"); zsd = torch.from_numpy(zs).cuda()
        opts = _lib.mh_lcp_opts(*[int(e) for e in DEFAULT_EXPS[kind]], -1.0, -1.0)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            st = dev.solve(kind, Md, qd, zd, opts=opts, z_size_in=zsd)
        side.synchronize()
        tag = "kind %d n %d" % (kind, n)
        np.testing.assert_array_equal(st.cpu().numpy(), host["status"], err_msg=tag)
        np.testing.assert_array_equal(zd.cpu().numpy(), host["z"], err_msg=tag)
        np.testing.assert_array_equal(dev.rng.cpu().numpy().view(np.uint32), host["rng"], err_msg=tag)
        np.testing.assert_array_equal(dev.pivots.cpu().numpy().view(np.uint32), host["pivots"], err_msg=tag)
        np.testing.assert_array_equal(dev.z_size.cpu().numpy(), host["z_size"], err_msg=tag)
        for b in range(B):
            R.assert_is_the_solution(M[b], q[b], zd[b].cpu().numpy(), idxs[b], tag=tag)
