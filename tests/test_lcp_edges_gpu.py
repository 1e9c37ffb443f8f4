"""The LCP entry at the sizes where its thread geometries change hands: half- and full-wave boundaries of the one-wavefront solver
(31, 32, 33, 63), n = T and T + 1 of the 128- / 256-thread block solvers, the `wide` switch (192, 384), the narrow caps (511, 512),
1023, 2047, the first size past the two-rows-per-lane LU (2049) and nonbasic blocks of exactly 1023 / 1024 / 1025 rows.

Every problem is tests/lcp_reference.py's known-solution problem: dense, positive definite, the active set scattered over the index
range.  Wherever the oracle is cheap the run equals it bit for bit (assert_parity), every accepted z is THE solution
(assert_is_the_solution: support, signs of w, forward error within n eps cond_2 max z), and the geometries that can run one size agree
with each other in z, pivots, rand() state and trace.  Each check prints `lcp-ratio` = error / bound (pytest -s shows them)."""
import numpy as np
import pytest

from moby_amd import _lib
from tests import lcp_reference as R
from tests.oracle_api import FAST, FAST_REG, LEMKE, LEMKE_REG
from tests.test_lcp_gpu import assert_parity, run_gpu

pytestmark = pytest.mark.gpu

KINDS = [FAST, FAST_REG, LEMKE, LEMKE_REG]


def batch(n, actives, seed):
    Ms, qs, idxs, zss = [], [], [], []
    for b, a in enumerate(actives):
        M, q, idx, zs = R.known_solution_problem(n, a, seed=seed + 17 * b)
        Ms.append(M); qs.append(q); idxs.append(idx); zss.append(zs)
    return np.array(Ms), np.array(qs), idxs, np.array(zss)


def perturbed(zss, seed):
    """z* with its positive entries moved by a relative 1e-3: the same nonbasic set, other values"""
    return zss * (1.0 + 1e-3 * np.random.default_rng(seed).standard_normal(zss.shape))


def known(M, q, idxs, ok, z, tag):
    assert ok.all(), tag
    worst = 0.0
    for b in range(len(idxs)):
        worst = max(worst, R.assert_is_the_solution(M[b], q[b], z[b], idxs[b], tag="%s problem %d" % (tag, b)))
    print("lcp-ratio %.4f %s" % (worst, tag))
    return worst


def same_run(a, b, tag):
    """two run_gpu results: status, z, pivots, rand() state, trace and its length, z.size()"""
    np.testing.assert_array_equal(a[0], b[0], err_msg=tag + ": status")
    np.testing.assert_array_equal(a[1], b[1], err_msg=tag + ": z")
    for f in ("pivots", "rng", "trace_len", "trace", "z_size"):
        np.testing.assert_array_equal(getattr(a[2], f), getattr(b[2], f), err_msg="%s: %s" % (tag, f))


def across_geometries(oracle, key, geometries, kind, M, q, idxs, tag, compact_oracle=False, **kw):
    """parity with the oracle under the first geometry (the oracle runs once), the known solution and bit-equality with that run under every one"""
    lib = _lib.load()
    first = None
    try:
        for g in geometries:
            _lib.check(lib.mh_debug_set(key, g))
            if first is None:
                if compact_oracle:
                    oracle.lib.oracle_dbg_lemke_compact(8)
                try:
                    assert_parity(oracle, kind, M, q, **kw)
                finally:
                    oracle.lib.oracle_dbg_lemke_compact(0)
            r = run_gpu(kind, M, q, kw.get("z0"), kw.get("z_size"))
            t = "%s key %d = %d" % (tag, key, g)
            known(M, q, idxs, r[0], r[1], t)
            if first is None:
                first = r
            else:
                same_run(r, first, t)
    finally:
        _lib.check(lib.mh_debug_set(key, 0))
    return first


# ---- one wavefront per problem -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [31, 32, 33, 63])
def test_wave_solver_at_the_ballot_mask_edges(oracle, kind, n):
    actives = [1, n // 2, n - 1]
    M, q, idxs, zss = batch(n, actives, seed=100 * n)
    tag = "wave kind %d n %d" % (kind, n)
    zs = np.zeros(3, dtype=np.int32)
    assert_parity(oracle, kind, M, q, z_size=zs)
    ok, z, _ = run_gpu(kind, M, q, z_size=zs)
    known(M, q, idxs, ok, z, tag + " cold")
    z0 = perturbed(zss, n)
    assert_parity(oracle, kind, M, q, z0=z0)
    ok, z, _ = run_gpu(kind, M, q, z0=z0)
    known(M, q, idxs, ok, z, tag + " warm")


# ---- the lcp_fast kinds on the block solver ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385, 511, 512])
def test_lcp_fast_kinds_at_the_block_geometry_edges(oracle, n):
    """automatic geometry, 256 threads (key 8 = 1) and 1024 threads (key 8 = 2): cold with 16 active variables, warm with n - 3
    (n < 192 warm under key 8 = 2: the register LU's U, k columns of 192 doubles, does not fit the n x n workspace area -- lcp_fast must
    send such a system through the workspace; n = 127 with 124 rows wrote past the allocation before it did)"""
    for kind in (FAST, FAST_REG):
        M, q, idxs, _ = batch(n, [16, 16], seed=3 * n + kind)
        across_geometries(oracle, 8, (0, 1, 2), kind, M, q, idxs, "fast kind %d n %d cold" % (kind, n), z_size=np.zeros(2, dtype=np.int32))
        M, q, idxs, zss = batch(n, [n - 3, n - 3], seed=5 * n + kind)
        across_geometries(oracle, 8, (0, 1, 2), kind, M, q, idxs, "fast kind %d n %d warm" % (kind, n), z0=perturbed(zss, n))


# ---- the lcp_lemke kinds -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [LEMKE, LEMKE_REG])
@pytest.mark.parametrize("n", [128, 129, 256, 257, 511, 512])
def test_lemke_kinds_on_the_four_geometries_up_to_512_rows(oracle, kind, n):
    """key 2 = 1 .. 4: 256, 1024, 64 and 128 threads per problem; problem 1 enters with z.size() = 0 and draws n rand() values"""
    M, q, idxs, _ = batch(n, [16, 16], seed=7 * n + kind)
    across_geometries(oracle, 2, (1, 2, 3, 4), kind, M, q, idxs, "lemke kind %d n %d" % (kind, n), z_size=np.array([n, 0], dtype=np.int32))


@pytest.mark.parametrize("kind", [LEMKE, LEMKE_REG])
def test_lemke_kinds_at_1023_rows(oracle, kind):
    """one below the compact cap of the 1024-thread geometry (key 2 = 2) and of the four-rows-per-lane geometry (key 2 = 5)"""
    n = 1023
    M, q, idxs, _ = batch(n, [16, 16], seed=7 * n + kind)
    across_geometries(oracle, 2, (2, 5), kind, M, q, idxs, "lemke kind %d n %d" % (kind, n), compact_oracle=True, z_size=np.array([n, 0], dtype=np.int32))


@pytest.mark.parametrize("kind", [LEMKE, LEMKE_REG])
def test_lemke_kinds_at_2047_rows(kind):
    """the two-rows-per-lane LU one row below its largest size: the known solution (the oracle is not asked)"""
    n = 2047
    M, q, idxs, _ = batch(n, [16, 16], seed=7 * n + kind)
    ok, z, lcp = run_gpu(kind, M, q, z_size=np.array([n, 0], dtype=np.int32))
    known(M, q, idxs, ok, z, "lemke kind %d n %d" % (kind, n))
    assert (lcp.pivots >= 16).all()


# ---- beyond what the oracle finishes in seconds --------------------------------------------------------------------------------
def twice(n, active, seed):
    M, q, idx, zs = R.known_solution_problem(n, active, seed)
    return np.array([M, M]), np.array([q, q]), [idx, idx], np.array([zs, zs])


def test_lemke_past_the_two_rows_per_lane_lu():
    """n = 2049 = MH_BLKX_MAX_N + 1: back on the 1024-thread geometry with the dense dgesv for every basis"""
    n = 2049
    M, q, idxs, _ = twice(n, 6, seed=n)
    ok, z, lcp = run_gpu(LEMKE, M, q, z_size=np.array([n, n], dtype=np.int32))
    known(M, q, idxs, ok, z, "lemke n %d" % n)
    np.testing.assert_array_equal(z[0], z[1])
    np.testing.assert_array_equal(lcp.pivots[0], lcp.pivots[1]); np.testing.assert_array_equal(lcp.rng[0], lcp.rng[1])
    assert (lcp.pivots >= 6).all()


@pytest.mark.parametrize("k", [1023, 1024, 1025])
def test_lcp_fast_nonbasic_block_at_the_lds_caps(k):
    """n = 1100, warm: the nonbasic index list and the right-hand side of exactly k rows -- the last two sizes that fit the LDS staging
    (LIST_CAP / RHS_CAP = 1024) and the first that lives in the workspace"""
    n = 1100
    M, q, idxs, zss = twice(n, k, seed=k)
    for kind in (FAST, FAST_REG):
        ok, z, lcp = run_gpu(kind, M, q, z0=perturbed(zss[:1], k).repeat(2, axis=0))
        known(M, q, idxs, ok, z, "fast kind %d n %d nonbasic %d" % (kind, n, k))
        np.testing.assert_array_equal(z[0], z[1])
        np.testing.assert_array_equal(lcp.pivots[0], lcp.pivots[1]); np.testing.assert_array_equal(lcp.rng[0], lcp.rng[1])
