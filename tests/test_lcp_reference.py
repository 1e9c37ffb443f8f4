"""tests/lcp_reference.py proved without a GPU: the CPU oracle's solutions of known-solution problems pass assert_is_the_solution
(support, signs, forward error within n eps cond_2 max(z)) for all four solver kinds, and the padded-buffer builder round-trips."""
import numpy as np
import pytest

from tests import lcp_reference as R
from tests.oracle_api import FAST, FAST_REG, LEMKE, LEMKE_REG

KINDS = [FAST, FAST_REG, LEMKE, LEMKE_REG]


@pytest.mark.parametrize("n", [33, 63, 128, 257])
def test_oracle_returns_the_known_solution(oracle, n):
    """three active-set sizes (one variable, a sixth of them, half of them) x four kinds, cold; the largest error / bound is printed"""
    worst = 0.0
    for active in (1, max(2, n // 6), n // 2):
        M, q, idx, zs = R.known_solution_problem(n, active, seed=1000 * n + active)
        assert len(idx) == active and len(np.unique(idx)) == active
        z_ref, cond = R.refined_solution(M, q, idx)
        np.testing.assert_allclose(z_ref.astype(np.float64), zs, rtol=0, atol=n * np.finfo(float).eps * cond * zs.max())
        for kind in KINDS:
            r = oracle.lcp(kind, M, q, z_size=0 if kind in (FAST, FAST_REG) else n, rng=oracle.rand_state(1))
            assert r["ok"], (kind, n, active)
            worst = max(worst, R.assert_is_the_solution(M, q, r["z"], idx, tag="kind %d n %d active %d" % (kind, n, active)))
    print("n = %d: largest |z - z_ref| / bound of the oracle = %.4f" % (n, worst))
    assert worst < 0.1                          # (0.014 measured: a reference that drifts towards its own bound is flagged long before a solver is)


def test_a_wrong_answer_is_refused():
    """the checker itself: a perturbation of one ulp-scale multiple beyond the bound, a spurious nonzero and a missing one all fail"""
    n = 63
    M, q, idx, zs = R.known_solution_problem(n, 20, seed=5)
    z_ref, cond = R.refined_solution(M, q, idx)
    z = z_ref.astype(np.float64)
    assert R.assert_is_the_solution(M, q, z, idx) < 0.1
    bound = n * np.finfo(float).eps * cond * float(z_ref.max())
    bad = z.copy(); bad[idx[3]] += 4.0 * bound
    with pytest.raises(AssertionError):
        R.assert_is_the_solution(M, q, bad, idx)
    off = np.setdiff1d(np.arange(n), idx)
    bad = z.copy(); bad[off[0]] = 1e-300
    with pytest.raises(AssertionError):
        R.assert_is_the_solution(M, q, bad, idx)
    bad = z.copy(); bad[idx[0]] = 0.0
    with pytest.raises(AssertionError):
        R.assert_is_the_solution(M, q, bad, idx)


@pytest.mark.parametrize("n,ld,extra,base", [(6, 9, 5, 0), (6, 6, 1, 0), (7, 7, 0, 1), (42, 45, 5, 3)])
def test_padded_buffer_round_trips(n, ld, extra, base):
    B = 4
    rng = np.random.default_rng(n + ld)
    M = rng.standard_normal((B, n, n))
    stride = ld * n + extra
    for fill in (np.nan, 1e300):
        buf = R.build_buffer(M, ld, stride, base, fill)
        assert buf.shape == (R.padded_size(B, n, ld, stride, base),)
        np.testing.assert_array_equal(R.compact_from_buffer(buf, B, n, ld, stride, base), M)
        # element (r, c) of problem b sits where the header says, and everything else is fill
        b, r, c = 2, n - 1, 1
        assert buf[base + b * stride + r + ld * c] == M[b, r, c]
        pad = np.ones(buf.shape, dtype=bool)
        for b in range(B):
            for c in range(n):
                o = base + b * stride + ld * c
                pad[o:o + n] = False
        assert pad.sum() == buf.size - B * n * n and pad[-R.SLACK:].all()
        assert R.same_bits(buf[pad], np.full(int(pad.sum()), fill))
    assert R.same_bits(buf, buf.copy()) and not R.same_bits(buf, np.where(np.arange(buf.size) == 0, 2.0, buf))
