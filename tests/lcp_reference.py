"""Helpers of the LCP entry tests that share no code with the oracle and need no GPU to import.

  known_solution_problem   a dense positive-definite LCP whose solution is known before any solver runs
  refined_solution         that solution to (nearly) working precision: LAPACK plus iterative refinement with long-double residuals
  assert_is_the_solution   a solver's z IS that solution: support, signs of w, forward error within the first-order bound
  solve_layout             mh_lcp_solve_batch[_dev] through ctypes with M in a padded column-major buffer (ld, strideM, base offset)

For a positive-definite M the LCP has exactly one solution, so whatever pivots a solver took, on whatever thread geometry, a status
of 1 obliges it to return this one."""
import ctypes

import numpy as np

SLACK = 64                                  # doubles of `fill` behind the last matrix of a padded buffer: a full wave's load past the last column stays inside
OPTIONAL = ("z_size_in", "z_size_out", "pivots", "trace", "trace_len")


def known_solution_problem(n, active, seed):
    """M = A A'/n + I (dense, PD); `active` indices idx drawn at random (NOT a prefix: a prefix hides index-mapping errors);
    z* uniform in [0.5, 2] on idx and 0 elsewhere, w* uniform in [0.5, 2] off idx and 0 on it; q = w* - M z*.
    Returns (M, q, idx (sorted), z*)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    M = A @ A.T / n + np.eye(n)
    idx = np.sort(rng.choice(n, size=active, replace=False))
    zs = np.zeros(n); zs[idx] = rng.uniform(0.5, 2.0, active)
    ws = rng.uniform(0.5, 2.0, n); ws[idx] = 0.0
    return M, ws - M @ zs, idx, zs


def refined_solution(M, q, idx):
    """z_ref (n long doubles, zero off idx) with M[idx, idx] z_ref[idx] = -q[idx]: np.linalg.solve and three steps of iterative
    refinement whose residuals are evaluated in np.longdouble; and cond_2(M[idx, idx])."""
    n = len(q)
    A = np.ascontiguousarray(M[np.ix_(idx, idx)])
    Al = A.astype(np.longdouble); rhs = -np.asarray(q)[idx].astype(np.longdouble)
    x = np.linalg.solve(A, rhs.astype(np.float64)).astype(np.longdouble)
    for _ in range(3):
        r = rhs - Al @ x
        x = x + np.linalg.solve(A, r.astype(np.float64)).astype(np.longdouble)
    z = np.zeros(n, dtype=np.longdouble); z[idx] = x
    return z, float(np.linalg.cond(A, 2))


def assert_is_the_solution(M, q, z, idx, tag=""):
    """z is the solution of the PD problem (M, q) whose positive variables are idx:
      - z >= 0, and its nonzero support is idx exactly (the solvers leave exact zeros off the basis);
      - w = M z + q, evaluated in long double, is positive off idx;
      - max |z - z_ref| <= n eps cond_2(M[idx, idx]) max(z_ref): the first-order forward-error bound of a backward-stable solve
        with the unit constant.
    Returns error / bound."""
    n = len(q)
    z = np.asarray(z, dtype=np.float64)
    assert z.shape == (n,), tag
    assert not np.isnan(z).any() and (z >= 0.0).all(), tag
    np.testing.assert_array_equal(np.flatnonzero(z != 0.0), np.asarray(idx), err_msg="support " + tag)
    w = np.asarray(M).astype(np.longdouble) @ z.astype(np.longdouble) + np.asarray(q).astype(np.longdouble)
    off = np.ones(n, dtype=bool); off[idx] = False
    assert (w[off] > 0).all(), tag
    z_ref, cond = refined_solution(M, q, idx)
    bound = n * np.finfo(np.float64).eps * cond * float(z_ref.max())
    err = float(np.abs(z.astype(np.longdouble) - z_ref).max())
    assert err <= bound, "%s: |z - z_ref| = %.3e > %.3e (cond %.2f)" % (tag, err, bound, cond)
    return err / bound


# ---- padded layouts -----------------------------------------------------------------------------------------------------------
def padded_size(B, n, ld, strideM, base_offset=0):
    return base_offset + (B - 1) * strideM + ld * (n - 1) + n + SLACK


def build_buffer(M, ld, strideM, base_offset=0, fill=np.nan):
    """M (B, n, n), M[b][r, c]  ->  doubles with M_b(r, c) at base_offset + b strideM + r + ld c, `fill` everywhere else (the
    rows n .. ld-1 of each column, the gap up to strideM, the base offset and SLACK doubles behind the last matrix)."""
    M = np.asarray(M, dtype=np.float64)
    B, n, _ = M.shape
    assert ld >= n and (B == 1 or strideM >= ld * (n - 1) + n)
    buf = np.full(padded_size(B, n, ld, strideM, base_offset), fill, dtype=np.float64)
    for b in range(B):
        for c in range(n):
            o = base_offset + b * strideM + ld * c
            buf[o:o + n] = M[b][:, c]
    return buf


def compact_from_buffer(buf, B, n, ld, strideM, base_offset=0):
    """the inverse of build_buffer: (B, n, n) with [b][r, c]"""
    M = np.empty((B, n, n))
    for b in range(B):
        for c in range(n):
            o = base_offset + b * strideM + ld * c
            M[b][:, c] = buf[o:o + n]
    return M


def same_bits(a, b):
    """equality of two double arrays that may hold NaNs"""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def solve_layout(kind, M, q, *, ld=None, strideM=None, base_offset=0, fill=np.nan, z0=None, z_size=None, seed=1, exps=None,
                 want=OPTIONAL, trace_cap=2048, device=False, stream=None):
    """One call of mh_lcp_solve_batch (device=False: host pointers) or mh_lcp_solve_batch_dev (device=True: the padded buffer
    lives in HBM as built, base offset and slack included, and is read back after the call) on M (B, n, n) laid out by
    build_buffer.  z_size: ints (B,) or None (= n everywhere).  Every optional argument of the entry that is not named in `want`
    is passed as NULL ("z_size_in" left out means z.size() == n for every problem, whatever z_size says).
    Returns dict(status, z, rng, pivots, z_size, trace, trace_len, buffer); what was not wanted is None."""
    from moby_amd import _lib
    from moby_amd.lcp import rand_states
    lib = _lib.load()
    M = np.asarray(M, dtype=np.float64)
    q = np.ascontiguousarray(q, dtype=np.float64)
    B, n = q.shape
    ld = n if ld is None else int(ld)
    strideM = ld * n if strideM is None else int(strideM)
    buf = build_buffer(M, ld, strideM, base_offset, fill)
    before = buf.copy()
    z = np.zeros((B, n)) if z0 is None else np.array(z0, dtype=np.float64)
    rng = rand_states(B, seed)
    status = np.full(B, -1, dtype=np.int32)
    zs_in = (np.full(B, n, dtype=np.int32) if z_size is None else np.ascontiguousarray(z_size, dtype=np.int32)) if "z_size_in" in want else None
    zs_out = np.full(B, -1, dtype=np.int32) if "z_size_out" in want else None
    piv = np.zeros(B, dtype=np.uint32) if "pivots" in want else None
    tr = np.zeros((B, trace_cap), dtype=np.int32) if "trace" in want else None
    tl = np.full(B, -1, dtype=np.int32) if "trace_len" in want else None
    opts = None
    if exps is not None:
        opts = _lib.mh_lcp_opts(int(exps[0]), int(exps[1]), int(exps[2]), -1.0, -1.0)
    po = ctypes.byref(opts) if opts is not None else None
    cap = trace_cap if tr is not None else 0
    if not device:
        P = lambda a: None if a is None else a.ctypes.data
        rc = lib.mh_lcp_solve_batch(kind, B, n, buf.ctypes.data + 8 * base_offset, ld, strideM, q.ctypes.data, z.ctypes.data,
                                    P(zs_in), P(zs_out), rng.ctypes.data, status.ctypes.data, P(piv), P(tr), cap, P(tl), po)
        _lib.check(rc)
        after = buf
    else:
        import torch
        dev = torch.device("cuda")
        up = lambda a: None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)
        d = dict(buf=up(buf), q=up(q), z=up(z), zi=up(zs_in), zo=up(zs_out), rng=up(rng), st=up(status), piv=up(piv), tr=up(tr), tl=up(tl))
        P = lambda t: None if t is None else t.data_ptr()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            s = torch.cuda.current_stream().cuda_stream
            rc = lib.mh_lcp_solve_batch_dev(s, kind, B, n, d["buf"].data_ptr() + 8 * base_offset, ld, strideM, P(d["q"]), P(d["z"]),
                                            P(d["zi"]), P(d["zo"]), P(d["rng"]), P(d["st"]), P(d["piv"]), P(d["tr"]), cap, P(d["tl"]), po)
        _lib.check(rc)
        torch.cuda.synchronize()
        dn = lambda t, like: None if t is None else t.cpu().numpy().view(like.dtype).reshape(like.shape)
        after = dn(d["buf"], buf); z = dn(d["z"], z); rng = dn(d["rng"], rng); status = dn(d["st"], status)
        zs_out = dn(d["zo"], zs_out); piv = dn(d["piv"], piv); tr = dn(d["tr"], tr); tl = dn(d["tl"], tl)
    return dict(status=status, z=z, rng=rng, pivots=piv, z_size=zs_out, trace=tr, trace_len=tl, buffer=after, buffer_before=before)
