"""World level: the sphere-stack batch through the one-wavefront kernel, whose lcp_fast skips rand_min reductions that decide nothing
(but consumes their draws), against the oracle's world_step_batch over a window in which the chain also falls through to lcp_lemke:
states, every aux counter and the rand() ring, bit for bit."""
import ctypes

import numpy as np
import pytest

from moby_amd import scene as S
from moby_amd.world import WorldBatch

pytestmark = pytest.mark.gpu

FIELDS = ("rng", "time", "status", "steps", "mini_steps", "lcp_solves", "lcp_rows", "lcp_pivots", "stab_iters", "stab_rows", "zlast_size", "zbuf_size")


def _lu_hist(oracle):
    h = np.zeros(130, dtype=np.uint64)
    oracle.lib.oracle_dbg_lu_hist(h.ctypes.data_as(ctypes.c_void_p))
    return h.astype(np.int64)


def test_sphere_stacks_64_worlds_260_steps_with_lemke_solves(oracle):
    """worlds 0..63 from t = 0: in the oracle all 64 of them reach lcp_lemke within the 260 steps (354 bases of 42 rows when this test was
    written); the assertion below only needs one"""
    B, nsteps = 64, 260
    sc = S.sphere_stack_scene()
    st0 = S.sphere_stack_state_range(0, B)
    wb = WorldBatch(sc, st0.copy())
    wb.step(1e-3, nsteps)
    st_o = st0.copy().reshape(B, -1); aux_o = S.new_aux(B)
    h0 = _lu_hist(oracle)
    oracle.world_step_batch(sc, st_o, aux_o, 1e-3, nsteps)
    lemke_bases = (_lu_hist(oracle) - h0)[65:]                 # [65 + n]: bases of n rows factorised by lcp_lemke
    assert lemke_bases.sum() >= 1 and lemke_bases[42] >= 1
    np.testing.assert_array_equal(np.asarray(wb.state).reshape(B, -1), st_o)
    for f in FIELDS:
        np.testing.assert_array_equal(wb.aux[f], aux_o[f], err_msg=f)
