"""The device-side counter reduction (mh::world_red::k_counters behind mh_world_batch_counters_dev, mh_world.hip): the batch's solver records reduced
to an 8-element SUM and an 8-element MAX vector in device memory, against numpy uint64 sums and maxima of the same fields.  Nothing is stepped: the aux
records are crafted and uploaded.  Sizes: one wave, the wave boundary, one block, the block boundary (257: two blocks), four blocks, and one size past
1024 blocks of 256, where the grid-stride loop takes a second trip."""
import ctypes

import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import scene as S
from moby_amd.world import WorldBatchDevice

pytestmark = pytest.mark.gpu

MH_COUNTERS = 8
FIELDS = ["steps", "lcp_rows", "lcp_pivots", None, "lcp_solves", "mini_steps", "stab_iters", "lcp_alg_bytes"]      # None: the failed-world count
STATUSES = [0, S.MH_WORLD_IMPACT_TOL, S.MH_WORLD_LCP_FAILED, S.MH_WORLD_IMPACT_TOL | S.MH_WORLD_STALLED, S.MH_WORLD_UNSUPPORTED]


def crafted_aux(B):
    """B records with seeded counters up to 2^40 (lcp_alg_bytes up to 2^50), scaled down where B of them would pass 2^64; the maximum of each counter
    sits in a world of its own where B allows: world 0, world B - 1, a world in lanes 64-255 of the first block, one in the middle of the last block, ..."""
    rng = np.random.RandomState(B % 65521)
    aux = S.new_aux(B)
    aux["zlast"][:] = rng.uniform(-1.0, 1.0, size=(B, 1))        # (fields the reduction must not read as counters)
    aux["time"] = 1e6
    aux["stab_rows"] = rng.randint(1, 2 ** 62, size=B, dtype=np.int64).astype(np.uint64)
    aux["status"] = np.array(STATUSES, dtype=np.int32)[rng.randint(0, len(STATUSES), size=B)]
    last = (B - 1) // 256 * 256
    spots = []
    for s in [0, B - 1, 101 % B, last + (B - 1 - last) // 2, B // 2, B // 3, (2 * B) // 3]:
        while B >= 7 and s in spots:                             # (257: the last block IS world B - 1)
            s = (s + 1) % B
        spots.append(s)
    k = 0
    for f in FIELDS:
        if f is None:
            continue
        limit = min(2 ** (50 if f == "lcp_alg_bytes" else 40), 2 ** 63 // B)
        v = rng.randint(0, limit // 2, size=B, dtype=np.int64).astype(np.uint64)
        v[spots[k]] = limit - 1 - k
        aux[f] = v
        k += 1
    return aux


def expected(aux):
    failed = ((aux["status"] & ~np.int32(S.MH_WORLD_IMPACT_TOL)) != 0).astype(np.uint64)
    cols = [failed if f is None else aux[f].astype(np.uint64) for f in FIELDS]
    for c in cols:
        assert int(c.astype(object).sum()) < 2 ** 64            # the exact sum fits: no wrap-around on either side
    return np.array([c.sum(dtype=np.uint64) for c in cols], dtype=np.uint64), np.array([c.max() for c in cols], dtype=np.uint64)


def reduce_on_device(dev, buf, stream=None):
    """the entry into buf[0:8] (SUM) and buf[8:16] (MAX) -> the two vectors as numpy uint64"""
    import torch
    ptr = buf.data_ptr()
    if stream is None:
        _lib.check(_lib.load().mh_world_batch_counters_dev(dev.handle, None, ctypes.c_void_p(ptr), ctypes.c_void_p(ptr + 8 * MH_COUNTERS)))
        torch.cuda.synchronize()
    else:
        _lib.check(_lib.load().mh_world_batch_counters_dev(dev.handle, ctypes.c_void_p(stream.cuda_stream), ctypes.c_void_p(ptr), ctypes.c_void_p(ptr + 8 * MH_COUNTERS)))
        stream.synchronize()
    got = buf.cpu().numpy().view(np.uint64)
    return got[:MH_COUNTERS].copy(), got[MH_COUNTERS:].copy()


def garbage():
    import torch
    buf = torch.full((2 * MH_COUNTERS,), -0x0123456789ABCDEF, dtype=torch.int64, device="cuda")      # (as uint64: above every expected value)
    torch.cuda.synchronize()
    return buf


def check(B, side_stream=False):
    sc = S.bouncing_ball_scene()
    assert sc.nb == 1 and sc.lcp_n_max == 8                      # 8 x 8 doubles of LU workspace per world
    aux = crafted_aux(B)
    sums, maxs = expected(aux)
    if B >= 7:
        assert len({int(np.argmax(aux[f])) for f in FIELDS if f}) == 7 and int(np.argmax(aux["steps"])) == 0 and int(np.argmax(aux["lcp_rows"])) == B - 1
    assert 0 < sums[3] < B or B == 1
    assert (aux["status"] == S.MH_WORLD_IMPACT_TOL).sum() > 0 or B == 1          # worlds that must NOT count as failed
    st = np.zeros((B, S.MH_BODY_STATE)); st[:, 6] = 1.0
    dev = WorldBatchDevice(sc, st, aux=aux)
    try:
        buf = garbage()
        got = reduce_on_device(dev, buf)
        np.testing.assert_array_equal(got[0], sums)
        np.testing.assert_array_equal(got[1], maxs)
        again = reduce_on_device(dev, buf)                        # into the same buffers: reset, not accumulated
        np.testing.assert_array_equal(again[0], sums)
        np.testing.assert_array_equal(again[1], maxs)
        if side_stream:
            buf2 = garbage()
            import torch
            side = reduce_on_device(dev, buf2, stream=torch.cuda.Stream())
            np.testing.assert_array_equal(side[0], sums)
            np.testing.assert_array_equal(side[1], maxs)
        aux_back = dev.download()[1]
        assert aux_back.tobytes() == aux.tobytes()                # the records are read, never written
    finally:
        dev.close()


@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_counter_reduction_equals_numpy(B):
    check(B, side_stream=B in (257, 1000))


def test_counter_reduction_with_a_second_grid_stride_trip():
    """B = 256 * 1024 + 300: the grid is capped at 1024 blocks, so the last 300 worlds are read in a second trip of the loop (one of the maxima is in
    world B - 1).  About 0.4 GB of aux records; nothing else is launched"""
    check(256 * 1024 + 300)
