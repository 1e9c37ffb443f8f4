"""The batches of tests/test_world_bookkeeping_gpu.py do exercise what they are there for: checked on the CPU oracle, no GPU needed."""
import numpy as np

from moby_amd import scene as S
from tests.world_bookkeeping_ref import TRACE_ATTEMPT, reference_run


def deltas(per_step, field):
    """per-step increments of a counter, (nsteps, B)"""
    v = per_step[field].astype(np.int64)
    return np.diff(np.concatenate([np.zeros((1, v.shape[1]), dtype=np.int64), v]), axis=0)


def impact_solves(traces):
    """(nsteps, B) impact solves per step: each opens with the attempt-0 mark (the stabiliser's plain lcp_fast leaves none)"""
    return np.array([[int((t == TRACE_ATTEMPT).sum()) for t in tw] for tw in traces]).T


def test_stack_window_has_islands_of_one_and_of_three_contacts():
    """NK = 16: an island of k contacts is an LCP of 14 k rows (the stabiliser's rows counted off).  Some step solves exactly one impact LCP of 14 rows,
    some step one of 42; steps of several mini-steps occur"""
    _, _, aux, per_step, traces = reference_run("stack")
    rows, mini = deltas(per_step, "lcp_rows") - deltas(per_step, "stab_rows"), deltas(per_step, "mini_steps")
    solves = impact_solves(traces)
    assert ((solves == 1) & (rows == 14)).any()
    assert ((solves == 1) & (rows == 42)).any()
    assert (mini > 1).any() and (aux["steps"] == 60).all()


def test_two_balls_have_two_active_islands_in_one_mini_step():
    """epsilon = 0, NK = 4: one solve of 8 rows per active island and mini-step.  A step of ONE mini-step with TWO solves of 8 rows each had two active
    islands in that mini-step; every world has such a step, and the balls never meet (no solve of 16 rows)"""
    c, st, _, per_step, traces = reference_run("two_balls")
    rows, mini = deltas(per_step, "lcp_rows") - deltas(per_step, "stab_rows"), deltas(per_step, "mini_steps")
    solves = impact_solves(traces)
    two = (mini == 1) & (solves == 2) & (rows == 16)
    assert two.any(axis=0).all(), two.sum(axis=0)
    assert (rows == 8 * solves).all()
    s = st.reshape(-1, 2, S.MH_BODY_STATE)
    assert (np.abs(s[:, 0, 0] - s[:, 1, 0]) > 2.0).all()


def test_wheel_and_box_ball_solve_lcps():
    for name in ("wheel", "box_ball"):
        _, _, aux, _, _ = reference_run(name)
        assert (aux["lcp_solves"] > 0).all(), name
    assert (reference_run("wheel")[2]["vns_size"] > 0).all()                 # the no-slip model ran


def test_square_has_an_island_of_eight_contacts():
    """NK = 4: an island of k contacts is an LCP of 8 k rows.  Every impact solve of step 1 has 64 rows: the four spheres are one island of 8 contacts"""
    _, _, _, per_step, traces = reference_run("square")
    rows = deltas(per_step, "lcp_rows") - deltas(per_step, "stab_rows")
    solves = impact_solves(traces)
    assert (solves[0] >= 1).all() and (rows[0] == 64 * solves[0]).all()


def test_sunk_stack_is_stabilised():
    _, _, aux, per_step, _ = reference_run("sunk_stack")
    assert (per_step["stab_iters"][0] > 0).all() and (aux["stab_rows"] > 0).all()


def test_regularised_window_walks_the_ladder():
    """the oracle's trace of the window holds the opening of a ladder attempt, in the first step already; so do most steps of the stack batch"""
    _, _, _, _, traces = reference_run("regularised")
    assert (traces[0][0] == (TRACE_ATTEMPT | 1)).any()
    laddered = np.array([[bool((t == (TRACE_ATTEMPT | 1)).any()) for t in tw] for tw in reference_run("stack")[4]])
    assert laddered.any(axis=1).all() and laddered.mean() > 0.5
