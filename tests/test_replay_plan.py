"""CPU checks of the exact-replay setup (replay_cases.py): the call plans cut the run where
test_gpu_replay.py says they do, the layouts build, and the reference itself is well conditioned at the
layouts' shapes over the whole run, so the stage-wise bars of test_gpu_replay.py are meaningful there."""
import numpy as np
import pytest

import replay_cases as rc
from helpers import STATE_CMP, rel_err
from oracle import dc_oracle as F
from oracle import philox_ref as R
from oracle import vectorised as V

SAVED = list(range(4, 27, 2))


@pytest.mark.parametrize("name", sorted(rc.PLANS))
def test_plan_covers_the_run_once_in_order(name):
    plan = rc.PLANS[name]
    assert all(first >= 1 and n >= 0 for first, n in plan)
    its = [it for first, n in plan for it in range(first, first + n)]
    assert its == list(range(1, rc.N + 1))
    nxt = 1
    for first, n in plan:                       # an empty call sits where the next one starts
        assert first == nxt
        nxt = first + n
    assert rc.saved_iterations(plan, rc.BURNIN, rc.THIN) == SAVED and len(SAVED) == 12


def test_plan_shapes():
    assert rc.ONE == [(1, 27)]
    assert len(rc.STEPPED) == 27 and all(n == 1 for _, n in rc.STEPPED)
    assert (14, 0) in rc.RAGGED and (4, 1) in rc.RAGGED


def test_flush_points():
    fp = {k: rc.flush_points(p, rc.BURNIN, rc.THIN, rc.ASM_BATCH) for k, p in rc.PLANS.items()}
    assert fp["ONE"] == [6, 10, 14, 18, 22, 26]
    assert fp["ALIGNED"] == fp["ONE"]
    assert fp["RAGGED"] == [4, 8, 12, 16, 20, 24, 27]          # 4 and 27: partial flushes at a call's end
    assert fp["STEPPED"] == SAVED
    assert fp["RAGGED"] != fp["ONE"] and fp["STEPPED"] != fp["ONE"]
    # every sample alone: one flush per saved sample, whatever the plan
    for p in rc.PLANS.values():
        assert rc.flush_points(p, rc.BURNIN, rc.THIN, 1) == SAVED


def test_draw_batches():
    assert rc.draw_batches(rc.ONE) == [(1, 8), (9, 8), (17, 8), (25, 3)]
    assert rc.draw_batches(rc.ALIGNED) == [(1, 6), (7, 8), (15, 8), (23, 5)]
    assert rc.draw_batches(rc.RAGGED) == [(1, 3), (4, 1), (5, 8), (13, 1), (14, 8), (22, 3), (25, 3)]
    assert rc.draw_batches(rc.STEPPED) == [(t, 1) for t in range(1, 28)]
    for plan in rc.PLANS.values():              # the batches tile the run
        assert [b0 + i for b0, nb in rc.draw_batches(plan) for i in range(nb)] == list(range(1, 28))
    assert rc.draw_batches([(3, 17)], DB=4) == [(3, 4), (7, 4), (11, 4), (15, 4), (19, 1)]


@pytest.mark.parametrize("name", ["ALIGNED", "RAGGED"])
def test_cuts_fall_inside_draw_batches(name):
    """A cut at iteration c is inside a draw batch when b0 < c < b0 + DB: the batch that starts at b0 is
    split by the call boundary.  At least one cut splits the last batch of the call before it (which that
    call therefore generated short), and at least one splits a batch of the unsplit run."""
    plan = rc.PLANS[name]
    DB = rc.DRAW_BATCH
    own = one = 0
    for (first, n), (nxt, _) in zip(plan, plan[1:]):
        if n == 0:
            continue
        cut = first + n
        assert cut == nxt
        own += any(b0 < cut < b0 + DB for b0, _ in rc.draw_batches([(first, n)]))
        one += any(b0 < cut < b0 + nb for b0, nb in rc.draw_batches(rc.ONE))
    assert own >= 1 and one >= 1


@pytest.mark.parametrize("layout", sorted(rc.LAYOUTS))
def test_layouts_build(layout):
    (n, p, g, K), flags = rc.LAYOUTS[layout]
    c = rc.case(layout)
    assert (c["n"], c["P"]) == rc.EXPECTED_NP[layout] == (n, p // g)
    assert (c["g"], c["K"]) == (g, K)
    assert (K > 32) == layout.startswith("wide")
    assert bool(flags & rc.UNFUSED) == layout.startswith("unfused")
    st = rc.init_state(c)
    assert "eta" not in st and st["Lambda"].shape == (c["P"], K, g)


@pytest.mark.parametrize("layout", ["wide64", "wide128", "unfused", "fused"])
def test_reference_is_well_conditioned(layout):
    """The faithful and the vectorised oracle, restarted from one state at every iteration and fed the host
    Philox variates of the chain seed, agree over all 27 iterations (bar 1e-10; measured 2.4e-15 to 2.3e-14)
    and X stays in the stationary range (max|X| < 10; measured 2.2 to 3.9)."""
    c = rc.case(layout)
    src = R.PhiloxSource(rc.CHAIN_SEED, c["n"], c["p"], c["g"], c["K"], c["hyper"])
    st = c["st"].copy()
    worst = xmax = 0.0
    for it in range(1, rc.N + 1):
        d = src.iteration(it)
        a, b = st.copy(), st.copy()
        F.gibbs_iteration(a, c["Yd"], c["rho"], c["hyper"], d)
        V.gibbs_iteration(b, c["Yd"], c["rho"], c["hyper"], d)
        for f in STATE_CMP:
            e = rel_err(getattr(b, f), getattr(a, f))
            worst = max(worst, e)
            assert e < 1e-10, f"iteration {it}: {f} differs between the two oracles by {e:.3e}"
        xmax = max(xmax, float(np.abs(a.X).max()))
        assert xmax < 10.0, f"iteration {it}: max|X| {xmax:.3g}: the reference left the stationary range"
        st = a
    print(f"REPLAY_CONDITIONING {layout}: oracle agreement {worst:.2e}, max|X| {xmax:.2g}")
