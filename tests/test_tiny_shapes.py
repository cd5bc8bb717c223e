"""The case list of tests/tiny_shapes.py: its census of edges, and the reference at every case.  No GPU.

  1. Census.  Every edge of tiny_shapes.EDGES (derived from make_dims' rounding rules, restated in
     tiny_shapes.dims and held here against csrc/dcfm.hip's text) is reached by at least one case, and the
     sub-lists the GPU file runs in other modes are cases of the list.
  2. The reference is well posed at every case, by the measurement tests/test_gpu_tiny_shapes.py makes of the
     library: the faithful loop's iteration from a given start against helpers.stagewise_errors (the vectorised
     restatement, stage by stage, from that same start).  Bars, the project's own: every stage <= 1e-12, the faithful
     loop's loading backward error <= 1e-15, every row's scaled measure <= 1 / 8 of the bar of its class
     (helpers.SBW_TOL_WELL / SBW_TOL), ps and omega finite and positive.  A case that misses gets another n or
     seed, never another bar.
  3. Q14 is live: at every P = 1, K >= 2 case the per-column reading of dc:157 / dc:161 moves delta or tau by far
     more than the GPU test's 1e-10, so a library without the P == 1 branch cannot pass.

Measured (the TINY_REFERENCE and TINY_Q14 lines this file prints), worst over the 18 cases x 3 iterations: stages
1.2e-15 (X, Z, eta; every later stage 0: they are the same code on the same Lambda), loading backward error 5.5e-16
((3, 5, 2, 1)), scaled measure 0.68 % of its bar, cond(D Q_j D) <= 40 but (17, 7, 2, 5): 5.1e3 (its iteration 2,
max|X| 54.3), residual_rounding_bound <= 4.5e-13 ((150, 1, 2, 70); 1.7e-13 before Q14 moved the P = 1 chains);
one delta step under the per-column reading moves delta / tau by 0.15, 0.58, 2.6, 47, 3.5 and 5.1 relative at
(5, 1, 3, 2), (9, 1, 4, 3), (40, 1, 3, 7), (45, 1, 2, 30), (60, 1, 2, 33) and (150, 1, 2, 70), and by nothing at
every other case.
"""
import re
from pathlib import Path

import numpy as np
import pytest

import tiny_shapes as ts
from helpers import SBW_TOL, SBW_TOL_WELL, loading_scaled_bars, rel_err, residual_rounding_bound, stagewise_errors
from oracle import dc_oracle as F

CSRC = next(Path(__file__).resolve().parents[1].glob("*_amd")) / "csrc"

SELF_TOL = 1e-12      # faithful loop vs the vectorised stages, from the same start
SELF_BW = 1e-15       # the faithful loop's own loading backward error
Q14_MOVES = 1e-3      # what the per-column reading must move delta / tau by at least (the GPU bar is 1e-10)


def test_dims_restate_make_dims():
    text = (CSRC / "dcfm.hip").read_text()
    assert re.search(r"d\.NP = round_up\(c\.n, 128\);", text) and re.search(r"d\.PP = round_up\(c\.P, 32\);", text)
    internal = (CSRC / "dcfm_internal.h").read_text()
    pw = re.search(r"constexpr int padded_width\(int K\) \{ return (.*?); \}", internal).group(1)
    assert [int(v) for v in re.findall(r"\d+", pw)] == [32, 32, 64, 64, 128], pw
    for n, P, K, want in ((2, 1, 1, (128, 32, 32)), (128, 32, 32, (128, 32, 32)), (129, 33, 33, (256, 64, 64)),
                          (150, 1, 70, (256, 32, 128))):
        d = ts.dims((n, P, 2, K))
        assert (d["NP"], d["PP"], d["KW"]) == want


def test_every_edge_has_a_case():
    assert len(set(ts.CASES)) == len(ts.CASES) == 18
    assert all(not ts.wide(c) for c in ts.NARROW) and all(ts.wide(c) for c in ts.WIDE)
    for sub in (ts.MODE_CASES, ts.UNFUSED_CASES, ts.GENERATED_CASES, [c for c, _ in ts.LOOPBACK_CASES],
                ts.INGEST_CASES, ts.M2_CASES, ts.TRACE_CASES):
        assert set(sub) <= set(ts.CASES)
    for (n, P, g, K), per_rank in ts.LOOPBACK_CASES:
        assert g == 2 * per_rank
    # nothing else in the suite is this small: every case has P < 10, and the narrow ones below P = 8 or n = 20
    assert all(P < 10 for _, P, _, _ in ts.CASES)
    for edge, cases in ts.census().items():
        print("TINY_CENSUS", edge, [ts.case_id(c) for c in cases])
        assert cases, f"no case reaches the edge {edge}"
    # dropping a case that alone reaches an edge is seen
    alone = {e: cs[0] for e, cs in ts.census().items() if len(cs) == 1}
    assert alone
    for e, c in alone.items():
        assert not ts.census([x for x in ts.CASES if x != c])[e]


@pytest.mark.parametrize("key", ts.CASES, ids=ts.case_id)
def test_reference_is_well_posed(key):
    c = ts.case(key)
    ref = c["st"].copy()
    assert not np.any(ref.Lambda), "iteration 1 starts from Lambda = 0 with the caller's Plam"
    worst, worst_bw, worst_sbw, worst_cond, worst_bound, xmax = {}, 0.0, 0.0, 0.0, 0.0, 0.0
    for it in range(1, ts.N_ITER + 1):
        start = ref.copy()
        dr = c["src"].iteration(it)
        F.gibbs_iteration(ref, c["Yd"], c["rho"], c["hyper"], dr)
        errs, bw, _, (sbw, cond) = stagewise_errors(start, ref.as_dict(), c["Yd"], c["rho"], c["hyper"], dr, scaled=True)
        for f in ("ps", "omega"):
            v = getattr(ref, f)
            assert np.all(np.isfinite(v)) and np.all(v > 0.0), f"{key} iteration {it}: reference {f} out of range"
        for f, e in errs.items():
            worst[f] = max(worst.get(f, 0.0), e)
        worst_bw = max(worst_bw, bw)
        over = float(np.max(sbw / loading_scaled_bars(cond)))
        worst_sbw, worst_cond = max(worst_sbw, over), max(worst_cond, float(cond.max()))
        worst_bound = max(worst_bound, float(residual_rounding_bound(ref.as_dict(), c["Yd"]).max()))
        xmax = max(xmax, float(np.abs(ref.X).max()))
        assert over <= 1.0 / 8.0, (f"{key} iteration {it}: the reference's scaled loading measure at {over:.3g} of its "
                                   f"bar ({SBW_TOL_WELL:g} / {SBW_TOL:g})")
    print("TINY_REFERENCE", ts.case_id(key), {f: f"{e:.2e}" for f, e in sorted(worst.items())},
          f"lambda_bw {worst_bw:.2e} sbw/bar {worst_sbw:.2e} cond(DQD) {worst_cond:.3g} ps_bound {worst_bound:.2e} "
          f"max|X| {xmax:.3g}")
    for f, e in worst.items():
        assert e <= SELF_TOL, f"{key}: the oracle's two flavours differ in {f} by {e:.3e} (bar {SELF_TOL:.0e})"
    assert worst_bw <= SELF_BW, f"{key}: the faithful loop's loading backward error {worst_bw:.3e} (bar {SELF_BW:.0e})"


def _per_column_delta_tau(st, hyper, d):
    """dc:155-165 under the reading the project had before Q14: per-column sums at every P."""
    P, K, g = st.Lambda.shape
    delta, tauh = st.delta, st.tauh
    for m in range(g):
        cs = (st.psi[:, :, m] * st.Lambda[:, :, m] ** 2).sum(axis=0)
        bd = hyper.bd1 + (0.5 * (1.0 / delta[0, 0, m])) * np.sum(tauh[:, 0, m] * cs)
        delta[0, 0, m] = (1.0 / bd) * d.Gdelta[0, m]
        tauh[...] = F.matlab_cumprod_delta(delta)
        for h in range(1, K):
            bd = hyper.bd2 + (0.5 * (1.0 / delta[h, 0, 0])) * np.sum(tauh[h:, 0, m] * cs[h:])
            delta[h, 0, m] = (1.0 / bd) * d.Gdelta[h, m]
            tauh[:, :, m] = np.cumprod(delta[:, :, m], axis=0)


@pytest.mark.parametrize("key", ts.CASES, ids=ts.case_id)
def test_q14_is_live_exactly_at_P1(key):
    """One delta step from the state before it (iteration 1 of the chain): the per-column reading against the
    oracle's.  P = 1 and K >= 2: they differ by more than Q14_MOVES; every other case: bit for bit the same."""
    n, P, g, K = key
    c = ts.case(key)
    st = c["st"].copy()
    dr = c["src"].iteration(1)
    for upd in (lambda: F.update_Z(st, c["Yd"], c["rho"], dr), lambda: F.update_X(st, c["Yd"], c["rho"], dr),
                lambda: F.update_eta(st, c["rho"]), lambda: F.update_Lambda(st, c["Yd"], dr),
                lambda: F.update_psi(st, c["hyper"], dr)):
        upd()
    a, b = st.copy(), st.copy()
    F.update_delta_tau(a, c["hyper"], dr)
    _per_column_delta_tau(b, c["hyper"], dr)
    moved = max(rel_err(b.delta, a.delta), rel_err(b.tauh, a.tauh))
    print("TINY_Q14", ts.case_id(key), f"per-column reading moves delta / tau by {moved:.3e}")
    if P == 1 and K >= 2:
        assert moved > Q14_MOVES, f"{key}: the two readings of sum(mat) differ by {moved:.3e} only"
    else:
        assert np.array_equal(a.delta, b.delta) and np.array_equal(a.tauh, b.tauh)
