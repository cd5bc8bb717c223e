"""CPU side of the read-outs at the smallest shapes (tests/tiny_readouts.py): the census (every edge of every
read-out's tiling has a case in the subset of the feature it belongs to; every feature has a P = 1, a 1 < P < 8 and a
wide case), the oracle's saved states at all 18 shapes, and -- a condition, not a measurement -- the host
restatement of every kept (feature, case, probe width / mask / response set) against the dense reference within
HALF of the bar the GPU test applies, kappa <= 1e6: the device is judged against bars the arithmetic meets with room.
Inputs were chosen to meet the condition, never bars (predict's `single` mask at (6, 2, 3, 2) is not kept:
tiny_readouts.PREDICT_CASES)."""
import functools

import numpy as np
import pytest

import corr_cases as cc
import loglik_cases as lc
import partial_corr_cases as rc
import precision_cases as qc
import precision_mean_cases as mc
import predict_cases as dc
import probe_cases as pc
import regression_cases as gc
import tiny_readouts as tr
from helpers import make_case, rel_err

HALF = 0.5
NORMWISE = 1e-10                     # the project's normwise bar


# ---- census ----------------------------------------------------------------------------------------------------
def test_every_edge_has_a_case_in_its_features_subset():
    for (edge, feature), cases in tr.census().items():
        assert cases, f"no case of {feature} reaches {edge}"


def test_a_dropped_case_is_seen():
    """(11, 2, 16, 3) alone reaches the sixteen-shards-of-two edge: without it the census has a hole."""
    fc = {f: [c for c in cs if c != (11, 2, 16, 3)] for f, cs in tr.FEATURE_CASES.items()}
    assert not tr.census(fc)[("tiles_sixteen_shards_of_two", "corr")]
    fc = {f: [c for c in cs if c != tr.ONE] for f, cs in tr.FEATURE_CASES.items()}
    assert not tr.census(fc)[("sigma_1x1", "sigma_solve")]


@pytest.mark.parametrize("feature", sorted(tr.FEATURE_CASES))
def test_every_feature_has_the_required_cases(feature):
    cases = tr.FEATURE_CASES[feature]
    assert all(c in tr.CASES for c in cases) and len(set(cases)) == len(cases)
    assert any(P == 1 and g >= 2 for _, P, g, _ in cases)
    assert any(1 < P < 8 for _, P, _, _ in cases)
    assert any(tr.wide(c) for c in cases)
    assert (tr.ONE in cases) == (feature in tr.ADMITS_P1)
    if feature in tr.SIGMA_OPS:
        ps = {P * g for _, P, g, _ in cases}
        assert {1, 3, 4, 10, 27, 32} <= ps and {5, 32} <= set(tr.SIGMA_NVS) and tr.SOLVE_NVS == (1, 5, 32, 40)


def test_dims_restate_the_kernels_rules():
    d = tr.dims((11, 2, 16, 3))
    assert (d["probe_slices"], d["probe_live"], d["fan_groups"], d["precision_slices"]) == (16, 2, 2, 1)
    d = tr.dims((9, 1, 4, 3))
    assert (d["probe_slices"], d["probe_live"], d["nr"], d["nr4"], d["pm_last_rows"]) == (32, 1, 1, 4, 1)
    d = tr.dims((15, 9, 3, 12))
    assert (d["p"], d["odd_p"], d["row_pairs"], d["reg_blocks"], d["nr"], d["nr4"]) == (27, True, 14, 2, 9, 12)
    assert tr.precision_slices(1, 21, 1, 5) == 2 and tr.precision_slices(3, 20, 3, 32) == 1   # test_gpu_precision_draws


def test_eig_ranks():
    assert tr.eig_ranks(1) == [1] and tr.eig_ranks(3) == [3, 1, 2] and tr.eig_ranks(4) == [4, 1, 3]
    assert tr.eig_ranks(10) == [1, 9] and tr.eig_ranks(27) == [27] and tr.eig_ranks(32) == [32]


def test_response_sets():
    assert list(tr.response_set(4, "last")) == [3] and list(tr.response_set(4, "all_but_first")) == [3, 2, 1]
    R = tr.response_set(32, "all_but_first")
    assert R.size == 31 and R[0] == 31 and R[-1] == 1
    assert tr.response_set(40, "all_but_first").size == 32
    for case in tr.REGRESSION_CASES:
        p = case[1] * case[2]
        for which in tr.response_sets(case):
            R = tr.response_set(p, which)
            assert 1 <= R.size < p and len(set(R.tolist())) == R.size and R.min() >= 0 and R.max() < p
    assert tr.response_sets((9, 1, 4, 3)) == tr.TINY_SETS and len(tr.response_sets((15, 9, 3, 12))) == 5


def test_tiny_masks_reach_the_impute_edges():
    seen = set()
    for case in tr.MISSING_CASES:
        n, P, g, K = case
        for pattern in tr.MISSING_PATTERNS:
            mk = tr.make_mask(pattern, case)
            assert mk.shape == (n, P, g) and mk.any()
            nmiss = int(mk.sum())
            seen |= {"nmiss<64"} if nmiss < 64 else {"nmiss>=64"}
            seen |= {"nmiss=1"} if nmiss == 1 else set()
            seen |= {"column"} if mk.all(axis=0).any() else set()
            if pattern == "tiny_edges" and case != tr.MISSING_ONE_ENTRY:
                assert mk.all(axis=0)[0, 0] and mk[1, :, :g - 1].all() and not mk[:, :, g - 1].any()
                if n % 2:
                    assert mk[n - 1, P - 1, g - 2]
                    seen.add("odd_row_out")
    assert seen >= {"nmiss<64", "nmiss>=64", "nmiss=1", "column", "odd_row_out"}
    assert tr.make_mask("tiny_edges", tr.MISSING_ONE_ENTRY).sum() == 1


# ---- the oracle's states ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tr.CASES, ids=tr.case_id)
def test_oracle_states(case):
    """make_case drops no column (asserted in oracle_states); the saved states are well conditioned."""
    sts = tr.oracle_states(case)
    assert len(sts) == len(pc.SAVED)
    kappa = max(np.linalg.cond(pc.sample_sigma(st["Lambda"], st["omega"], 0.5)) for st in sts)
    om, lam = min(st["omega"].min() for st in sts), max(np.abs(st["Lambda"]).max() for st in sts)
    print(f"TINY_READOUTS_STATES {tr.case_id(case)}: cond {kappa:.3e}, min omega {om:.3f}, max |Lambda| {lam:.3f}")
    assert kappa <= 1.1e2 and om >= 0.10 and lam <= 2.6


@functools.lru_cache(maxsize=None)
def _yd(case):
    n, P, g, K = case
    return make_case(n, P * g, g, K, seed=21, k0=4)["Yd"]


# ---- host restatements within half of each bar -------------------------------------------------------------------
@pytest.mark.parametrize("case", tr.PRECISION_CASES, ids=tr.case_id)
def test_precision_recursion(case):
    n, P, g, K = case
    worst = [0.0, 0.0]
    for nv in tr.PRECISION_NVS:
        V = pc.probe_block(P * g, nv)
        for st in tr.oracle_states(case):
            Q, ld = qc.woodbury(V, st["Lambda"], st["omega"], 0.5)
            rq, rl, kappa = qc.ratios(Q, ld, V, st, 0.5)
            worst = [max(worst[0], rq), max(worst[1], rl)]
            assert kappa <= 1e6 and rq <= HALF and rl <= HALF, (nv, rq, rl, kappa)
            if nv >= 3:
                assert not Q[1].any() and not Q[:, 1].any()
    print(f"TINY_READOUTS_HOST precision {tr.case_id(case)}: Q {worst[0]:.4f}, log det {worst[1]:.4f} of the bar")


@pytest.mark.parametrize("case", tr.LOGLIK_CASES, ids=tr.case_id)
def test_loglik_recursion(case):
    worst = [0.0, 0.0]
    for st in tr.oracle_states(case):
        q, ld = lc.recursion(_yd(case), st["Lambda"], st["omega"], 0.5)
        rq, rl, kappa = lc.ratios(q, ld, _yd(case), st, 0.5)
        worst = [max(worst[0], rq), max(worst[1], rl)]
        assert kappa <= 1e6 and rq <= HALF and rl <= HALF, (rq, rl, kappa)
    print(f"TINY_READOUTS_HOST loglik {tr.case_id(case)}: q {worst[0]:.4f}, log det {worst[1]:.4f} of the bar")


PREDICT = [(c, k) for c, kinds in tr.PREDICT_CASES.items() for k in kinds]


@pytest.mark.parametrize("case,kind", PREDICT, ids=[f"{tr.case_id(c)}-{k}" for c, k in PREDICT])
def test_predict_recursion(case, kind):
    n, P, g, K = case
    p = P * g
    ob = dc.mask(kind, P, g)
    worst = {}
    for T in tr.PREDICT_TS:
        Y = dc.new_rows(p, T)
        for st in tr.oracle_states(case):
            yhat, cv, q, ld = dc.recursion(Y, ob, st["Lambda"], st["omega"], 0.5)
            d = dc.dense(Y, ob, st["Lambda"], st["omega"], 0.5)
            r = dc.ratios(yhat, cv, q, ld, d, dc.bounds(d, P, K, g, T))
            assert d["kappa"] <= 1e6
            for f, v in r.items():
                worst[f] = max(worst.get(f, 0.0), v)
            assert all(v <= HALF for v in r.values()), (T, r)
    print(f"TINY_READOUTS_HOST predict {tr.case_id(case)} {kind} |A| = {int(ob.sum())}: "
          + ", ".join(f"{f} {v:.4f}" for f, v in worst.items()))


def test_predict_single_is_not_kept_where_the_bar_is_not_met_with_room():
    assert "single" not in tr.PREDICT_CASES[(6, 2, 3, 2)]
    for case in ((9, 1, 4, 3), (12, 3, 2, 4), (17, 7, 2, 5)):
        assert "single" in tr.PREDICT_CASES[case]


REGRESSION = [(c, w) for c in tr.REGRESSION_CASES for w in tr.response_sets(c)]


@pytest.mark.parametrize("case,which", REGRESSION, ids=[f"{tr.case_id(c)}-{w}" for c, w in REGRESSION])
def test_regression_panel_form(case, which):
    sts = tr.oracle_states(case)
    R = tr.response_set(case[1] * case[2], which)
    ref, got = gc.dense_ref(sts, 0.5, R), gc.panel_ref(sts, 0.5, R)
    errs = {f: rel_err(got[f], ref[f]) for f in gc.FIELDS}
    ratio = float(np.max(np.abs(got["coef"] - ref["coef"]) / ref["bound"]))
    print(f"TINY_READOUTS_HOST regression {tr.case_id(case)} {which} (q = {R.size}): entrywise ratio {ratio:.3e}, "
          f"normwise {max(errs.values()):.2e}")
    assert max(ref["kappa"]) <= 1e6
    assert all(e < HALF * NORMWISE for e in errs.values()), errs
    assert ratio <= HALF
    assert not got["coef"][R].any()


@pytest.mark.parametrize("case", tr.MOMENT_CASES, ids=tr.case_id)
def test_corr_restatement(case):
    sts = tr.oracle_states(case)
    ref, got = cc.dense_moments(sts, 0.5, pc.EFFSAMP), cc.device_moments(sts, 0.5, pc.EFFSAMP)
    b = ref["b"]
    e = {f: float(np.max(np.abs(got[f] - ref[f]))) for f in ("C", "C2", "H", "H2")}
    print(f"TINY_READOUTS_HOST corr {tr.case_id(case)}: " + ", ".join(f"{f} {v / b:.4f} b" for f, v in e.items()))
    assert e["C"] <= HALF * b and e["H"] <= HALF * b and e["C2"] <= HALF * 2 * b and e["H2"] <= HALF * 2 * b
    for f in ("C", "C2", "H", "H2"):
        assert rel_err(got[f], ref[f]) < HALF * NORMWISE


@pytest.mark.parametrize("case", tr.MOMENT_CASES, ids=tr.case_id)
def test_partial_corr_panel_form(case):
    sts = tr.oracle_states(case)
    ref = rc.dense_moments(sts, 0.5, pc.EFFSAMP)
    PC, PC2 = rc.panel_moments(sts, 0.5, pc.EFFSAMP)
    b = ref["b"]
    e1, e2 = float(np.max(np.abs(PC - ref["PC"]))), float(np.max(np.abs(PC2 - ref["PC2"])))
    print(f"TINY_READOUTS_HOST partial_corr {tr.case_id(case)}: mean {e1 / b:.4f} b, m2 {e2 / b:.4f} b")
    assert max(ref["kappa"]) <= 1e6
    assert e1 <= HALF * b and e2 <= HALF * 2 * b
    assert rel_err(PC, ref["PC"]) < HALF * NORMWISE and rel_err(PC2, ref["PC2"]) < HALF * NORMWISE


@pytest.mark.parametrize("case", tr.MOMENT_CASES, ids=tr.case_id)
def test_precision_mean_panels(case):
    sts = tr.oracle_states(case)
    ref = mc.dense_mean(sts, 0.5, pc.EFFSAMP)
    T = sum(mc.from_panels(*mc.panels(st["Lambda"], st["omega"], 0.5), case[1]) for st in sts) / pc.EFFSAMP
    r, e = mc.ratio(T, ref), rel_err(T, ref["T"])
    print(f"TINY_READOUTS_HOST precision_mean {tr.case_id(case)}: {r:.4f} of the bound, rel_err {e:.2e}")
    assert max(ref["kappa"]) <= 1e6 and r <= HALF and e < HALF * NORMWISE
