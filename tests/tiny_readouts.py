"""The per-feature read-outs at the smallest shapes: tiny_shapes.CASES handed to the read-out helpers as
(n, P g, g, K), the edges of each read-out's own tiling that only such shapes reach, and the few cases each feature
runs (tests/test_tiny_readouts.py: the census and the host restatements on the CPU;
tests/test_gpu_tiny_readouts.py: the device).

The chain is probe_cases': burn-in 1, 6 iterations, thin 2, three saved samples, injected draws,
make_case(..., seed=21, k0=4) -- what every run_* helper of the read-out tests does.  No bar is new: every
assertion is the one of the feature's own test file, at new shapes.

  unit                                   fixed granularity                          reached only when
  k_probes                               probe_slices(G) = min(32, 256 / G) slices   P < S: empty slices; P = 1: one live
                                         of a shard's P rows, j0 = floor(P sl / S)   slice of one row
  k_precision (loglik, predict too)      precision_slices, 32 staged rows, 4-row     P < 8: one slice; nr < 4; nr = 1;
                                         MFMA k-step (nr4)                           nv = 0 and 32 with K = 1; g = 16
  loglik T pass / k_loglik_close         16-row tiles of n                           n = 2, n < 16, n = 15, n = 17
  predict                                per-row mask weights                        P = 1: a masked shard is one variable;
                                                                                     a shard with no observed row; |A| = 1, 0
  panel stage of precision_mean.hip      PM_PROWS = 64 rows per block                P < 64; P = 1
  slot_tiles.h (m2, partial corr, corr)  128 x 128 tile, 16 x 16 MFMA tiles          p < 16; p = 1; P = 1, g >= 2: no
                                                                                     same-shard pair off the diagonal;
                                                                                     P = 2, g = 16
  k_reg_rows / k_reg_small               RG_ROWS = 16 rows per block                 p < 16; P = 1; q = p - 1; nsh = q
  k_impute / k_impute_yy                 one lane per missing entry, 256 per block   nmiss < 64; nmiss = 1; a wholly missing
                                                                                     column; n = 2
  k_sigma_apply / CG panels / Krylov     128-row tiles, row pairs per thread         p < 16; p = 1; p odd with nv > 1;
                                                                                     nv = 32 > p; r = p; r < p <= 4
"""
import functools

import numpy as np

import tiny_shapes as ts

CASES = ts.CASES
case_id = ts.case_id
wide = ts.wide

PROBE_SLICES_MAX, PROBE_FAN, PREC_ROWS, PM_PROWS, RG_ROWS, TILE = 32, 8, 32, 64, 16, 128   # csrc/dcfm_internal.h, *.hip


def shape(case):
    """(n, p, g, K) of a case (n, P, g, K): what the run_* helpers and make_case take."""
    n, P, g, K = case
    return (n, P * g, g, K)


def probe_slices(G):
    return 1 if G >= 256 else min(256 // G, PROBE_SLICES_MAX)


def precision_slices(G, P, K, nv):
    wp = (K + nv + 15) // 16 * 16
    rows = max(wp // 2, 8)
    return min(probe_slices(G), max(P // rows, 1))


def dims(case):
    """The rounding rules of the read-out kernels at a case."""
    n, P, g, K = case
    p = P * g
    S = probe_slices(g)
    live = sum(1 for sl in range(S) if P * sl // S < P * (sl + 1) // S)
    sp = precision_slices(g, P, K, 0)
    nr = min(PREC_ROWS, P * 1 // sp)                              # rows of slice 0's first staged block
    return dict(n=n, P=P, g=g, K=K, p=p, probe_slices=S, probe_live=live, precision_slices=sp, nr=nr,
                nr4=(nr + 3) & ~3, fan_groups=(g + PROBE_FAN - 1) // PROBE_FAN,
                row_tiles=(n + 15) // 16, row_tile_last=(n - 1) % 16 + 1,
                pm_blocks=(P + PM_PROWS - 1) // PM_PROWS, pm_last_rows=(P - 1) % PM_PROWS + 1,
                tiles=(p + TILE - 1) // TILE, mfma_tiles=(p + 15) // 16,
                reg_blocks=(p + RG_ROWS - 1) // RG_ROWS, reg_shards_per_block=min(g, (RG_ROWS + P - 1) // P),
                row_pairs=(p + 1) // 2, odd_p=p % 2 == 1)


# ---- per-feature subsets -------------------------------------------------------------------------------------
P1, P1_K1, P1_WIDE = (9, 1, 4, 3), (2, 1, 3, 1), (60, 1, 2, 33)
ONE = (4, 1, 1, 1)                                                        # p = 1
PROBE_CASES = [ONE, P1, (6, 2, 3, 2), (17, 7, 2, 5), (11, 2, 16, 3), P1_WIDE, (45, 3, 2, 40)]
PROBE_NVS = (1, 5, 32)
PRECISION_CASES = [ONE, P1_K1, P1, (6, 2, 3, 2), (7, 3, 1, 2), (17, 7, 2, 5), (15, 9, 3, 12), (11, 2, 16, 3), P1_WIDE,
                   (45, 3, 2, 40)]
PRECISION_NVS = (0, 1, 5, 32)
LOGLIK_CASES = [ONE, P1_K1, (5, 1, 3, 2), P1, (45, 1, 2, 30), (3, 5, 2, 1), (17, 7, 2, 5), (15, 9, 3, 12), P1_WIDE,
                (45, 3, 2, 40)]                                           # n = 2, 3, 5, 15, 17 among them
LOGLIK_PRECISION_CASE = P1                                                # the cross-check with the precision draws
PREDICT_TS = (0, 1, 5)
# case -> the masks kept ("single" at (6, 2, 3, 2) is not: |A| = 1 makes the bar's kappa(Sigma_AA) 1 while the
# Woodbury form cancels -- its host restatement reaches 0.748 of the q bar at T = 5)
_ALL = ("random", "shard_off", "shard_on", "single", "empty", "full")
PREDICT_CASES = {ONE: ("empty", "full"), P1: _ALL, (6, 2, 3, 2): tuple(k for k in _ALL if k != "single"),
                 (12, 3, 2, 4): _ALL, (17, 7, 2, 5): _ALL, (11, 2, 16, 3): ("random", "shard_off"),
                 (45, 3, 2, 40): ("random", "shard_off", "full"), P1_WIDE: ("random", "empty")}
MOMENT_CASES = [ONE, P1_K1, P1, (6, 2, 3, 2), (17, 7, 2, 5), (11, 2, 16, 3), P1_WIDE, (45, 3, 2, 40)]   # mean, pc, corr, m2
BATCHED_CASES = [P1, P1_K1]                      # one run(1, N) with asm_batch 2: slot starts at odd multiples of K = 3, 1
REGRESSION_CASES = [P1_K1, P1, (6, 2, 3, 2), (17, 7, 2, 5), (15, 9, 3, 12), (11, 2, 16, 3), P1_WIDE, (45, 3, 2, 40)]
MISSING_CASES = [P1_K1, P1, (6, 2, 3, 2), (45, 3, 2, 40)]
MISSING_ONE_ENTRY = P1_K1                        # tiny_edges there: nmiss = 1
MISSING_PATTERNS = ("tiny_random", "tiny_edges")
MISSING_ACC_CASE = P1
# the Sigma operators by p: 1, 3 (odd), 4, 10, 27 (odd: unaligned panel columns with nv = 5 and 32), 32, and a wide chain
SIGMA_CASES = [ONE, (5, 1, 3, 2), P1, (3, 5, 2, 1), (15, 9, 3, 12), (11, 2, 16, 3), (45, 3, 2, 40)]
SIGMA_NVS = (1, 5, 32)
SOLVE_NVS = (1, 5, 32, 40)
LOOPBACK_CASE = P1                               # two ranks, two shards each


def eig_ranks(p):
    """The ranks sigma_eigs runs at a p: r = p where p <= 4 (the start block spans everything), r = 1 and p - 1 at
    p = 3, 4, 10, min(32, p) at p = 27 and 32, else 1 and min(6, p)."""
    if p == 1:
        return [1]
    if p in (3, 4):
        return [p, 1, p - 1]
    if p == 10:
        return [1, p - 1]
    if p in (27, 32):
        return [min(32, p)]
    return sorted({1, min(6, p)})


FEATURE_CASES = {
    "probes": PROBE_CASES, "precision": PRECISION_CASES, "loglik": LOGLIK_CASES, "predict": list(PREDICT_CASES),
    "precision_mean": MOMENT_CASES, "partial_corr": MOMENT_CASES, "corr": MOMENT_CASES, "sigma_m2": MOMENT_CASES,
    "regression": REGRESSION_CASES, "missing": MISSING_CASES, "sigma_apply": SIGMA_CASES, "sigma_solve": SIGMA_CASES,
    "sigma_eigs": SIGMA_CASES,
}
ADMITS_P1 = {f for f in FEATURE_CASES if f not in ("regression", "missing")}   # q < p; a mask of the only variable

MOMENTS = ("precision_mean", "partial_corr", "corr", "sigma_m2")
SIGMA_OPS = ("sigma_apply", "sigma_solve", "sigma_eigs")

# {edge: (the features it belongs to, predicate on dims())}
EDGES = {
    # k_probes
    "probes_empty_slices": (("probes",), lambda d: d["probe_live"] < d["probe_slices"]),
    "probes_one_live_slice_of_one_row": (("probes",), lambda d: d["P"] == 1 and d["probe_live"] == 1),
    "probes_two_fan_groups": (("probes", "precision"), lambda d: d["fan_groups"] == 2 and d["P"] == 2),
    # k_precision (also under loglik and predict)
    "precision_one_slice_under_8_rows": (("precision", "loglik", "predict"),
                                         lambda d: d["precision_slices"] == 1 and d["P"] < 8),
    "precision_fewer_rows_than_a_k_step": (("precision", "loglik", "predict"), lambda d: 1 < d["nr"] < 4),
    "precision_one_row": (("precision", "loglik", "predict"), lambda d: d["nr"] == 1),
    "precision_partial_k_step": (("precision",), lambda d: d["nr"] > 4 and d["nr4"] != d["nr"]),
    "precision_k1": (("precision",), lambda d: d["K"] == 1),          # with nv = 0 and 32: PRECISION_NVS
    # loglik: 16-row tiles of n
    "loglik_n_two": (("loglik",), lambda d: d["n"] == 2),
    "loglik_n_below_a_tile": (("loglik",), lambda d: d["row_tiles"] == 1 and d["row_tile_last"] < 15),
    "loglik_n_one_short_of_a_tile": (("loglik",), lambda d: d["row_tiles"] == 1 and d["row_tile_last"] == 15),
    "loglik_n_one_past_a_tile": (("loglik",), lambda d: d["row_tiles"] == 2 and d["row_tile_last"] == 1),
    # predict
    "predict_masked_shard_is_one_variable": (("predict",), lambda d: d["P"] == 1 and d["g"] >= 2),
    # panel stage of precision_mean.hip
    "panels_partial_block": (("precision_mean", "partial_corr", "regression"),
                             lambda d: d["pm_blocks"] == 1 and 1 < d["pm_last_rows"] < PM_PROWS),
    "panels_one_row": (("precision_mean", "partial_corr", "regression"), lambda d: d["P"] == 1),
    # slot_tiles.h
    "tiles_below_one_mfma_tile": (MOMENTS, lambda d: d["p"] < 16),
    "tiles_1x1": (MOMENTS, lambda d: d["p"] == 1),
    "tiles_no_same_shard_pair": (MOMENTS, lambda d: d["P"] == 1 and d["g"] >= 2),
    "tiles_sixteen_shards_of_two": (MOMENTS, lambda d: d["P"] == 2 and d["g"] == 16),
    # k_reg_rows / k_reg_small
    "reg_below_one_block": (("regression",), lambda d: d["p"] < RG_ROWS),
    "reg_every_row_its_own_shard": (("regression",), lambda d: d["P"] == 1 and d["g"] >= 2),
    "reg_two_blocks": (("regression",), lambda d: d["reg_blocks"] == 2),
    # k_impute / k_impute_yy (nmiss itself: tests/test_tiny_readouts.py counts the masks)
    "impute_n_two": (("missing",), lambda d: d["n"] == 2),
    "impute_one_row_shards": (("missing",), lambda d: d["P"] == 1),
    # k_sigma_apply / CG panels / block Krylov
    "sigma_below_one_mfma_tile": (SIGMA_OPS, lambda d: d["p"] < 16),
    "sigma_1x1": (SIGMA_OPS, lambda d: d["p"] == 1),
    "sigma_odd_p": (SIGMA_OPS, lambda d: d["odd_p"] and d["p"] > 1),
    "sigma_odd_p_past_a_tile": (SIGMA_OPS, lambda d: d["odd_p"] and d["p"] > 16),
    "sigma_block_wider_than_p": (SIGMA_OPS, lambda d: d["p"] < 32),
    "sigma_basis_saturates": (("sigma_eigs",), lambda d: 1 < d["p"] <= 4),
}


def census(feature_cases=None):
    """{(edge, feature): the cases of that feature's subset that reach the edge}."""
    fc = FEATURE_CASES if feature_cases is None else feature_cases
    return {(e, f): [c for c in fc[f] if pred(dims(c))] for e, (feats, pred) in EDGES.items() for f in feats}


# ---- tiny inputs ---------------------------------------------------------------------------------------------
TINY_SETS = ("last", "all_but_first")


def response_set(p, which):
    """The tiny response sets: `last` = [p - 1]; `all_but_first` = p - 1 ... 1 descending, capped at 32 (q = p - 1:
    one predictor, and at P = 1 every response is in its own shard); the others are regression_cases.response_set's
    (they need p >= 7)."""
    import regression_cases as gc
    if which == "last":
        return np.array([p - 1], dtype=np.int64)
    if which == "all_but_first":
        return np.arange(p - 1, 0, -1, dtype=np.int64)[:32].copy()
    assert p >= 7, "regression_cases.response_set needs p >= 7"
    return gc.response_set(p, which)


def response_sets(case):
    import regression_cases as gc
    p = case[1] * case[2]
    return TINY_SETS + (gc.SETS if p >= 7 else ())


def make_mask(pattern, case, seed=17):
    """Boolean n x P x g mask (True = missing).  `tiny_random`: 30 % missing completely at random.  `tiny_edges`: at
    MISSING_ONE_ENTRY one entry in total; else column 0 of shard 0 wholly missing (its yy starts from 0), row 1
    wholly missing in every shard but the last, the last shard untouched, and where n is odd the last row missing
    alone (one normal of a Philox pair) in the last column of the last touched shard."""
    n, P, g, K = case
    mk = np.zeros((n, P, g), dtype=bool)
    if pattern == "tiny_random":
        return np.random.default_rng(seed).random((n, P, g)) < 0.30
    assert pattern == "tiny_edges", pattern
    if tuple(case) == MISSING_ONE_ENTRY:
        mk[n - 1, P - 1, g // 2] = True
        return mk
    assert g >= 2 and n >= 3
    mk[:, 0, 0] = True
    mk[1, :, :g - 1] = True
    if n % 2:
        mk[n - 1, P - 1, g - 2] = True
    assert not mk[:, :, g - 1].any()
    return mk


@functools.lru_cache(maxsize=None)
def oracle_states(case, rho=0.5):
    """The saved (Lambda, omega) of the oracle's chain at the case (precision_cases.oracle_states; make_case must
    drop no column)."""
    import precision_cases as qc
    from helpers import make_case
    n, P, g, K = case
    c = make_case(n, P * g, g, K, seed=21, k0=4, rho=rho)
    assert (c["n"], c["P"], c["p"]) == (n, P, P * g), "preprocessing dropped a column"
    return qc.oracle_states(shape(case), rho=rho)
