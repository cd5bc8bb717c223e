"""The smallest shapes: P < 8 variables per shard and n < 16 rows, down to P = 1 and n = 2, and the cases that
reach every piece of edge logic that only such shapes reach.

Every buffer of the library is padded (csrc/dcfm.hip make_dims: NP = ceil(n / 128) 128 rows, PP = ceil(P / 32) 32
columns, the factor width to 32, 64 or 128), and every kernel works on fixed tiles of the padded shape:

  unit                                                         its edges are reached when
  k_lambda: 8 loading rows per wave                            P < 8 (one live row: P = 1), P = 7, P = 9
  resid_rows8: 8 rows per wave                                 P < 8, in an exact-residual or guard launch
  k_resid_flagged: 32-row residual tiles                       K > 32 and P = 1, or 1 < P < 32
  W pass: ceil(P / 8) live 8-column chunks of a 32-column      P <= 8 (three skipped), P % 8 != 0 (partial)
  stripe's four
  16-row MFMA tiles of n                                       n < 16, n = 15, n = 17
  NP = ceil(n / 128) 128                                       n < 16 (>= 112 padding rows), n > 128
  colsum_tile: rows dealt to 8 groups                          P < 8 (empty groups), P = 1
  trace: 16 row slices per shard                               P < 16 (empty slices), P = 1
  k_colstats: 4 columns per block, 1 / (n - 1)                 P g % 4 != 0, P g < 4, n = 2
  k_assemble: 128-row tiles                                    P = 1, g >= 2: every off-diagonal pair is cross-shard
  delta_shard: the P == 1 branch (Q14)                         P = 1 and K >= 2; narrow, KW 64 and KW 128
  delta_shard: the K == 1 chain (Q5)                           K = 1, g >= 2, at P = 1 and at P > 1
  Sigma 1 x 1                                                  P = g = 1

EDGES names each edge and states it as a predicate on dims(); census() derives, from those rules restated here (dims()), which case reaches which edge;
tests/test_tiny_shapes.py asserts that every edge has a case, so an edit of CASES cannot silently drop one, and
measures the reference at every case.  Cases are (n, P, g, K); runs are 3 iterations (burn-in 1, two saved
samples) with injected draws, as tests/k_paths.py's.
"""
import functools

BURNIN, MCMC, THIN = 1, 2, 1
N_ITER = BURNIN + MCMC
SEED = 3

UNFUSED, EXACT, GUARD_ALL = 0x2, 0x10, 0x40     # include/dcfm.h
MODES = {"default": 0, "guard_all": GUARD_ALL, "exact": EXACT, "unfused": UNFUSED}

NARROW = [
    (2, 1, 3, 1),        # n = 2 (n - 1 = 1), the Q5 chain at P = 1
    (4, 1, 1, 1),        # p = 1: Sigma is 1 x 1
    (5, 1, 3, 2),        # Q4 and Q14
    (9, 1, 4, 3),
    (40, 1, 3, 7),
    (45, 1, 2, 30),      # k_lambda<30> with one live row
    (3, 5, 2, 1),
    (6, 2, 3, 2),
    (7, 3, 1, 2),        # g = 1
    (12, 3, 2, 4),
    (17, 7, 2, 5),       # one row short of a wave; iteration 2 is a mild excursion of the reference (max|X| 54)
    (15, 9, 3, 12),      # a full wave plus one row; n one short of a 16-row tile
    (40, 7, 2, 30),
    (11, 2, 16, 3),      # 16 shards of two rows: k_xdraw's source chunking at tiny P
]
WIDE = [
    (60, 1, 2, 33),      # KW 64; one live row in the 32-row residual tile
    (45, 3, 2, 40),
    (150, 1, 2, 70),     # KW 128, n > 128
    (100, 2, 2, 70),     # KW 128
]
CASES = NARROW + WIDE

MODE_CASES = [(9, 1, 4, 3), (12, 3, 2, 4), (15, 9, 3, 12), (60, 1, 2, 33), (45, 3, 2, 40)]   # guard_all and exact
UNFUSED_CASES = [(2, 1, 3, 1), (5, 1, 3, 2), (17, 7, 2, 5)]
GENERATED_CASES = [(9, 1, 4, 3), (15, 9, 3, 12), (60, 1, 2, 33)]
LOOPBACK_CASES = [((9, 1, 4, 3), 2), ((60, 1, 2, 33), 1)]          # (case, shards per rank) on two ranks
INGEST_CASES = [(2, 1, 3, 1), (9, 1, 4, 3), (3, 5, 2, 1)]          # P g = 3, 4 and 10 columns; n - 1 = 1
M2_CASES = [(9, 1, 4, 3), (17, 7, 2, 5)]
TRACE_CASES = [(2, 1, 3, 1), (15, 9, 3, 12)]


def round_up(a, b):
    return (a + b - 1) // b * b


def dims(case):
    """make_dims' rounding rules and the tile counts the kernels derive from them."""
    n, P, g, K = case
    kw = 32 if K <= 32 else (64 if K <= 64 else 128)
    return dict(n=n, P=P, g=g, K=K, p=P * g, NP=round_up(n, 128), PP=round_up(P, 32), KW=kw,
                lambda_waves=(P + 7) // 8, lambda_last_rows=(P - 1) % 8 + 1,        # 8 loading rows per wave
                wpass_chunks=round_up(P, 32) // 8, wpass_live=(P + 7) // 8,          # 8-column chunks of the W pass
                row_tiles=(n + 15) // 16, row_tile_last=(n - 1) % 16 + 1,            # 16-row MFMA tiles of n
                resid_tiles=round_up(P, 32) // 32, resid_last_rows=(P - 1) % 32 + 1,  # 32-row residual tiles (K > 32)
                colsum_groups_live=min(P, 8), trace_slices_live=min(P, 16),
                colstats_blocks=(P * g + 3) // 4, colstats_last_cols=(P * g - 1) % 4 + 1)


EDGES = {
    # k_lambda / resid_rows8: 8 rows per wave
    "lambda_one_live_row": lambda d: d["P"] == 1,
    "lambda_partial_single_wave": lambda d: 1 < d["P"] < 8,
    "lambda_one_row_short_of_a_wave": lambda d: d["lambda_waves"] == 1 and d["lambda_last_rows"] == 7,
    "lambda_full_wave_plus_one_row": lambda d: d["lambda_waves"] == 2 and d["lambda_last_rows"] == 1,
    "lambda30_one_live_row": lambda d: d["P"] == 1 and 25 <= d["K"] <= 30,
    "resid_partial_wave_in_a_residual_launch": lambda d: d["lambda_last_rows"] < 8 and tuple(
        d[k] for k in ("n", "P", "g", "K")) in MODE_CASES,
    # k_resid_flagged: 32-row tiles (wide K only)
    "resid_tile_one_live_row": lambda d: d["KW"] > 32 and d["resid_tiles"] == 1 and d["resid_last_rows"] == 1,
    "resid_tile_partial": lambda d: d["KW"] > 32 and 1 < d["resid_last_rows"] < 32,
    # W pass
    "wpass_three_padding_chunks": lambda d: d["wpass_chunks"] == 4 and d["wpass_live"] == 1,
    "wpass_partial_second_chunk": lambda d: d["wpass_live"] == 2 and d["P"] % 8 != 0,
    # 16-row MFMA tiles of n, NP
    "n_two_rows": lambda d: d["n"] == 2,
    "n_below_one_row_tile": lambda d: d["row_tiles"] == 1 and d["row_tile_last"] < 15,
    "n_one_short_of_a_row_tile": lambda d: d["row_tiles"] == 1 and d["row_tile_last"] == 15,
    "n_one_past_a_row_tile": lambda d: d["row_tiles"] == 2 and d["row_tile_last"] == 1,
    "np_one_block_mostly_padding": lambda d: d["NP"] == 128 and d["n"] < 16,
    "np_two_blocks": lambda d: d["NP"] == 256,
    # colsum_tile, trace
    "colsum_one_live_group": lambda d: d["colsum_groups_live"] == 1,
    "colsum_some_empty_groups": lambda d: 1 < d["colsum_groups_live"] < 8,
    "trace_one_live_slice": lambda d: d["trace_slices_live"] == 1 and tuple(
        d[k] for k in ("n", "P", "g", "K")) in TRACE_CASES,
    "trace_some_empty_slices": lambda d: 1 < d["trace_slices_live"] < 16 and tuple(
        d[k] for k in ("n", "P", "g", "K")) in TRACE_CASES,
    # k_colstats: four columns per block, /(n - 1)
    "colstats_fewer_columns_than_a_block": lambda d: d["p"] < 4 and tuple(
        d[k] for k in ("n", "P", "g", "K")) in INGEST_CASES,
    "colstats_one_whole_block": lambda d: d["p"] == 4 and tuple(d[k] for k in ("n", "P", "g", "K")) in INGEST_CASES,
    "colstats_partial_last_block": lambda d: d["colstats_blocks"] > 1 and d["colstats_last_cols"] < 4 and tuple(
        d[k] for k in ("n", "P", "g", "K")) in INGEST_CASES,
    "colstats_n_minus_1_is_1": lambda d: d["n"] == 2 and tuple(d[k] for k in ("n", "P", "g", "K")) in INGEST_CASES,
    # k_assemble
    "assemble_every_pair_cross_shard": lambda d: d["P"] == 1 and d["g"] >= 2,
    "assemble_1x1": lambda d: d["p"] == 1,
    # delta_shard
    "delta_q14_narrow": lambda d: d["P"] == 1 and d["K"] >= 2 and d["KW"] == 32,
    "delta_q14_kw64": lambda d: d["P"] == 1 and d["KW"] == 64,
    "delta_q14_kw128": lambda d: d["P"] == 1 and d["KW"] == 128,
    "delta_q14_with_q4": lambda d: d["P"] == 1 and d["K"] >= 2 and d["g"] >= 3,
    "delta_q5_at_p1": lambda d: d["P"] == 1 and d["K"] == 1 and d["g"] >= 2,
    "delta_q5_above_p1": lambda d: 1 < d["P"] < 8 and d["K"] == 1 and d["g"] >= 2,
    "g_one": lambda d: d["g"] == 1 and d["P"] > 1,
    "xdraw_sixteen_sources": lambda d: d["g"] == 16 and d["P"] < 8,
}


def census(cases=None):
    """{edge: the cases that reach it}."""
    cases = CASES if cases is None else cases
    return {e: [c for c in cases if pred(dims(c))] for e, pred in EDGES.items()}


def shape(case):
    return tuple(case)


def case_id(case):
    return "n%d_P%d_g%d_K%d" % tuple(case)


def wide(case):
    return case[3] > 32


@functools.lru_cache(maxsize=None)
def case(key):
    """helpers.make_case at the shape `key` = (n, P, g, K): data, initial state and draw source, made once."""
    from helpers import make_case
    n, P, g, K = key
    c = make_case(n, P * g, g, K, seed=SEED)
    assert (c["n"], c["P"]) == (n, P), "preprocessing dropped a column"
    return c
