"""The per-feature read-outs on the device at the smallest shapes: P < 8 variables per shard, n < 16 rows, P = 1,
p = 1 and odd p (tests/tiny_readouts.py: the cases of every feature and the edges they reach;
tests/test_tiny_readouts.py holds the host restatement of every combination run here within half of its bar on the
CPU).  Every runner and every assertion is the one of the feature's own test file; no bar is new.

  probes            probe_cases.run_probed, nv = 1, 5, 32; every draw within host_draw's bound (test_gpu_probes)
  precision         run_precision, nv = 0, 1, 5, 32; test_gpu_precision_draws._assert_draw; the zero probe gives exact
                    zeros; the log det does not depend on nv, bit for bit
  loglik            run_loglik and test_gpu_loglik._assert_run at n = 2, 3, 5, 15, 17; at a P = 1 case the precision
                    draws of the same rows
  predict           run_predict, T = 0, 1, 5, every kept mask; test_gpu_predict._assert_run; the full mask against the
                    precision draws
  precision mean, partial corr, corr, second moment
                    their runners and _assert_mean / _assert_moments / _check; symmetry, diagonals and stripes exact;
                    one run(1, N) with asm_batch 2 gives the stepped run's bits
  regression        run_reg with `last`, `all_but_first` (q = p - 1) and, from p = 7, the three existing sets;
                    _assert_moments entrywise; q = 1 at p = 1 is invalid
  missing           the step is the conditional (STEP_BAR, observed entries bit for bit) and the sweep reads the
                    completed data (1e-10 stage-wise, 1e-13 backward error; default, EXACT_RESIDUAL, GUARD_ALL) at
                    `tiny_random` and `tiny_edges`; the accumulators at one case (test_gpu_missing's bodies)
  sigma_apply       identity columns bit for bit, random V within _bound, nv = 1, 5, 32, p = 1, 3, 4, 10, 27, 32
  sigma_solve       check_solution with nv = 1, 5, 32, 40; columns of Sigma give identity columns; a column does not
                    depend on its neighbours, bit for bit, at odd p (the 8-byte panel path)
  sigma_eigs        _check at r = p (p <= 4, one pass), r = 1 and p - 1, r = min(32, p); r = p + 1 invalid
  two loopback ranks  (9, 1, 4, 3), two shards per rank: probes, precision, loglik and the moment read-outs

Measured on the MI355X: DESIGN.md section 2, "Smallest shapes"."""
import threading

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
import test_gpu_corr as TC
import test_gpu_loglik as TL
import test_gpu_missing as TMi
import test_gpu_partial_corr as TPC
import test_gpu_precision_draws as TQ
import test_gpu_precision_mean as TPM
import test_gpu_predict as TP
import test_gpu_probes as TPr
import test_gpu_regression as TR
import test_gpu_sigma_apply as TA
import test_gpu_sigma_eigs as TE
import test_gpu_sigma_moments as TM
import test_gpu_sigma_solve as TS
import tiny_readouts as tr
from helpers import make_case, rel_err, stacked_draws, state_dict
from sigma_cases import cases  # noqa: F401  (a fixture: shape -> (sampler after its chain, its Sigmaout))

pytestmark = pytest.mark.gpu

S = len(pc.SAVED)
RHO = 0.5
_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _cache.clear()


def _say(feature, case, **figures):
    print(f"TINY_READOUTS {feature} {tr.case_id(case)} " + " ".join(f"{k}={v:.4e}" for k, v in figures.items()))


# ---- probes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", tr.PROBE_NVS)
@pytest.mark.parametrize("case", tr.PROBE_CASES, ids=tr.case_id)
def test_probes(dcfm, case, nv):
    shape = tr.shape(case)
    V = pc.probe_block(shape[1], nv)
    r = pc.run_probed(dcfm, shape, V)
    assert r["draws"].shape == (S, nv, nv) and len(r["states"]) == S
    worst = 0.0
    for s, st in enumerate(r["states"]):
        Q, bound = pc.host_draw(V, st["Lambda"], st["omega"], r["rho"])
        assert np.all(np.isfinite(r["draws"][s]))
        TPr._assert_within(r["draws"][s], Q, bound, f"{shape} nv={nv} draw {s}")
        worst = max(worst, float(np.max(np.abs(r["draws"][s] - Q) / np.where(bound > 0, bound, 1.0))))
    if nv >= 3:                                              # the all-zero probe: exact zeros
        assert not r["draws"][:, 1, :].any() and not r["draws"][:, :, 1].any()
    assert np.array_equal(r["draws"], np.swapaxes(r["draws"], 1, 2))
    _say("probes", case, nv=nv, ratio=worst)


# ---- precision -------------------------------------------------------------------------------------------------
def _precision(dcfm, case, nv):
    shape = tr.shape(case)
    V = pc.probe_block(shape[1], nv)
    return V, _once(("precision", case, nv), lambda: qc.run_precision(dcfm, shape, V))


@pytest.mark.parametrize("nv", tr.PRECISION_NVS)
@pytest.mark.parametrize("case", tr.PRECISION_CASES, ids=tr.case_id)
def test_precision(dcfm, case, nv):
    V, r = _precision(dcfm, case, nv)
    assert r["Q"].shape == (S, nv, nv) and r["logdet"].shape == (S,) and len(r["states"]) == S
    wq = wl = 0.0
    for s, st in enumerate(r["states"]):
        TQ._assert_draw(r["Q"][s], r["logdet"][s], V, st, RHO, f"{tr.shape(case)} nv={nv} draw {s}")
        rq, rl, _ = qc.ratios(r["Q"][s], r["logdet"][s], V, st, RHO)
        wq, wl = max(wq, rq), max(wl, rl)
    if nv >= 3:                                              # the all-zero probe: exact zeros
        assert not r["Q"][:, 1, :].any() and not r["Q"][:, :, 1].any()
    assert np.array_equal(r["Q"], np.swapaxes(r["Q"], 1, 2))
    _say("precision", case, nv=nv, Q=wq, logdet=wl)


@pytest.mark.parametrize("case", tr.PRECISION_CASES, ids=tr.case_id)
def test_precision_logdet_does_not_depend_on_the_probes(dcfm, case):
    """Bit for bit among the widths that choose the same slice count (tiny_readouts.precision_slices), as
    test_gpu_precision_draws.test_logdet_does_not_depend_on_the_probes; at P < 16 that is every width."""
    n, P, g, K = case
    by_slices = {}
    for nv in tr.PRECISION_NVS:
        by_slices.setdefault(tr.precision_slices(g, P, K, nv), []).append(_precision(dcfm, case, nv)[1]["logdet"])
    assert len(by_slices) == 1 or P >= 16
    for lds in by_slices.values():
        assert all(np.array_equal(lds[0], x) for x in lds[1:])


# ---- loglik ----------------------------------------------------------------------------------------------------
def _loglik(dcfm, case):
    return _once(("loglik", case), lambda: lc.run_loglik(dcfm, tr.shape(case)))


@pytest.mark.parametrize("case", tr.LOGLIK_CASES, ids=tr.case_id)
def test_loglik(dcfm, case):
    r = _loglik(dcfm, case)
    TL._assert_run(r, tr.shape(case), f"{tr.shape(case)}")
    worst = [lc.ratios(r["maha"][s], r["logdet"][s], r["Yd"], st, RHO)[:2] for s, st in enumerate(r["states"])]
    _say("loglik", case, q=max(w[0] for w in worst), logdet=max(w[1] for w in worst))


def test_loglik_agrees_with_the_precision_draws_of_the_same_rows(dcfm):
    """test_gpu_loglik's cross-check at a P = 1 case: all n rows of get_data() as precision probes."""
    case = tr.LOGLIK_PRECISION_CASE
    shape = tr.shape(case)
    n, p, g, K = shape
    P, nr = p // g, min(n, 32)
    both = lc.run_loglik(dcfm, shape, precision_rows=nr, states=False)
    off = lc.run_loglik(dcfm, shape, precision_rows=nr, states=False, on=False)
    assert off["maha"].shape == (0, n) and both["Q"].shape == (S, nr, nr)
    assert both["Q"].tobytes() == off["Q"].tobytes() and both["qlogdet"].tobytes() == off["qlogdet"].tobytes()
    full = _loglik(dcfm, case)
    assert both["maha"].tobytes() == full["maha"].tobytes() and both["logdet"].tobytes() == full["logdet"].tobytes()
    for s, st in enumerate(full["states"]):
        qd, _, kappa = lc.dense(full["Yd"], st["Lambda"], st["omega"], full["rho"])
        bl, bld = lc.bounds(qd, kappa, P, K, g)
        bq = 4.0 * (P + K + g + nr) * lc.EPS * kappa * np.abs(qd)       # precision_cases.bounds on the diagonal
        d = np.abs(both["Q"][s].diagonal() - both["maha"][s, :nr])
        assert np.all(d <= bl[:nr] + bq[:nr])
        assert abs(both["qlogdet"][s] - both["logdet"][s]) <= bld


# ---- predict ---------------------------------------------------------------------------------------------------
PREDICT = [(c, k) for c, kinds in tr.PREDICT_CASES.items() for k in kinds]


@pytest.mark.parametrize("case,kind", PREDICT, ids=[f"{tr.case_id(c)}-{k}" for c, k in PREDICT])
def test_predict(dcfm, case, kind):
    shape = tr.shape(case)
    worst = {}
    for T in tr.PREDICT_TS:
        Y, ob = TP._inputs(shape, T, kind)
        r = dc.run_predict(dcfm, shape, Y, ob)
        for f, v in TP._assert_run(r, shape, T, kind, f"{shape} T={T} {kind}").items():
            worst[f] = max(worst.get(f, 0.0), v)
        mean, m2, cvar, maha, ld, cnt = r["raw"]
        if T >= 3:                                           # the all-zero new row: exact zeros
            assert not mean[:, 1].any() and not m2[:, 1].any() and not maha[:, 1].any()
        assert np.all(cvar > 0) and np.all(m2 >= 0)
        if kind == "empty":
            assert not mean.any() and not maha.any() and np.all(np.abs(ld) <= 0.0)
    _say("predict_" + kind, case, **worst)


@pytest.mark.parametrize("case", [tr.ONE, tr.P1, (17, 7, 2, 5)], ids=tr.case_id)
def test_predict_full_mask_agrees_with_the_precision_draws(dcfm, case):
    """test_gpu_predict.test_full_mask_agrees_with_the_precision_draws at the tiny cases."""
    shape = tr.shape(case)
    n, p, g, K = shape
    V = pc.probe_block(p, 5)
    r = dc.run_predict(dcfm, shape, V, dc.mask("full", p // g, g), keep=True,
                       setup=lambda smp: smp.set_precision_probes(V))
    try:
        Q, qld = r["smp"].precision_draws()
    finally:
        r["smp"].close()
    maha, ld = r["raw"][3], r["raw"][4]
    assert Q.shape == (S, 5, 5) and maha.shape == (S, 5)
    for s, st in enumerate(r["states"]):
        Qd, _, kappa = qc.dense(V, st["Lambda"], st["omega"], r["rho"])
        bq, bl = qc.bounds(Qd, kappa, p // g, K, g, 5)
        b = dc.bounds(dc.dense(V, np.ones(p), st["Lambda"], st["omega"], r["rho"]), p // g, K, g, 5)
        assert np.all(np.abs(Q[s].diagonal() - maha[s]) <= bq.diagonal() + b["q"])
        assert abs(qld[s] - ld[s]) <= bl + b["ld"]


# ---- precision mean, partial corr, corr, second moment ------------------------------------------------------------
def _run_m2(dcfm, shape, states=True, **kw):
    """probe_cases' chain with the second moment on: what run_mean / run_pc / run_corr do for their flags."""
    n, p, g, K = shape
    c = make_case(n, p, g, K, seed=21, k0=4)
    smp = pc.start(dcfm, c, g, K, sigma_m2=True, **kw)
    try:
        sts = []
        if not states:
            smp.run(1, pc.N)
        for it in range(1, pc.N + 1 if states else 0):
            smp.run(it, 1)
            if it in pc.SAVED:
                sts.append(smp.get_state(("Lambda", "omega")))
        c0, nc = rc.stripe(p)
        out = {w: smp.get_sigma_moment(w) for w in ("mean", "m2", "sd")}
        out.update({w + "_cols": smp.get_sigma_moment_cols(w, c0, nc) for w in ("mean", "m2", "sd")})
        out.update(sigma=smp.get_sigma(), states=sts, saved=smp.saved_samples(), c0=c0, nc=nc)
        return out
    finally:
        smp.close()


_MOMENT_FIELDS = {"precision_mean": ("T", "cols"), "partial_corr": ("mean", "m2", "sd", "mean_cols", "m2_cols", "sd_cols"),
                  "corr": ("mean", "m2", "sd", "mean_cols", "m2_cols", "sd_cols", "h", "h2", "hsd"),
                  "sigma_m2": ("mean", "m2", "sd", "mean_cols", "m2_cols", "sd_cols", "sigma")}


def _moment_run(dcfm, feature, case, **kw):
    shape = tr.shape(case)
    if feature == "precision_mean":
        return mc.run_mean(dcfm, shape, RHO, **kw)
    if feature == "partial_corr":
        return rc.run_pc(dcfm, shape, RHO, **kw)
    if feature == "corr":
        return cc.run_corr(dcfm, shape, RHO, **kw)
    return _run_m2(dcfm, shape, **kw)


def _stepped_moments(dcfm, feature, case):
    return _once((feature, case), lambda: _moment_run(dcfm, feature, case))


@pytest.mark.parametrize("case", tr.MOMENT_CASES, ids=tr.case_id)
def test_precision_mean(dcfm, case):
    shape = tr.shape(case)
    r = _stepped_moments(dcfm, "precision_mean", case)
    assert r["saved"] == len(r["states"]) == S
    ref = mc.dense_mean(r["states"], RHO, pc.EFFSAMP)
    TPM._assert_mean(r["T"], ref, f"{shape}")
    assert r["cols"].shape == (shape[1], r["nc"])
    assert np.array_equal(r["cols"], r["T"][:, r["c0"]:r["c0"] + r["nc"]])
    _say("precision_mean", case, ratio=mc.ratio(r["T"], ref), normwise=rel_err(r["T"], ref["T"]))


@pytest.mark.parametrize("case", tr.MOMENT_CASES, ids=tr.case_id)
def test_partial_corr(dcfm, case):
    r = _stepped_moments(dcfm, "partial_corr", case)
    assert r["saved"] == len(r["states"]) == S
    ref = rc.dense_moments(r["states"], RHO, pc.EFFSAMP)
    TPC._assert_moments(r, ref, r["saved"], pc.EFFSAMP, f"{tr.shape(case)}")
    _say("partial_corr", case, mean=float(np.max(np.abs(r["mean"] - ref["PC"]))) / ref["b"],
         m2=float(np.max(np.abs(r["m2"] - ref["PC2"]))) / (2 * ref["b"]))


@pytest.mark.parametrize("case", tr.MOMENT_CASES, ids=tr.case_id)
def test_corr(dcfm, case):
    r = _stepped_moments(dcfm, "corr", case)
    assert r["saved"] == len(r["states"]) == S
    ref = cc.dense_moments(r["states"], RHO, pc.EFFSAMP)
    TC._assert_moments(r, ref, r["saved"], pc.EFFSAMP, f"{tr.shape(case)}")
    b = ref["b"]
    _say("corr", case, C=float(np.max(np.abs(r["mean"] - ref["C"]))) / b, C2=float(np.max(np.abs(r["m2"] - ref["C2"]))) / (2 * b),
         H=float(np.max(np.abs(r["h"] - ref["H"]))) / b, H2=float(np.max(np.abs(r["h2"] - ref["H2"]))) / (2 * b))


@pytest.mark.parametrize("case", tr.MOMENT_CASES, ids=tr.case_id)
def test_second_moment(dcfm, case):
    r = _stepped_moments(dcfm, "sigma_m2", case)
    ref = TM._Ref(pc.EFFSAMP)
    for st in r["states"]:
        ref.add(st["Lambda"], st["omega"], RHO)
    assert r["saved"] == len(ref.samples) == S
    assert np.array_equal(r["mean"], r["sigma"]) and rel_err(r["mean"], ref.mean) < 1e-10
    TM._check(r["m2"], r["sd"], ref, f"TINY_READOUTS_M2 {tr.case_id(case)}")
    p = tr.shape(case)[1]
    for w in ("mean", "m2", "sd"):
        assert r[w + "_cols"].shape == (p, r["nc"]) and np.array_equal(r[w + "_cols"], r[w][:, r["c0"]:r["c0"] + r["nc"]])
    _say("sigma_m2", case, m2=rel_err(r["m2"], ref.m2) / 1e-10,
         var=float(np.max(np.abs(r["sd"] ** 2 - ref.var))) / (1e-10 * float(np.max(np.abs(ref.m2)))))


# what a flush rescales (add_tile: tile += (1 / effsamp) x the flush's sum) and what each carries as its squares
_RESCALED = {"precision_mean": ("T",), "partial_corr": ("mean", "m2"), "corr": ("mean", "m2"),
             "sigma_m2": ("mean", "sigma", "m2")}
_ONE_K_EXTENT = ("T", "sigma")  # and every mean but corr's: their kernels run a batch's slots along one k extent
SEAMS = [(1, 4), (5, 3)]       # saved iterations 2, 4 | 6: the run calls that end where asm_batch 2 flushes


def _assert_stepped(feature, case, r, sts, what):
    """The feature's own assertion on a run r against the dense reference of the states sts."""
    if feature == "precision_mean":
        return TPM._assert_mean(r["T"], mc.dense_mean(sts, RHO, pc.EFFSAMP), what)
    if feature == "partial_corr":
        return TPC._assert_moments(r, rc.dense_moments(sts, RHO, pc.EFFSAMP), S, pc.EFFSAMP, what)
    if feature == "corr":
        return TC._assert_moments(r, cc.dense_moments(sts, RHO, pc.EFFSAMP), S, pc.EFFSAMP, what)
    ref = TM._Ref(pc.EFFSAMP)
    for st in sts:
        ref.add(st["Lambda"], st["omega"], RHO)
    assert rel_err(r["mean"], ref.mean) < 1e-10
    TM._check(r["m2"], r["sd"], ref, what)


@pytest.mark.parametrize("feature", sorted(_MOMENT_FIELDS))
@pytest.mark.parametrize("case", tr.BATCHED_CASES, ids=tr.case_id)
def test_batched_flush_in_one_run(dcfm, case, feature):
    """One run(1, N) with asm_batch 2: the three saved samples flushed 2 + 1, the second slot at column K (K = 3 or
    1: 8-byte aligned only).

    A flush adds (1 / effsamp) x (the sum of its slots) to the tile (slot_tiles.h add_tile; k_assemble alike), and
    1 / effsamp = 1 / 3 here, so a run that groups the samples differently -- the stepped run flushes 1 + 1 + 1 --
    rounds differently: fl(c (t1 + t2)) against fl(c t1) + fl(c t2).  Measured on the MI355X: corr's mean at
    (9, 1, 4, 3) differs from the stepped run's in the last bit.  That is the design (tests/test_gpu_corr.py: "a run
    call ends with a flush, so another cut would regroup the sums"), not an alignment fault, so the bitwise
    comparison is with the same chain cut at the flush seams, as test_gpu_corr.test_batched_flush_in_one_run has it,
    and the stepped run is held to

      * the same bits wherever nothing is rescaled per flush (the communalities; the stripes against the matrices),
      * every assertion of the feature against the dense reference of the stepped run's states (the chain is the
        same bit for bit), and
      * |batched - stepped| <= 4 eps c sum_s |t_s| entrywise on the sums of the per-slot tile loop (slot_tiles.h:
        the per-sample products t_s are the same bits in both runs; either side is then within three roundings,
        3 x 2^-53, of the exact c sum_s t_s relative to c sum_s |t_s|), which is the second moment itself for a sum
        of squares and at most sqrt((S / effsamp) M2_ab) for corr's mean (Cauchy-Schwarz).  Sigmaout, the precision
        mean and the partial correlations' mean run a batch's slots along one k extent, so there the per-sample
        product never exists: they are held to their own bars against the dense reference alone."""
    one = _moment_run(dcfm, feature, case, states=False, asm_batch=2)
    stepped = _stepped_moments(dcfm, feature, case)
    assert one["saved"] == S
    shape = tr.shape(case)
    c = make_case(*shape, seed=21, k0=4)
    flag = {"precision_mean": "precision_mean", "partial_corr": "partial_corr", "corr": "corr", "sigma_m2": "sigma_m2"}
    smp = pc.start(dcfm, c, shape[2], shape[3], asm_batch=2, **{flag[feature]: True})
    try:
        for first, cnt in SEAMS:
            smp.run(first, cnt)
        assert smp.saved_samples() == S
        if feature == "precision_mean":
            cut = {"T": smp.get_precision_mean()}
        elif feature == "partial_corr":
            cut = rc.read_all(smp)
        elif feature == "corr":
            cut = cc.read_all(smp)
        else:
            cut = {w: smp.get_sigma_moment(w) for w in ("mean", "m2", "sd")}
    finally:
        smp.close()
    for f in cut:
        if isinstance(cut[f], np.ndarray):
            assert one[f].tobytes() == cut[f].tobytes(), (feature, f)
    full = dict(one, states=stepped["states"])
    _assert_stepped(feature, case, full, stepped["states"], f"batched {feature} {shape}")
    worst = 0.0
    for f in _MOMENT_FIELDS[feature]:
        if f.endswith("cols"):
            continue
        if f not in _RESCALED[feature]:
            if not f.endswith("sd"):                         # h, h2: added term by term, each with its own 1 / effsamp
                assert one[f].tobytes() == stepped[f].tobytes(), (feature, f)
            continue
        if f in _ONE_K_EXTENT or (f == "mean" and feature != "corr"):
            continue
        if f == "m2":
            mass = np.abs(stepped["m2"])
        else:
            mass = np.sqrt((S / pc.EFFSAMP) * np.abs(stepped["m2"]))
        diff = np.abs(one[f] - stepped[f])
        bar = 4.0 * pc.EPS * mass
        worst = max(worst, float(np.max(diff / np.where(bar > 0, bar, 1.0))))
        assert np.all(diff <= bar), (feature, f, float(np.max(diff / np.where(bar > 0, bar, 1.0))))
    _say("batched_" + feature, case, regroup=worst)


# ---- regression ------------------------------------------------------------------------------------------------
REGRESSION = [(c, w) for c in tr.REGRESSION_CASES for w in tr.response_sets(c)]


@pytest.mark.parametrize("case,which", REGRESSION, ids=[f"{tr.case_id(c)}-{w}" for c, w in REGRESSION])
def test_regression(dcfm, case, which):
    shape = tr.shape(case)
    R = tr.response_set(shape[1], which)
    r = gc.run_reg(dcfm, shape, RHO, R)
    assert r["count"] == len(r["states"]) == S
    ref = gc.dense_ref(r["states"], RHO, R)
    TR._assert_moments(r, ref, R, f"{shape} {which} (q={R.size})", entrywise=True)
    assert not r["coef"][R].any()                            # the response rows: exact zeros
    _say("regression_" + which, case, ratio=float(np.max(np.abs(r["coef"] - ref["coef"]) / ref["bound"])),
         normwise=max(rel_err(r[f], ref[f]) for f in gc.FIELDS) / 1e-10)


def test_regression_at_p_1_is_invalid(dcfm):
    """q < p: with one variable there is no regression; set_regression([0]) is the invalid-argument error."""
    from dcfm_amd import _abi
    n, p, g, K = tr.shape(tr.ONE)
    c = make_case(n, p, g, K, seed=21, k0=4)
    smp = pc.start(dcfm, c, g, K, regression=True)
    try:
        with pytest.raises(dcfm.DcfmError) as e:
            smp.set_regression(np.array([0], dtype=np.int64))
        assert e.value.code == _abi.DCFM_ERR_INVALID
        smp.run(1, pc.N)                                     # the handle still works
        assert smp.saved_samples() == S
    finally:
        smp.close()


# ---- missing ---------------------------------------------------------------------------------------------------
def _missing_name(case):
    name = "tiny_" + tr.case_id(case)
    TMi.SHAPES.setdefault(name, (tr.shape(case), 0))
    return name


MISSING = [(c, pat) for c in tr.MISSING_CASES for pat in tr.MISSING_PATTERNS]
_MISSING_IDS = [f"{tr.case_id(c)}-{pat}" for c, pat in MISSING]


@pytest.mark.parametrize("case,pattern", MISSING, ids=_MISSING_IDS)
def test_missing_the_step_is_the_conditional(dcfm, case, pattern):
    name, mask = _missing_name(case), tr.make_mask(pattern, case)
    try:
        worst = TMi._check_step(TMi._case(name), mask, TMi._stepped(dcfm, name, pattern, mask=mask),
                                f"{name} {pattern}")
    finally:
        TMi._cache.pop(("stepped", name, pattern, 0), None)
    _say("missing_step", case, nmiss=float(mask.sum()), ratio=worst)


@pytest.mark.parametrize("flags", [0, TMi.mc.EXACT_RESIDUAL, TMi.mc.GUARD_ALL], ids=["default", "exact", "guard_all"])
@pytest.mark.parametrize("case,pattern", MISSING, ids=_MISSING_IDS)
def test_missing_the_sweep_reads_the_completed_data(dcfm, case, pattern, flags):
    name, mask = _missing_name(case), tr.make_mask(pattern, case)
    try:
        stage, bw = TMi._check_sweep(TMi._case(name), TMi._stepped(dcfm, name, pattern, flags, mask=mask),
                                     f"{name} {pattern} flags {flags:#x}")
    finally:
        TMi._cache.pop(("stepped", name, pattern, flags), None)
    _say("missing_sweep", case, flags=float(flags), stage=stage / TMi.TOL, bw=bw / TMi.BW_TOL)


def test_missing_accumulators(dcfm):
    case = tr.MISSING_ACC_CASE
    worst = TMi._check_accumulators(dcfm, _missing_name(case), tr.make_mask("tiny_edges", case))
    _say("missing_acc", case, ratio=worst)


# ---- the Sigma operators ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tr.SIGMA_CASES, ids=tr.case_id)
def test_sigma_apply(cases, case):
    shape = tr.shape(case)
    smp, Sg = cases(shape)
    p = shape[1]
    for nv in tr.SIGMA_NVS:                                  # identity columns: Sigma's columns bit for bit
        if nv > p:
            continue
        for c0 in TA._starts(p, nv):
            V = np.zeros((p, nv))
            V[c0 + np.arange(nv), np.arange(nv)] = 1.0
            Y = smp.sigma_apply(V)
            assert Y.shape == (p, nv) and np.array_equal(Y, smp.get_sigma_cols(c0, nv)), (shape, nv, c0)
            assert np.array_equal(Y, Sg[:, c0:c0 + nv])
    rng = np.random.default_rng(5)
    worst = 0.0
    for nv in tr.SIGMA_NVS:                                  # nv = 5 and 32 at odd p: unaligned panel columns
        V = rng.standard_normal((p, nv))
        Y = smp.sigma_apply(V)
        err, bd = np.abs(Y - Sg @ V), TA._bound(Sg, V, p)
        worst = max(worst, float(np.max(err / bd)))
        assert Y.shape == (p, nv) and np.all(err <= bd), (shape, nv, float(np.max(err / bd)))
        assert np.array_equal(smp.sigma_apply(V), Y), "same input, different bytes"
        for j in sorted({0, nv // 2, nv - 1}):               # a column on its own: the same bits
            assert np.array_equal(smp.sigma_apply(V[:, j]), Y[:, j]), (shape, nv, j)
    _say("sigma_apply", case, ratio=worst)


@pytest.mark.parametrize("case", tr.SIGMA_CASES, ids=tr.case_id)
def test_sigma_solve(cases, case):
    shape = tr.shape(case)
    smp, Sg = cases(shape)
    p = shape[1]
    rng = np.random.default_rng(6)
    for nv in tr.SOLVE_NVS:
        B = rng.standard_normal((p, nv))
        X, info = smp.sigma_solve(B, tol=TS.TOL, return_info=True)
        TS.check_solution(Sg, B, X, info)
        X2, info2 = smp.sigma_solve(B, tol=TS.TOL, return_info=True)
        assert np.array_equal(X2, X), "same input, different bytes"
        for f in ("relres", "iters", "quad"):
            assert np.array_equal(info2[f], info[f]), f
    k = TS.kappa(Sg)
    for nv in (1, min(p, 17)):                               # columns of Sigma give identity columns
        for c0 in TS._starts(p, nv):
            B = np.asfortranarray(Sg[:, c0:c0 + nv])
            X, info = smp.sigma_solve(B, tol=TS.TOL, return_info=True)
            E = np.zeros((p, nv))
            E[c0 + np.arange(nv), np.arange(nv)] = 1.0
            err = np.linalg.norm(X - E, axis=0)
            assert np.all(err <= k * info["relres"] + p * TS.EPS * k), (shape, nv, c0)
            TS.check_solution(Sg, B, X, info)
    _say("sigma_solve", case, kappa=k)


@pytest.mark.parametrize("case", [c for c in tr.SIGMA_CASES if tr.dims(c)["odd_p"]], ids=tr.case_id)
def test_sigma_solve_a_column_does_not_depend_on_its_neighbours_at_odd_p(cases, case):
    """With p odd every second panel column starts 8 bytes off a 16-byte boundary: the 8-byte loads and stores of
    csrc/sigma_solve.hip.  A column's bits are those of the column solved alone (test_gpu_sigma_solve's test)."""
    shape = tr.shape(case)
    smp, _ = cases(shape)
    B = np.random.default_rng(12).standard_normal((shape[1], 40))
    X, info = smp.sigma_solve(B, tol=TS.TOL, return_info=True)
    for j in (0, 1, 7, 30, 31, 32, 39):                      # odd and even columns; 32, 39: the second chunk
        xj, ij = smp.sigma_solve(B[:, j], tol=TS.TOL, return_info=True)
        assert np.array_equal(xj, X[:, j]), j
        assert ij["relres"] == info["relres"][j] and ij["iters"] == info["iters"][j] and ij["quad"] == info["quad"][j]
    assert np.array_equal(smp.sigma_solve(B[:, 30:36], tol=TS.TOL), X[:, 30:36])
    assert np.array_equal(smp.sigma_solve(B[:, 1:6], tol=TS.TOL), X[:, 1:6])


@pytest.mark.parametrize("case", tr.SIGMA_CASES, ids=tr.case_id)
def test_sigma_eigs(cases, dcfm, case):
    from dcfm_amd import _abi
    shape = tr.shape(case)
    smp, Sg = cases(shape)
    p = shape[1]
    for r in tr.eig_ranks(p):
        res = smp.sigma_eigs(r, tol=TE.TOL)
        TE._check(res, Sg, r)
        if r == p:                                           # the start block spans everything
            assert res["passes"] == 1
        again = smp.sigma_eigs(r, tol=TE.TOL)
        for f in ("values", "vectors", "resid"):
            assert np.array_equal(res[f], again[f]), f
    if p < 32:
        with pytest.raises(dcfm.DcfmError) as e:
            smp.sigma_eigs(p + 1)                            # r > p
        assert e.value.code == _abi.DCFM_ERR_INVALID


# ---- two loopback ranks ------------------------------------------------------------------------------------------
def test_two_loopback_ranks_probes_precision_loglik(dcfm):
    """(9, 1, 4, 3), two one-row shards per rank: the assertions of the three features' own loopback tests."""
    case = tr.LOOPBACK_CASE
    shape = tr.shape(case)
    nv = 5
    V = pc.probe_block(shape[1], nv, seed=9)
    out, _ = pc.loopback_probed(dcfm, V, *shape)
    assert out[0].shape == (S, nv, nv) and out[0].tobytes() == out[1].tobytes()
    assert np.array_equal(out[0], np.swapaxes(out[0], 1, 2))
    one = pc.run_probed(dcfm, shape, V, case_seed=23)
    for s, st in enumerate(one["states"]):
        Q, bound = pc.host_draw(V, st["Lambda"], st["omega"], one["rho"])
        TPr._assert_within(out[0][s], one["draws"][s], bound, f"probes, two ranks against one, draw {s}")
        TPr._assert_within(out[0][s], Q, bound, f"probes, two ranks against the state, draw {s}")
    out, _ = qc.loopback_precision(dcfm, V, *shape)
    (Q0, l0), (Q1, l1) = out
    assert Q0.shape == (S, nv, nv) and l0.shape == (S,)
    assert Q0.tobytes() == Q1.tobytes() and l0.tobytes() == l1.tobytes()
    assert np.array_equal(Q0, np.swapaxes(Q0, 1, 2)) and not Q0[:, 1, :].any()
    one = qc.run_precision(dcfm, shape, V, case_seed=23)
    for s, st in enumerate(one["states"]):
        TQ._assert_draw(Q0[s], l0[s], V, st, one["rho"], f"precision, two ranks against the one-rank state, draw {s}")
        TQ._assert_draw(one["Q"][s], one["logdet"][s], V, st, one["rho"], f"precision, one rank, draw {s}")
    out, _ = lc.loopback_loglik(dcfm, *shape)
    (ll0, q0, l0), (ll1, q1, l1) = out
    assert q0.shape == (S, shape[0]) and l0.shape == (S,)
    assert q0.tobytes() == q1.tobytes() and l0.tobytes() == l1.tobytes() and ll0.tobytes() == ll1.tobytes()
    one = lc.run_loglik(dcfm, shape, case_seed=23)
    for s, st in enumerate(one["states"]):
        lc.assert_draw(q0[s], l0[s], one["Yd"], st, one["rho"], f"loglik, two ranks against the one-rank state, draw {s}")
        lc.assert_draw(one["maha"][s], one["logdet"][s], one["Yd"], st, one["rho"], f"loglik, one rank, draw {s}")


def _read_moments(smp, p):
    """Every collective moment read-out of a handle with all five accumulators on (rank > 0 passes NULL: None)."""
    c0, nc = rc.stripe(p)
    out = {"Sig": smp.get_sigma(), "m2": smp.get_sigma_moment("m2"), "sd": smp.get_sigma_moment("sd"),
           "sd_cols": smp.get_sigma_moment_cols("sd", c0, nc), "T": smp.get_precision_mean(),
           "T_cols": smp.get_precision_mean_cols(c0, nc)}
    for w in ("mean", "m2", "sd"):
        out["pc_" + w], out["corr_" + w] = smp.get_partial_corr(w), smp.get_corr(w)
    out["pc_cols"], out["corr_cols"] = smp.get_partial_corr_cols("sd", c0, nc), smp.get_corr_cols("sd", c0, nc)
    out["block"] = smp.sigma_block()
    return out


def test_two_loopback_ranks_moments(dcfm):
    """The moment features' test_two_ranks_loopback at (9, 1, 4, 3): one tile row, so rank 1's block is empty.
    Rank 0's gathered moments are bitwise the one-rank run's; rank 1 passed NULL; both ranks hold the same
    communalities; the oracle's chain is the reference at the features' own bars."""
    case = tr.LOOPBACK_CASE
    n, p, g, K = tr.shape(case)
    nr, asm_batch = 2, 2
    from sharded_protocol import sigma_split
    burnin, mcmc, thin, N = pc.BURNIN, pc.MCMC, pc.THIN, pc.N
    assert sigma_split(-(-p // 128), nr) == [0, 1, 1]
    flags = dict(sigma_m2=True, precision_mean=True, partial_corr=True, corr=True)
    c = make_case(n, p, g, K, seed=21, k0=4)
    G = g // nr
    draws = stacked_draws(c["src"], 1, N)
    smps = [dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], burnin, mcmc, thin, inject_draws=True, nranks=nr, rank=r,
                         device=0, asm_batch=asm_batch, **flags) for r in range(nr)]
    out, errs = [None] * nr, []
    try:
        dcfm.Sampler.comm_loopback(smps)
        for r, smp in enumerate(smps):
            smp.set_data(c["Yd"][:, :, r * G:(r + 1) * G])
            st = state_dict(c["st"], r * G, G)
            smp.set_state({f: st[f] for f in st if f != "eta"})
            smp.set_draws(draws, 1, N)

        def work(r):
            try:
                smps[r].run(1, N)
                out[r] = _read_moments(smps[r], p)
            except Exception as e:                        # surfaced below
                errs.append(e)

        ths = [threading.Thread(target=work, args=(r,)) for r in range(nr)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(timeout=100)
        assert not any(t.is_alive() for t in ths), "a rank did not finish"
        assert not errs, errs
        for r in range(nr):                               # not collective: one rank after the other
            for w in ("mean", "m2", "sd"):
                out[r]["h" + w] = smps[r].get_communality(w)
    finally:
        for smp in smps:
            smp.close()
    assert (out[0]["block"]["row0"], out[0]["block"]["row1"]) == (0, p)
    assert out[1]["block"]["row0"] == out[1]["block"]["row1"] and out[1]["block"]["bytes"] == 0
    fields = [f for f in out[0] if f != "block" and not f.startswith("h")]
    assert all(out[1][f] is None for f in fields)            # rank 1 passed NULL
    one = pc.start(dcfm, c, g, K, asm_batch=asm_batch, **flags)
    try:
        one.run(1, N)
        ref1 = _read_moments(one, p)
        for w in ("mean", "m2", "sd"):
            ref1["h" + w] = one.get_communality(w)
    finally:
        one.close()
    assert out[0]["block"]["bytes"] == ref1["block"]["bytes"]
    for f in fields:
        assert out[0][f].tobytes() == ref1[f].tobytes(), f
    for w in ("mean", "m2", "sd"):
        assert out[0]["h" + w].tobytes() == out[1]["h" + w].tobytes() == ref1["h" + w].tobytes(), w
    # and against the oracle's samples, at the features' own bars
    sts = qc.oracle_states((n, p, g, K))
    ref = TM._Ref(pc.EFFSAMP)
    for st in sts:
        ref.add(st["Lambda"], st["omega"], RHO)
    assert rel_err(out[0]["Sig"], ref.mean) < 1e-10
    TM._check(out[0]["m2"], out[0]["sd"], ref, "two ranks")
    TPM._assert_mean(out[0]["T"], mc.dense_mean(sts, RHO, pc.EFFSAMP), "two ranks")
    pref, cref = rc.dense_moments(sts, RHO, pc.EFFSAMP), cc.dense_moments(sts, RHO, pc.EFFSAMP)
    assert rel_err(out[0]["pc_mean"], pref["PC"]) < 1e-10 and rel_err(out[0]["pc_m2"], pref["PC2"]) < 1e-10
    assert rel_err(out[0]["corr_mean"], cref["C"]) < 1e-10 and rel_err(out[0]["corr_m2"], cref["C2"]) < 1e-10
    assert rel_err(out[1]["hmean"], cref["H"]) < 1e-10 and rel_err(out[1]["hm2"], cref["H2"]) < 1e-10
