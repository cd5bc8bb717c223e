"""GPU tests of the conditional prediction (dcfm_set_predict / dcfm_get_predict, csrc/predict.hip): the stepped
injected chain read out after every saved iteration against the dense Gaussian conditional of the state the
device held (predict_cases.dense and its bounds), cross-checks against the precision draws and Sigmaout, the
bitwise properties (rerun, call seams, NaN at unobserved entries, a zero row), off-means-off and coexistence with
every other recording, capacity and reset, the argument errors, the refusal on collective handles, and the
driver."""
import ctypes as C

import numpy as np
import pytest

import precision_cases as qc
import predict_cases as dc
import probe_cases as pc
from helpers import make_case, stacked_draws, state_dict

pytestmark = pytest.mark.gpu

BASE = (30, 60, 3, 3)
S = len(pc.SAVED)
# ((n, p, g, K), T, rho, mask): the base shape at every width, rho = 0 and 1 and every mask; one shard with one
# factor (uneven slices); P = 37 (no multiple of the MFMA step or of the 32-row block); twelve shards (two shard
# groups); K = 33 (a ragged last tile); K = 100 and 128 (the largest LDS plans)
CASES = ([(BASE, T, 0.5, "random") for T in (0, 1, 5, 32)] + [(BASE, 5, 0.0, "random"), (BASE, 5, 1.0, "random")] +
         [(BASE, 5, 0.5, kind) for kind in dc.MASKS if kind != "random"] +
         [((30, 21, 1, 1), 5, 0.5, "random"), ((30, 74, 2, 5), 5, 0.5, "random"), ((30, 60, 12, 2), 5, 0.5, "random"),
          ((40, 99, 3, 33), 5, 0.5, "random"), ((120, 200, 2, 100), 32, 0.5, "random"),
          ((120, 200, 2, 128), 5, 0.5, "shard_off")])
_runs = {}


def _inputs(shape, T, kind):
    p, g = shape[1], shape[2]
    return dc.new_rows(p, T), dc.mask(kind, p // g, g)


@pytest.fixture(scope="module")
def ran(dcfm):
    """(shape, T, rho, kind) -> the stepwise chain's read-outs and states, computed once and never modified."""
    def get(shape=BASE, T=5, rho=0.5, kind="random"):
        key = (shape, T, rho, kind)
        if key not in _runs:
            Y, ob = _inputs(shape, T, kind)
            _runs[key] = dc.run_predict(dcfm, shape, Y, ob, rho=rho)
        return _runs[key]
    yield get
    _runs.clear()


def _assert_run(r, shape, T, kind, what):
    n, p, g, K = shape
    P = p // g
    Y, ob = _inputs(shape, T, kind)
    assert len(r["reads"]) == S == len(r["states"])
    run, worst = dc.Running(), {}
    for s, (st, raw) in enumerate(zip(r["states"], r["reads"])):
        mean, m2, cvar, maha, ld, cnt = raw
        assert cnt == s + 1 and mean.shape == (p, T) == m2.shape and cvar.shape == (p,)
        assert maha.shape == (s + 1, T) and ld.shape == (s + 1,)
        d = dc.dense(Y, ob, st["Lambda"], st["omega"], r["rho"])
        b = dc.bounds(d, P, K, g, T)
        assert d["kappa"] <= 1e6
        run.add(d, b)
        rs = run.ratios(mean, m2, cvar)
        rs["q"] = dc._ratio(maha[s] - d["q"], b["q"])
        rs["ld"] = dc._ratio(ld[s] - d["ld"], b["ld"])
        for f, v in rs.items():
            worst[f] = max(worst.get(f, 0.0), v)
        if s:                                                # earlier draws stay as they were recorded
            assert np.array_equal(maha[:s], r["reads"][s - 1][3]) and np.array_equal(ld[:s], r["reads"][s - 1][4])
    print(f"{what}: err / bound " + ", ".join(f"{f} {v:.4f}" for f, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    return worst


@pytest.mark.parametrize("shape,T,rho,kind", CASES)
def test_every_read_out_matches_the_dense_conditional(ran, shape, T, rho, kind):
    r = ran(shape, T, rho, kind)
    _assert_run(r, shape, T, kind, f"{shape} T={T} rho={rho} {kind}")
    mean, m2, cvar, maha, ld, cnt = r["raw"]
    if T >= 3:                                               # the all-zero new row: exact zeros
        assert not mean[:, 1].any() and not m2[:, 1].any() and not maha[:, 1].any()
    assert np.all(cvar > 0) and np.all(m2 >= 0)


def test_full_mask_agrees_with_the_precision_draws(dcfm):
    """Y* = V under the full mask: diag q and the log det against precision_draws() of the same chain, produced
    by the unmasked kernel path, within the sum of the two bounds."""
    n, p, g, K = BASE
    V = pc.probe_block(p, 5)
    r = dc.run_predict(dcfm, BASE, V, dc.mask("full", p // g, g), keep=True,
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


def test_empty_mask(dcfm, ran):
    """Nothing observed: the prediction is the prior -- mean and maha exact zeros, log det of the empty matrix 0,
    and cvar the average of diag Sigma(s) = r diag(Sigmaout), r = effsamp / saved samples."""
    n, p, g, K = BASE
    r = dc.run_predict(dcfm, BASE, dc.new_rows(p, 5), dc.mask("empty", p // g, g), states=False, keep=True)
    try:
        sig = r["smp"].get_sigma()
    finally:
        r["smp"].close()
    mean, m2, cvar, maha, ld, cnt = r["raw"]
    assert cnt == S and not mean.any() and not m2.any() and not maha.any()
    assert np.all(np.abs(ld) <= 0.0)                         # its bound: |A| = 0
    want = (pc.EFFSAMP / S) * sig.diagonal()
    assert np.all(np.abs(cvar - want) <= 1e-12 * np.abs(want))
    assert dc.raw_bytes(r["raw"]) == dc.raw_bytes(ran(BASE, 5, 0.5, "empty")["raw"])


def test_bitwise_rerun_and_call_seams(dcfm, ran):
    """A rerun, one dcfm_run call, and a ragged cut (an empty call, cuts inside an assembly batch of two) give the
    bytes of the one-iteration-per-call chain for every output."""
    for key in ((BASE, 5, 0.5, "random"), ((40, 99, 3, 33), 5, 0.5, "random")):
        shape, T, rho, kind = key
        Y, ob = _inputs(shape, T, kind)
        want = dc.raw_bytes(ran(*key)["raw"])
        assert dc.raw_bytes(dc.run_predict(dcfm, shape, Y, ob, rho=rho)["raw"]) == want
        assert dc.raw_bytes(dc.run_predict(dcfm, shape, Y, ob, rho=rho, states=False)["raw"]) == want
        c = make_case(*shape, seed=21, k0=4, rho=rho)
        smp = pc.start(dcfm, c, shape[2], shape[3], asm_batch=2)
        try:
            smp.set_predict(Y, ob)
            for first, cnt in ((1, 0), (1, 3), (4, 1), (5, 0), (5, 3)):
                smp.run(first, cnt)
            assert dc.raw_bytes(smp.predict_raw()) == want
        finally:
            smp.close()


def test_unobserved_entries_are_ignored_and_a_zero_row_is_zero(dcfm, ran):
    Y, ob = _inputs(BASE, 5, "random")
    Ynan = np.where(ob[:, None] != 0, Y, np.nan)
    got = dc.run_predict(dcfm, BASE, Ynan, ob, states=False)["raw"]
    Yz = np.where(ob[:, None] != 0, Y, 0.0)
    zer = dc.run_predict(dcfm, BASE, Yz, ob, states=False)["raw"]
    assert dc.raw_bytes(got) == dc.raw_bytes(zer) == dc.raw_bytes(ran()["raw"])
    assert not got[0][:, 1].any() and not got[3][:, 1].any()  # new_rows' all-zero column


def test_off_means_off(dcfm):
    n, p, g, K = BASE
    c = make_case(n, p, g, K, seed=21, k0=4)
    Y, ob = _inputs(BASE, 5, "random")
    sig = []
    for on in (False, True):
        smp = dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], pc.BURNIN, pc.MCMC, pc.THIN, seed=11)
        try:
            smp.set_data(c["Yd"])
            smp.init_state()
            assert smp.predict()["count"] == 0
            if on:
                smp.set_predict(Y, ob)
                assert smp.predict()["count"] == 0           # nothing accumulated yet
            smp.run(1, pc.N)
            out = smp.predict()
            assert out["count"] == (S if on else 0)
            assert out["maha"].shape == (out["count"], 5 if on else 0) and out["logdet"].shape == (out["count"],)
            if on:
                assert out["mean"].shape == (p, 5) == out["sd_total"].shape == out["sd_between"].shape
                assert np.all(np.isfinite(out["mean"])) and np.all(out["sd_total"] >= np.sqrt(out["cvar"])[:, None])
            sig.append(smp.get_sigma())
        finally:
            smp.close()
    assert np.array_equal(sig[0], sig[1])                    # the same Philox chain, bit for bit


def test_coexistence(dcfm, ran):
    """Probes, precision probes, log-likelihood, second moment and precision mean on at once: each of their outputs
    is bitwise what it is without the prediction, and the prediction's are bitwise what they are alone."""
    n, p, g, K = BASE
    Y, ob = _inputs(BASE, 5, "random")
    V, W = pc.probe_block(p, 4, seed=6), pc.probe_block(p, 7, seed=8)

    def others(smp):
        smp.set_probes(W)
        smp.set_precision_probes(V)
        smp.set_loglik()

    got = []
    for on in (True, False):
        r = dc.run_predict(dcfm, BASE, Y, ob if on else None, states=False, keep=True, setup=others, sigma_m2=True,
                           precision_mean=True)
        smp = r["smp"]
        try:
            Q, qld = smp.precision_draws()
            _, lm, lld = smp.loglik_draws(parts=True)
            got.append({"sigma": smp.get_sigma(), "sd": smp.get_sigma_moment("sd"), "theta": smp.get_precision_mean(),
                        "probe": smp.probe_draws(), "Q": Q, "qld": qld, "maha": lm, "lld": lld, "raw": r["raw"]})
        finally:
            smp.close()
    for f in got[0]:
        if f != "raw":
            assert got[0][f].tobytes() == got[1][f].tobytes() and got[0][f].size, f
    assert got[1]["raw"][5] == 0
    assert dc.raw_bytes(got[0]["raw"]) == dc.raw_bytes(ran()["raw"])


def test_capacity_and_reset(dcfm, ran):
    full = ran()
    Y, ob = _inputs(BASE, 5, "random")
    r = dc.run_predict(dcfm, BASE, Y, ob, capacity=2, states=False, keep=True)
    smp = r["smp"]
    try:
        assert r["raw"][5] == 2                              # the first two samples, in the draws and the accumulators
        assert dc.raw_bytes(r["raw"]) == dc.raw_bytes(full["reads"][1])
        smp.set_predict(Y, ob, 4)                            # again: zeroes the accumulators and the count
        assert smp.predict_raw()[5] == 0
        smp.run(2, 1)
        one = smp.predict_raw()
        assert one[5] == 1 and one[0].any()
        smp.set_predict(None, None, 0)                       # off, buffers freed
        smp.run(2, 1)                                        # a saved iteration with the feature off
        off = smp.predict()
        assert off["count"] == 0 and off["mean"].shape == (BASE[1], 0)
    finally:
        smp.close()


def test_argument_errors_leave_the_setting_intact(dcfm, ran):
    from dcfm_amd import _abi
    n, p, g, K = BASE
    Y, ob = _inputs(BASE, 5, "random")
    c = make_case(*BASE, seed=21, k0=4)
    smp = pc.start(dcfm, c, g, K)
    lib, DP, UP = smp.lib, C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    Yf = np.asfortranarray(Y)
    bad = Yf.copy(order="F")
    bad[np.flatnonzero(ob)[3], 2] = np.inf                   # a non-finite observed entry
    try:
        smp.set_predict(Y, ob)
        yp, op = Yf.ctypes.data_as(DP), ob.ctypes.data_as(UP)
        for args in ((yp, None, 5, 3), (None, op, 5, 3), (yp, op, -1, 3), (yp, op, 33, 3), (yp, op, 5, -1),
                     (bad.ctypes.data_as(DP), op, 5, 3)):
            assert lib.dcfm_set_predict(smp.h, *args) == _abi.DCFM_ERR_INVALID, args[2:]
            assert lib.dcfm_last_error(smp.h)
        assert lib.dcfm_get_predict(smp.h, None, None, None, None, None, None) == _abi.DCFM_ERR_INVALID
        assert b"null argument" in lib.dcfm_last_error(smp.h)
        smp.run(1, pc.N)                                     # the setting made before is the one accumulated
        raw = smp.predict_raw()
        assert dc.raw_bytes(raw) == dc.raw_bytes(ran()["raw"])
        cnt = C.c_int64(-1)                                  # every output but count is nullable
        assert lib.dcfm_get_predict(smp.h, None, None, None, None, None, C.byref(cnt)) == _abi.DCFM_OK
        assert cnt.value == S
        only = np.zeros(p)
        assert lib.dcfm_get_predict(smp.h, None, None, only.ctypes.data_as(DP), None, None, C.byref(cnt)) == _abi.DCFM_OK
        assert np.array_equal(only, raw[2])
    finally:
        smp.close()


def _refused(smp, p, g):
    from dcfm_amd import _abi
    with pytest.raises(_abi.DcfmError) as ei:
        smp.set_predict(dc.new_rows(p, 2), dc.mask("random", p // g, g))
    assert ei.value.code == _abi.DCFM_ERR_UNSUPPORTED and "all shards" in str(ei.value)
    assert smp.predict()["count"] == 0


def test_loopback_ranks_are_refused(dcfm):
    """Two loopback ranks: DCFM_ERR_UNSUPPORTED with a message that says why, whichever of set_predict and
    comm_init_loopback comes second; nothing is set."""
    n, p, g, K = 30, 60, 4, 3
    refused = lambda smp: _refused(smp, p, g)
    smps = [dcfm.Sampler(n, p // g, g, K, 0.5, pc.BURNIN, pc.MCMC, pc.THIN, inject_draws=True, nranks=2, rank=r)
            for r in range(2)]
    try:
        for smp in smps:
            refused(smp)                                     # before the communicator
        dcfm.Sampler.comm_loopback(smps)
        for smp in smps:
            refused(smp)                                     # and after it
            smp.set_predict(None, None, 0)                   # turning it off stays legal
    finally:
        for smp in smps:
            smp.close()


def test_a_comm_self_handle_is_refused(dcfm):
    """One rank on the collective path (DCFM_FLAG_COMM_SELF): refused before and after dcfm_comm_init."""
    from dcfm_amd import _abi
    n, p, g, K = 30, 60, 4, 3
    smp = dcfm.Sampler(n, p // g, g, K, 0.5, pc.BURNIN, pc.MCMC, pc.THIN, flags=_abi.DCFM_FLAG_COMM_SELF)
    try:
        _refused(smp, p, g)
        smp.comm_init(dcfm.Sampler.unique_id())
        _refused(smp, p, g)
    finally:
        smp.close()


def test_read_out_after_a_numeric_error(dcfm):
    """The non-finite state of test_gpu_errors.py: the run ends in DCFM_ERR_NUMERIC at the next synchronising call
    and the read-out still returns, with what the device holds (no stage takes a data-dependent trip count)."""
    from dcfm_amd import _abi
    c = make_case(30, 40, 4, 3, seed=5)
    smp = dcfm.Sampler(c["n"], c["P"], 4, 3, c["rho"], 0, 3, 1, inject_draws=True)
    try:
        smp.set_data(c["Yd"])
        st = {f: np.array(v, copy=True) for f, v in state_dict(c["st"]).items() if f != "eta"}
        st["ps"][3, 0, 1] = np.nan
        smp.set_state(st)
        smp.set_draws(stacked_draws(c["src"], 1, 3), 1, 3)
        smp.set_predict(dc.new_rows(40, 2), dc.mask("random", 10, 4))
        smp.run(1, 1)
        with pytest.raises(_abi.DcfmError) as ei:
            smp.synchronize()
        assert ei.value.code == _abi.DCFM_ERR_NUMERIC
        out = smp.predict()
        assert out["count"] == 1 and out["mean"].shape == (40, 2) and not np.all(np.isfinite(out["cvar"]))
    finally:
        smp.close()


def test_driver_predict(dcfm):
    """divideconquer(..., predict=) on sparse-factor data with a dropped column and held-out rows: the dict equals
    the Sampler-level result pushed through the unit conversion, and the conditional mean beats the training
    column mean on the unobserved entries (a sanity check: only the inequality, the seed fixed)."""
    n, p0, g, k0, K, nt = 60, 61, 3, 3, 3, 6
    rng = np.random.default_rng(41)
    L0 = rng.standard_normal((p0, k0)) * (rng.random((p0, k0)) < 0.5)
    Yall = rng.standard_normal((n + nt, k0)) @ L0.T + 0.3 * rng.standard_normal((n + nt, p0)) + 2.0
    Yall[:, 17] = 0.0                                        # dropped: p = 60
    Y, Ynew = Yall[:n], Yall[n:]
    obs = rng.random(p0) < 0.6
    obs[17] = True                                           # a dropped column counts as unobserved whatever it says
    burnin, mcmc, thin = 20, 20, 2
    Sg, prd, info = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, 0.5, seed=5, predict=(Ynew, obs), return_info=True)
    assert set(prd) == {"mean", "sd_between", "sd_total", "log_density", "lppd", "count"} and prd["count"] == mcmc // thin
    assert prd["mean"].shape == (nt, p0) == prd["sd_total"].shape and prd["log_density"].shape == (mcmc // thin, nt)
    assert prd["lppd"].shape == (nt,) and np.all(np.isfinite(prd["lppd"]))
    assert not prd["mean"][:, 17].any() and not prd["sd_total"][:, 17].any()
    S0, _ = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, 0.5, seed=5, return_info=True)
    assert np.array_equal(Sg, S0)                            # Sigmaout does not see the prediction
    keep, varind = info["keep"], info["varind"]
    cmean, csd = dcfm.driver.column_moments(Y)
    Ystd, ob = dcfm.driver.standardize_rows(Ynew, obs, cmean, csd, keep, varind)
    assert ob.sum() == obs.sum() - 1
    smp = dcfm.Sampler(n, info["P"], g, info["K"], 0.5, burnin, mcmc, thin, seed=5)
    try:
        smp.set_data_raw(Y, dcfm.shard_columns(keep, varind, info["P"], 0, g))
        smp.init_state()
        smp.set_predict(Ystd, ob)
        smp.run(1, burnin + mcmc)
        want = dcfm.driver.unstandardize_prediction(smp.predict(), cmean, csd, keep, varind, p0)
    finally:
        smp.close()
    assert np.array_equal(want["mean"], prd["mean"]) and np.array_equal(want["sd_total"], prd["sd_total"])
    un = ~obs
    un[17] = False
    mse = np.mean((prd["mean"][:, un] - Ynew[:, un]) ** 2)
    base = np.mean((cmean[un][None, :] - Ynew[:, un]) ** 2)
    print(f"mse of the conditional mean {mse:.4f}, of the training column mean {base:.4f}")
    assert mse < base
