"""Posterior mean of the precision matrix on the GPU (DCFM_FLAG_PRECISION_MEAN, precision_mean.hip,
dcfm_get_precision_mean[_cols]).

The reference is built here, in NumPy: (1/effsamp) sum_s inv(Sigma(s)) with Sigma(s) the oracle's
assemble_sample of the state of every saved iteration (precision_mean_cases.dense_mean) -- the library's
own output is never its own reference.  Bars: entry by entry the bound of precision_mean_cases.dense_mean
(first order in eps kappa; every kappa_s must stay below 1e6), normwise the project's 1e-10
(helpers.rel_err), symmetry exact, a positive diagonal."""
import ctypes as C
import threading

import numpy as np
import pytest

import precision_mean_cases as mc
import probe_cases as pc
from helpers import STATE_CMP, make_case, rel_err, stacked_draws, state_dict
from oracle import dc_oracle as F

pytestmark = pytest.mark.gpu

# ((n, p, g, K), rho)
SWEEP = [
    ((30, 48, 4, 5), 0.5),         # one partial tile
    ((30, 36, 3, 1), 0.5),         # K = 1
    ((37, 300, 3, 7), 0.5),        # P = 100: shard edges inside tiles, mixed tiles
    ((37, 300, 3, 7), 0.0),        # no cross-shard term
    ((37, 300, 3, 7), 1.0),        # no same-shard term
    ((64, 384, 3, 30), 0.5),       # P = 128: pure cross and pure same-shard tiles; c3's K
    ((50, 128, 2, 32), 0.5),       # K = 32, aligned
    ((40, 99, 3, 33), 0.5),        # the wide state layout
    ((32, 1152, 9, 3), 0.5),       # 9 tile rows: crosses an 8 x 8 supertile
    ((120, 200, 2, 100), 0.5),     # K = 100
    ((140, 256, 2, 128), 0.5),     # K = 128: the LDS limit
]


def _assert_mean(T, ref, what):
    r, e = mc.ratio(T, ref), rel_err(T, ref["T"])
    print(f"{what}: kappa max {max(ref['kappa']):.3e}, max err / bound {r:.4f}, rel_err {e:.3e}")
    assert np.all(np.isfinite(T))
    assert max(ref["kappa"]) <= 1e6, f"{what}: kappa {max(ref['kappa']):.3e}"
    assert r <= 1.0, f"{what}: {r:.3f} of the bound"
    assert e < 1e-10
    assert np.array_equal(T, T.T)
    assert np.all(T.diagonal() > 0)


@pytest.mark.parametrize("shape,rho", SWEEP)
def test_stepwise_sweep(dcfm, shape, rho):
    """One iteration per run: the reference inverts the state the device held."""
    r = mc.run_mean(dcfm, shape, rho)
    assert r["saved"] == len(r["states"]) == len(pc.SAVED)
    ref = mc.dense_mean(r["states"], rho, pc.EFFSAMP)
    _assert_mean(r["T"], ref, f"{shape} rho={rho}")
    assert r["cols"].shape == (shape[1], r["nc"])
    assert np.array_equal(r["cols"], r["T"][:, r["c0"]:r["c0"] + r["nc"]])


def _saved(it, burnin, thin):
    return it % thin == 0 and it > burnin                          # dc:180


def _injected(dcfm, c, burnin, mcmc, thin, **kw):
    """A sampler at the case's initial state with injected draws for every iteration."""
    N = burnin + mcmc
    smp = dcfm.Sampler(c["n"], c["P"], c["g"], c["K"], c["rho"], burnin, mcmc, thin, inject_draws=True, **kw)
    smp.set_data(c["Yd"])
    smp.set_state({f: v for f, v in state_dict(c["st"]).items() if f != "eta"})
    smp.set_draws(stacked_draws(c["src"], 1, N), 1, N)
    return smp


def _oracle_states(c, burnin, mcmc, thin):
    """(Lambda, omega) of every saved iteration of the oracle's run_chain on case c."""
    st, out = c["st"].copy(), []
    for it in range(1, burnin + mcmc + 1):
        F.run_chain(c["Yd"], st, c["rho"], c["hyper"], c["src"].iteration, it, 1, burnin, mcmc, thin)
        if _saved(it, burnin, thin):
            out.append({"Lambda": st.Lambda.copy(), "omega": st.omega.copy()})
    return out


@pytest.mark.parametrize("K", [6, 5])     # slot starts s*K = 6, 12 (16-byte aligned) and 5, 10 (5: 8-byte only)
def test_batched_flush_in_one_run(dcfm, K):
    """7 saved samples flushed in batches of 3, 3 and 1 by a single run, against the oracle's chain.  The
    device's chain agrees with the oracle's to the project's normwise 1e-10 (the parity tests), not to the
    rounding bound of one inversion, so the bar here is the normwise one; the bound's ratio is printed."""
    n, p, g = 48, 64, 4
    burnin, mcmc, thin = 2, 14, 2
    c = make_case(n, p, g, K, seed=9)
    smp = _injected(dcfm, c, burnin, mcmc, thin, asm_batch=3, precision_mean=True)
    try:
        smp.run(1, burnin + mcmc)
        assert smp.saved_samples() == 7
        T = smp.get_precision_mean()
    finally:
        smp.close()
    sts = _oracle_states(c, burnin, mcmc, thin)
    assert len(sts) == 7
    ref = mc.dense_mean(sts, c["rho"], mcmc / thin)
    e = rel_err(T, ref["T"])
    print(f"batched K={K}: kappa max {max(ref['kappa']):.3e}, max err / bound {mc.ratio(T, ref):.4f}, rel_err {e:.3e}")
    assert max(ref["kappa"]) <= 1e6 and e < 1e-10
    assert np.array_equal(T, T.T) and np.all(T.diagonal() > 0)


def test_q8_scaling_and_mid_run(dcfm):
    """thin does not divide mcmc: effsamp = 2.5 while dc:180 saves iterations 2, 4 and 6.  The precision mean
    carries 1/effsamp as Sigmaout does; before the first saved sample it is all zeros."""
    n, p, g, K = 30, 40, 4, 3
    burnin, mcmc, thin = 1, 5, 2
    effsamp = mcmc / thin
    c = make_case(n, p, g, K)
    smp = _injected(dcfm, c, burnin, mcmc, thin, precision_mean=True)
    sts = []
    try:
        for it in range(1, burnin + mcmc + 1):
            if not sts:                                           # before any saved sample
                assert np.array_equal(smp.get_precision_mean(), np.zeros((p, p)))
                assert np.array_equal(smp.get_precision_mean_cols(3, 9), np.zeros((p, 9)))
            smp.run(it, 1)
            if not _saved(it, burnin, thin):
                continue
            sts.append(smp.get_state(("Lambda", "omega")))
            assert smp.saved_samples() == len(sts)
            _assert_mean(smp.get_precision_mean(), mc.dense_mean(sts, c["rho"], effsamp), f"Q8 after {len(sts)} saved")
        T = smp.get_precision_mean()
    finally:
        smp.close()
    assert len(sts) == 3 != effsamp
    plain = mc.dense_mean(sts, c["rho"], len(sts))["T"]           # the samples' plain mean
    assert rel_err(T * (effsamp / len(sts)), plain) < 1e-10


def test_flag_changes_nothing_that_exists(dcfm):
    from dcfm_amd import _abi
    n, p, g, K = 30, 200, 4, 5
    burnin, mcmc, thin = 1, 4, 1
    N = burnin + mcmc
    c = make_case(n, p, g, K, seed=4)
    V, W = pc.probe_block(p, 5), pc.probe_block(p, 7, seed=6)
    res = {}
    # the flag alone / nothing; then everything else with and without the flag
    for key, kw, extras in (("off", {}, False), ("on", dict(precision_mean=True), False),
                            ("rest", dict(sigma_m2=True), True),
                            ("all", dict(sigma_m2=True, precision_mean=True), True)):
        smp = _injected(dcfm, c, burnin, mcmc, thin, asm_batch=3, **kw)
        try:
            if extras:
                smp.set_probes(W)
                smp.set_precision_probes(V)
            smp.run(1, N)
            r = {"state": smp.get_state(), "Sig": smp.get_sigma(), "block": smp.sigma_block(),
                 "cols": smp.get_sigma_cols(37, 70)}
            if extras:
                r["m2"], r["sd"] = smp.get_sigma_moment("m2"), smp.get_sigma_moment("sd")
                r["probe"] = smp.probe_draws()
                r["Q"], r["logdet"] = smp.precision_draws()
            if kw.get("precision_mean"):
                r["T"] = smp.get_precision_mean()
                r["T_cols"] = smp.get_precision_mean_cols(37, 70)   # starts and ends off a 32 boundary
                with pytest.raises(dcfm.DcfmError) as e:
                    smp.get_precision_mean_cols(150, 51)            # past p
                assert e.value.code == _abi.DCFM_ERR_INVALID
                buf = np.zeros((p, 4), order="F")
                for c0, nc in ((-1, 4), (0, -1), (p, 1)):           # a bad column range
                    assert smp.lib.dcfm_get_precision_mean_cols(
                        smp.h, c0, nc, buf.ctypes.data_as(C.POINTER(C.c_double))) == _abi.DCFM_ERR_INVALID, (c0, nc)
                assert smp.lib.dcfm_get_precision_mean(smp.h, None) == _abi.DCFM_ERR_INVALID        # NULL out on rank 0
                assert smp.lib.dcfm_get_precision_mean_cols(smp.h, 0, 4, None) == _abi.DCFM_ERR_INVALID
                with pytest.raises(dcfm.DcfmError) as e:
                    smp.get_sigma_moment(3)                         # no new `which`
                assert e.value.code == _abi.DCFM_ERR_INVALID
            else:
                for call in (smp.get_precision_mean, lambda: smp.get_precision_mean_cols(0, 8)):
                    with pytest.raises(dcfm.DcfmError) as e:
                        call()
                    assert e.value.code == _abi.DCFM_ERR_INVALID and "DCFM_FLAG_PRECISION_MEAN" in str(e.value)
            res[key] = r
        finally:
            smp.close()
    off = res["off"]
    for key in ("on", "rest", "all"):
        assert np.array_equal(off["Sig"], res[key]["Sig"]) and np.array_equal(off["cols"], res[key]["cols"]), key
        for f in STATE_CMP:
            assert np.array_equal(off["state"][f], res[key]["state"][f]), (key, f)
        assert (res[key]["block"]["row0"], res[key]["block"]["row1"]) == (off["block"]["row0"], off["block"]["row1"])
    for f in ("m2", "sd", "probe", "Q", "logdet"):
        assert res["rest"][f].tobytes() == res["all"][f].tobytes(), f
    assert res["on"]["T"].tobytes() == res["all"]["T"].tobytes()
    assert np.array_equal(res["on"]["T_cols"], res["on"]["T"][:, 37:107])
    one = off["block"]["bytes"]
    assert one > 0 and [res[k]["block"]["bytes"] for k in ("on", "rest", "all")] == [2 * one, 2 * one, 3 * one]
    assert np.any(res["on"]["T"] != 0)


def test_two_ranks_loopback(dcfm):
    """Two ranks on one device (in-process loopback): 3 tile rows split [0, 2) | [2, 3).  The per-sample omega
    travels in the flush's all-gather and each rank forms the factor panels of all four shards.  Rank 0's
    gathered precision mean is bitwise the one-rank run's (same tiles, same factor bytes, same arithmetic)."""
    from sharded_protocol import sigma_split
    n, p, g, K, nr = 32, 384, 4, 6, 2
    burnin, mcmc, thin, asm_batch = 1, 4, 1, 3
    N = burnin + mcmc
    assert sigma_split(-(-p // 128), nr) == [0, 2, 3]
    c = make_case(n, p, g, K, seed=13)
    G = g // nr
    draws = stacked_draws(c["src"], 1, N)
    smps = [dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], burnin, mcmc, thin, inject_draws=True, nranks=nr, rank=r,
                         device=0, asm_batch=asm_batch, precision_mean=True) for r in range(nr)]
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
                out[r] = {"Sig": smps[r].get_sigma(), "T": smps[r].get_precision_mean(),
                          "T_cols": smps[r].get_precision_mean_cols(100, 200), "block": smps[r].sigma_block()}
            except Exception as e:                        # surfaced below
                errs.append(e)

        ths = [threading.Thread(target=work, args=(r,)) for r in range(nr)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(timeout=100)
        assert not any(t.is_alive() for t in ths), "a rank did not finish"
        assert not errs, errs
    finally:
        for smp in smps:
            smp.close()
    assert (out[1]["block"]["row0"], out[1]["block"]["row1"]) == (256, 384)
    assert all(out[1][f] is None for f in ("Sig", "T", "T_cols"))
    one = _injected(dcfm, c, burnin, mcmc, thin, asm_batch=asm_batch, precision_mean=True)
    try:
        one.run(1, N)
        ref1 = {"Sig": one.get_sigma(), "T": one.get_precision_mean()}
        total = one.sigma_block()["bytes"]
    finally:
        one.close()
    assert out[0]["block"]["bytes"] + out[1]["block"]["bytes"] == total
    for f in ("Sig", "T"):
        assert np.array_equal(out[0][f], ref1[f]), f
    assert np.array_equal(out[0]["T_cols"], ref1["T"][:, 100:300])
    # and against the oracle's samples
    _assert_mean(out[0]["T"], mc.dense_mean(_oracle_states(c, burnin, mcmc, thin), c["rho"], mcmc / thin), "two ranks")


def test_same_bits_on_a_second_run(dcfm):
    shape = (37, 300, 3, 7)
    a = mc.run_mean(dcfm, shape, states=False)
    b = mc.run_mean(dcfm, shape, states=False)
    assert a["T"].tobytes() == b["T"].tobytes() and a["cols"].tobytes() == b["cols"].tobytes()
    assert np.any(a["T"] != 0)


def test_driver_returns_the_precision_mean(dcfm):
    import oracle
    from dcfm_amd import driver as D
    n, p, g, K, rho = 40, 48, 4, 3, 0.5
    burnin, mcmc, thin, seed = 2, 6, 2, 31
    Y, _ = oracle.synth.make_data(n, p, k0=4)
    S, T, info = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, rho, seed=seed, return_precision=True,
                                    return_info=True)
    S2, SD, T2, pcs = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, rho, seed=seed, return_sd=True,
                                         return_precision=True, n_components=2)
    plain = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, rho, seed=seed)
    assert S.shape == T.shape == SD.shape == (p, p) and isinstance(info, dict) and set(pcs) >= {"values", "vectors"}
    assert np.array_equal(S, plain) and np.array_equal(S2, plain) and np.array_equal(T, T2)
    # the same chain at the Sampler level
    nn, pk, P, Kk, keep = D.preprocess_device(Y, g, K * g)
    smp = dcfm.Sampler(nn, P, g, Kk, rho, burnin, mcmc, thin, seed=seed, precision_mean=True)
    try:
        smp.set_data_raw(Y, D.shard_columns(keep, info["varind"], P, 0, g))
        smp.init_state()
        smp.run(1, burnin + mcmc)
        assert np.array_equal(smp.get_sigma(), S)
        assert np.array_equal(smp.get_precision_mean(), T)
    finally:
        smp.close()
    assert np.array_equal(T, T.T) and np.all(T.diagonal() > 0)
    R = dcfm.partial_correlations(T)
    assert np.array_equal(R.diagonal(), np.ones(p)) and np.all(np.abs(R) <= 1.0 + 1e-12)
    # back in the input's coordinates a precision entry is divided by the standard deviations
    sd_cols = np.asarray(Y)[:, D.output_columns(info["keep"], info["varind"])].std(axis=0, ddof=1)
    full = dcfm.unpermute_precision(T, info["keep"], info["varind"], Y.shape[1], sd=sd_cols)
    a, b = 3, 17
    ca, cb = D.output_columns(info["keep"], info["varind"])[[a, b]]
    assert full[ca, cb] == T[a, b] / sd_cols[a] / sd_cols[b]
