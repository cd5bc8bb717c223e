"""Posterior mean and standard deviation of the correlation matrix and of the communalities on the GPU
(DCFM_FLAG_CORR, corr.hip, dcfm_get_corr[_cols], dcfm_get_communality).

The reference is built here, in NumPy: the oracle's dense Sigma(s) divided by sqrt(diag x diag) for the state of
every saved iteration, and |Lambda_a|^2 / Sigma(s)_aa (corr_cases.dense_moments) -- the library's own output is
never its own reference.  Bars (corr_cases: derived from the arithmetic, no condition number enters), with
b = (saved/effsamp) (4 (K + 4) + saved) eps: max|C - ref| <= b, max|C2 - ref| <= 2 b, max|SD^2 - var_ref| <= 4 r b
with r = effsamp / saved (the variance is compared, not the SD), the same three for the communalities; normwise the
project's 1e-10 (helpers.rel_err); symmetry, the diagonal and the column stripes exact."""
import ctypes as C
import threading

import numpy as np
import pytest

import corr_cases as cc
import probe_cases as pc
from helpers import STATE_CMP, make_case, rel_err, stacked_draws, state_dict
from oracle import dc_oracle as F

pytestmark = pytest.mark.gpu

MOMENTS = ("mean", "m2", "sd")


def _assert_moments(r, ref, saved, effsamp, what):
    """The stepwise bars on read_all's dict r against dense_moments' ref."""
    Cm, C2, SD = r["mean"], r["m2"], r["sd"]
    H, H2, HSD = r["h"], r["h2"], r["hsd"]
    b, rs = ref["b"], effsamp / saved
    e1, e2 = float(np.max(np.abs(Cm - ref["C"]))), float(np.max(np.abs(C2 - ref["C2"])))
    ev = float(np.max(np.abs(SD * SD - ref["var"])))
    h1, h2 = float(np.max(np.abs(H - ref["H"]))), float(np.max(np.abs(H2 - ref["H2"])))
    hv = float(np.max(np.abs(HSD * HSD - ref["hvar"])))
    print(f"{what}: b {b:.3e}, max|C - ref| {e1:.3e}, max|C2 - ref| {e2:.3e}, max|SD^2 - var| {ev:.3e}, "
          f"max|H - ref| {h1:.3e}, max|H2 - ref| {h2:.3e}, max|HSD^2 - var| {hv:.3e}, "
          f"rel_err {rel_err(Cm, ref['C']):.3e} / {rel_err(C2, ref['C2']):.3e}")
    for M in (Cm, C2, SD):
        assert np.all(np.isfinite(M))
        assert np.array_equal(M, M.T)
    assert e1 <= b, f"{what}: mean off by {e1:.3e}, bound {b:.3e}"
    assert e2 <= 2 * b, f"{what}: second moment off by {e2:.3e}, bound {2 * b:.3e}"
    assert ev <= 4 * rs * b, f"{what}: variance off by {ev:.3e}, bound {4 * rs * b:.3e}"
    assert h1 <= b, f"{what}: communality mean off by {h1:.3e}, bound {b:.3e}"
    assert h2 <= 2 * b, f"{what}: communality second moment off by {h2:.3e}, bound {2 * b:.3e}"
    assert hv <= 4 * rs * b, f"{what}: communality variance off by {hv:.3e}, bound {4 * rs * b:.3e}"
    assert rel_err(Cm, ref["C"]) < 1e-10 and rel_err(C2, ref["C2"]) < 1e-10
    assert rel_err(H, ref["H"]) < 1e-10 and rel_err(H2, ref["H2"]) < 1e-10
    p = Cm.shape[0]
    assert np.array_equal(Cm.diagonal(), np.full(p, saved / effsamp))
    assert np.array_equal(C2.diagonal(), np.full(p, saved / effsamp))
    assert np.array_equal(SD.diagonal(), np.zeros(p))
    assert np.all(np.abs(Cm) <= saved / effsamp + b)      # |R(s)| <= 1 up to the product's rounding
    assert H.shape == H2.shape == HSD.shape == (p,) and np.all(H > 0) and np.all(HSD >= 0)
    c0, nc = r["c0"], r["nc"]
    for f in MOMENTS:
        assert r[f + "_cols"].shape == (p, nc)
        assert np.array_equal(r[f + "_cols"], r[f][:, c0:c0 + nc]), f


@pytest.mark.parametrize("shape,rho", cc.SWEEP)
def test_stepwise_sweep(dcfm, shape, rho):
    """One iteration per run: the reference normalises the state the device held."""
    r = cc.run_corr(dcfm, shape, rho)
    assert r["saved"] == len(r["states"]) == len(pc.SAVED)
    ref = cc.dense_moments(r["states"], rho, pc.EFFSAMP)
    _assert_moments(r, ref, r["saved"], pc.EFFSAMP, f"{shape} rho={rho}")


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


def _everything(smp):
    return {**{w: smp.get_corr(w) for w in MOMENTS}, **{"h" + w: smp.get_communality(w) for w in MOMENTS}}


@pytest.mark.parametrize("K", [6, 5])     # slot starts s*K = 6, 12 (16-byte aligned) and 5, 10 (5: 8-byte only)
def test_batched_flush_in_one_run(dcfm, K):
    """7 saved samples flushed in batches of 3, 3 and 1 by a single run, against the oracle's chain.  The
    device's chain agrees with the oracle's to the project's normwise 1e-10 (the parity tests), not to the
    rounding bound of one product, so the bars are the normwise one on the means and the second moments and,
    on the variances, test_gpu_sigma_moments._check's 1e-10 max|M2_ref|.  The same chain cut into three run
    calls at the flush seams (after iterations 8 and 14: the flush grouping 3 + 3 + 1 is the single call's; a
    run call ends with a flush, so another cut would regroup the sums) gives the single call's bits."""
    n, p, g = 48, 64, 4
    burnin, mcmc, thin = 2, 14, 2
    c = make_case(n, p, g, K, seed=9)
    smp = _injected(dcfm, c, burnin, mcmc, thin, asm_batch=3, corr=True)
    try:
        smp.run(1, burnin + mcmc)
        assert smp.saved_samples() == 7
        one = _everything(smp)
    finally:
        smp.close()
    smp = _injected(dcfm, c, burnin, mcmc, thin, asm_batch=3, corr=True)
    try:
        for first, cnt in ((1, 8), (9, 6), (15, 2)):
            smp.run(first, cnt)
        assert smp.saved_samples() == 7
        cut = _everything(smp)
    finally:
        smp.close()
    for f in one:
        assert one[f].tobytes() == cut[f].tobytes(), f
    sts = _oracle_states(c, burnin, mcmc, thin)
    assert len(sts) == 7
    ref = cc.dense_moments(sts, c["rho"], mcmc / thin)
    e = [rel_err(one["mean"], ref["C"]), rel_err(one["m2"], ref["C2"]), rel_err(one["hmean"], ref["H"]),
         rel_err(one["hm2"], ref["H2"])]
    ev, scale = float(np.max(np.abs(one["sd"] ** 2 - ref["var"]))), float(np.max(np.abs(ref["C2"])))
    hv, hscale = float(np.max(np.abs(one["hsd"] ** 2 - ref["hvar"]))), float(np.max(np.abs(ref["H2"])))
    print(f"batched K={K}: rel_err {e}, max|SD^2 - var| = {ev:.3e} (bar {1e-10 * scale:.3e}), communality "
          f"{hv:.3e} (bar {1e-10 * hscale:.3e})")
    assert max(e) < 1e-10
    assert ev <= 1e-10 * scale and hv <= 1e-10 * hscale
    for w in MOMENTS:
        assert np.array_equal(one[w], one[w].T) and np.all(np.isfinite(one[w])) and np.all(np.isfinite(one["h" + w]))
    assert np.all(one["sd"] >= 0) and np.all(one["hsd"] >= 0)


def test_q8_scaling_and_mid_run(dcfm):
    """thin does not divide mcmc: effsamp = 2.5 while dc:180 saves iterations 2, 4 and 6.  All four accumulators
    carry 1/effsamp as Sigmaout does; before the first saved sample they are all zeros and the SDs are refused."""
    from dcfm_amd import _abi
    n, p, g, K = 30, 40, 4, 3
    burnin, mcmc, thin = 1, 5, 2
    effsamp = mcmc / thin
    c = make_case(n, p, g, K)
    smp = _injected(dcfm, c, burnin, mcmc, thin, corr=True)
    sts = []
    try:
        for it in range(1, burnin + mcmc + 1):
            if not sts:                                           # before any saved sample
                for w in ("mean", "m2"):
                    assert np.array_equal(smp.get_corr(w), np.zeros((p, p)))
                    assert np.array_equal(smp.get_corr_cols(w, 3, 9), np.zeros((p, 9)))
                    assert np.array_equal(smp.get_communality(w), np.zeros(p))
                for call in (lambda: smp.get_corr("sd"), lambda: smp.get_corr_cols("sd", 3, 9),
                             lambda: smp.get_communality("sd")):
                    with pytest.raises(dcfm.DcfmError) as e:
                        call()
                    assert e.value.code == _abi.DCFM_ERR_INVALID and "no saved sample" in str(e.value)
            smp.run(it, 1)
            if not _saved(it, burnin, thin):
                continue
            sts.append(smp.get_state(("Lambda", "omega")))
            assert smp.saved_samples() == len(sts)
            _assert_moments(cc.read_all(smp), cc.dense_moments(sts, c["rho"], effsamp), len(sts), effsamp,
                            f"Q8 after {len(sts)} saved")
        Cm, H = smp.get_corr("mean"), smp.get_communality("mean")
    finally:
        smp.close()
    assert len(sts) == 3 != effsamp
    plain = cc.dense_moments(sts, c["rho"], len(sts))             # the samples' plain means
    assert rel_err(Cm * (effsamp / len(sts)), plain["C"]) < 1e-10
    assert rel_err(H * (effsamp / len(sts)), plain["H"]) < 1e-10
    assert np.array_equal(Cm.diagonal(), np.full(p, 3 / 2.5))


def test_flag_changes_nothing_that_exists(dcfm):
    from dcfm_amd import _abi
    n, p, g, K = 30, 200, 4, 5
    burnin, mcmc, thin = 1, 4, 1
    N = burnin + mcmc
    c = make_case(n, p, g, K, seed=4)
    rest_kw = dict(sigma_m2=True, precision_mean=True, partial_corr=True)
    res = {}
    for key, kw in (("rest", rest_kw), ("all", dict(rest_kw, corr=True)), ("alone", dict(corr=True))):
        smp = _injected(dcfm, c, burnin, mcmc, thin, asm_batch=3, **kw)
        try:
            smp.set_trace(N)
            smp.run(1, N)
            r = {"state": smp.get_state(), "Sig": smp.get_sigma(), "block": smp.sigma_block(), "trace": smp.get_trace()}
            if kw.get("sigma_m2"):
                r["sd"], r["T"] = smp.get_sigma_moment("sd"), smp.get_precision_mean()
                r["pc"] = {w: smp.get_partial_corr(w) for w in MOMENTS}
            if kw.get("corr"):
                r["corr"] = _everything(smp)
                with pytest.raises(dcfm.DcfmError) as e:
                    smp.get_corr_cols("mean", 150, 51)             # past p
                assert e.value.code == _abi.DCFM_ERR_INVALID
                buf = np.zeros((p, 4), order="F")
                for c0, nc in ((-1, 4), (0, -1), (p, 1)):          # a bad column range
                    assert smp.lib.dcfm_get_corr_cols(
                        smp.h, 0, c0, nc, buf.ctypes.data_as(C.POINTER(C.c_double))) == _abi.DCFM_ERR_INVALID, (c0, nc)
                assert smp.lib.dcfm_get_corr(smp.h, 0, None) == _abi.DCFM_ERR_INVALID   # NULL out on rank 0
                assert smp.lib.dcfm_get_corr_cols(smp.h, 0, 0, 4, None) == _abi.DCFM_ERR_INVALID
                assert smp.lib.dcfm_get_communality(smp.h, 0, None) == _abi.DCFM_ERR_INVALID
                for w in (3, -1):                                  # a bad `which`
                    for call in (lambda: smp.get_corr(w), lambda: smp.get_corr_cols(w, 0, 4),
                                 lambda: smp.get_communality(w)):
                        with pytest.raises(dcfm.DcfmError) as e:
                            call()
                        assert e.value.code == _abi.DCFM_ERR_INVALID
            else:
                for call in (smp.get_corr, lambda: smp.get_corr_cols("m2", 0, 8), smp.get_communality):
                    with pytest.raises(dcfm.DcfmError) as e:
                        call()
                    assert e.value.code == _abi.DCFM_ERR_INVALID and "DCFM_FLAG_CORR" in str(e.value)
            if key == "alone":                                     # none of the other accumulators
                for call in (smp.get_precision_mean, lambda: smp.get_sigma_moment("sd"), smp.get_partial_corr):
                    with pytest.raises(dcfm.DcfmError) as e:
                        call()
                    assert e.value.code == _abi.DCFM_ERR_INVALID
            res[key] = r
        finally:
            smp.close()
    rest, al, alone = res["rest"], res["all"], res["alone"]
    for other in (al, alone):
        assert np.array_equal(rest["Sig"], other["Sig"])
        assert rest["trace"].tobytes() == other["trace"].tobytes()
        for f in STATE_CMP:
            assert np.array_equal(rest["state"][f], other["state"][f]), f
    for f in ("sd", "T"):
        assert rest[f].tobytes() == al[f].tobytes(), f
    for w in MOMENTS:
        assert rest["pc"][w].tobytes() == al["pc"][w].tobytes(), w
    for f in al["corr"]:
        assert al["corr"][f].tobytes() == alone["corr"][f].tobytes(), f
    assert np.any(al["corr"]["sd"] != 0) and np.any(al["corr"]["hsd"] != 0)
    five = rest["block"]["bytes"]                                  # Sigma, Sigma2, Prec, PC, PC2
    assert five % 5 == 0
    unit = five // 5
    assert al["block"]["bytes"] == five + 2 * unit and alone["block"]["bytes"] == 3 * unit
    # the contrast with the plug-in of Sigmaout (informational): two different quantities
    gap = float(np.max(np.abs(al["corr"]["mean"] * ((mcmc / thin) / mcmc) - dcfm.correlation(al["Sig"]))))
    print(f"max |C_mean effsamp / saved - correlation(Sigmaout)| = {gap:.3e}")
    assert np.isfinite(gap)


def test_two_ranks_loopback(dcfm):
    """Two ranks on one device (in-process loopback): p = 300, the three tile rows split [0, 2) | [2, 3).  Each
    rank scales all 300 rows of the gathered batch.  Rank 0's gathered moments are bitwise the one-rank run's
    (same tiles, same scales, same arithmetic); both ranks hold the same communalities, bit for bit."""
    from sharded_protocol import sigma_split
    n, p, g, K, nr = 32, 300, 4, 6, 2
    burnin, mcmc, thin, asm_batch = 1, 4, 1, 3
    N = burnin + mcmc
    assert sigma_split(-(-p // 128), nr) == [0, 2, 3]
    c = make_case(n, p, g, K, seed=13)
    G = g // nr
    draws = stacked_draws(c["src"], 1, N)
    smps = [dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], burnin, mcmc, thin, inject_draws=True, nranks=nr, rank=r,
                         device=0, asm_batch=asm_batch, corr=True) for r in range(nr)]
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
                out[r] = {w: smps[r].get_corr(w) for w in MOMENTS}
                out[r]["cols"] = smps[r].get_corr_cols("sd", 100, 150)
                out[r]["block"] = smps[r].sigma_block()
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
            for w in MOMENTS:
                out[r]["h" + w] = smps[r].get_communality(w)
    finally:
        for smp in smps:
            smp.close()
    assert (out[1]["block"]["row0"], out[1]["block"]["row1"]) == (256, 300)
    assert all(out[1][f] is None for f in MOMENTS + ("cols",))          # rank 1 passed NULL
    one = _injected(dcfm, c, burnin, mcmc, thin, asm_batch=asm_batch, corr=True)
    try:
        one.run(1, N)
        ref1 = _everything(one)
        total = one.sigma_block()["bytes"]
    finally:
        one.close()
    assert out[0]["block"]["bytes"] + out[1]["block"]["bytes"] == total
    for w in MOMENTS:
        assert out[0][w].tobytes() == ref1[w].tobytes(), w
        assert out[0]["h" + w].tobytes() == out[1]["h" + w].tobytes() == ref1["h" + w].tobytes(), w
    assert np.array_equal(out[0]["cols"], ref1["sd"][:, 100:250])
    ref = cc.dense_moments(_oracle_states(c, burnin, mcmc, thin), c["rho"], mcmc / thin)
    assert rel_err(out[0]["mean"], ref["C"]) < 1e-10 and rel_err(out[0]["m2"], ref["C2"]) < 1e-10
    assert rel_err(out[1]["hmean"], ref["H"]) < 1e-10 and rel_err(out[1]["hm2"], ref["H2"]) < 1e-10


def test_same_bits_on_a_second_run(dcfm):
    shape = (37, 300, 3, 7)
    a = cc.run_corr(dcfm, shape, states=False)
    b = cc.run_corr(dcfm, shape, states=False)
    for f in ("mean", "m2", "sd", "mean_cols", "m2_cols", "sd_cols", "h", "h2", "hsd"):
        assert a[f].tobytes() == b[f].tobytes(), f
    assert np.any(a["sd"] != 0) and np.any(a["hsd"] != 0)


def test_driver_returns_the_correlations(dcfm):
    import oracle
    from dcfm_amd import driver as D
    n, p, g, K, rho = 40, 48, 4, 3, 0.5
    burnin, mcmc, thin, seed = 2, 6, 2, 31
    Y, _ = oracle.synth.make_data(n, p + 2, k0=4, zero_cols=2)
    p_orig = Y.shape[1]
    S, R, info = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, rho, seed=seed, return_corr=True,
                                    return_info=True)
    S2, SD, PR, R2, pcs = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, rho, seed=seed, return_sd=True,
                                             return_partial=True, return_corr=True, n_components=2)
    plain = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, rho, seed=seed)
    keys = ("mean", "sd", "communality", "communality_sd")
    assert set(R) == set(keys) and R["mean"].shape == R["sd"].shape == (p_orig, p_orig)
    assert R["communality"].shape == R["communality_sd"].shape == (p_orig,)
    assert isinstance(info, dict) and set(PR) == {"mean", "sd"} and set(pcs) >= {"values", "vectors"}
    assert SD.shape == S.shape
    assert np.array_equal(S, plain) and np.array_equal(S2, plain)
    for f in keys:
        assert R[f].tobytes() == R2[f].tobytes(), f
    # the same chain at the Sampler level
    nn, pk, P, Kk, keep = D.preprocess_device(Y, g, K * g)
    smp = dcfm.Sampler(nn, P, g, Kk, rho, burnin, mcmc, thin, seed=seed, corr=True)
    try:
        smp.set_data_raw(Y, D.shard_columns(keep, info["varind"], P, 0, g))
        smp.init_state()
        smp.run(1, burnin + mcmc)
        assert np.array_equal(smp.get_sigma(), S)
        Rm, Rs = smp.get_corr("mean"), smp.get_corr("sd")
        hm, hs = smp.get_communality("mean"), smp.get_communality("sd")
    finally:
        smp.close()
    kv = (info["keep"], info["varind"], p_orig)
    assert R["mean"].tobytes() == dcfm.unpermute_corr(Rm, *kv).tobytes()
    assert R["sd"].tobytes() == dcfm.unpermute_corr(Rs, *kv, diag=0.0).tobytes()
    assert R["communality"].tobytes() == dcfm.unpermute_communality(hm, *kv).tobytes()
    assert R["communality_sd"].tobytes() == dcfm.unpermute_communality(hs, *kv).tobytes()
    cols = D.output_columns(info["keep"], info["varind"])
    assert cols.size < p_orig                                   # a column was dropped
    a, b = 3, 17
    assert R["mean"][cols[a], cols[b]] == Rm[a, b] and R["sd"][cols[a], cols[b]] == Rs[a, b]
    assert R["communality"][cols[a]] == hm[a] and 0 < hm[a] < 1
    dropped = np.setdiff1d(np.arange(p_orig), cols)
    assert np.isnan(R["mean"][dropped[0], cols[0]]) and R["mean"][dropped[0], dropped[0]] == 1.0
    assert np.isnan(R["sd"][dropped[0], cols[0]]) and R["sd"][dropped[0], dropped[0]] == 0.0
    assert np.isnan(R["communality"][dropped[0]]) and np.isnan(R["communality_sd"][dropped[0]])
    e = dcfm.partial_correlation_edges(R["mean"], R["sd"])
    assert e["edges"].shape == (p_orig, p_orig) and not e["edges"][dropped].any()
