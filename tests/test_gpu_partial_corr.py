"""Posterior mean and standard deviation of the partial correlations on the GPU (DCFM_FLAG_PARTIAL_CORR,
partial_corr.hip, dcfm_get_partial_corr[_cols]).

The reference is built here, in NumPy: the partial correlations of np.linalg.inv of the oracle's Sigma(s) for
the state of every saved iteration (partial_corr_cases.dense_moments) -- the library's own output is never its
own reference.  Bars, with b = (1/effsamp) sum_s 8 (P + 2K + g) eps kappa_s (every kappa_s must stay below 1e6):
max|PC - ref| <= b, max|PC2 - ref| <= 2 b (|t^2 - t_ref^2| <= 2 |t| err), max|SD^2 - var_ref| <= 4 r b with
r = effsamp / saved (the variance is compared, not the SD); normwise the project's 1e-10 (helpers.rel_err);
symmetry, the diagonal and the column stripes exact."""
import ctypes as C
import threading

import numpy as np
import pytest

import partial_corr_cases as rc
import probe_cases as pc
from helpers import STATE_CMP, make_case, rel_err, stacked_draws, state_dict
from oracle import dc_oracle as F

pytestmark = pytest.mark.gpu


def _assert_moments(r, ref, saved, effsamp, what):
    """The stepwise bars on read_all's dict r against dense_moments' ref."""
    PC, PC2, SD = r["mean"], r["m2"], r["sd"]
    b, rs = ref["b"], effsamp / saved
    e1, e2 = float(np.max(np.abs(PC - ref["PC"]))), float(np.max(np.abs(PC2 - ref["PC2"])))
    ev = float(np.max(np.abs(SD * SD - ref["var"])))
    print(f"{what}: kappa max {max(ref['kappa']):.3e}, b {b:.3e}, max|PC - ref| {e1:.3e}, max|PC2 - ref| {e2:.3e}, "
          f"max|SD^2 - var| {ev:.3e}, rel_err {rel_err(PC, ref['PC']):.3e} / {rel_err(PC2, ref['PC2']):.3e}")
    for M in (PC, PC2, SD):
        assert np.all(np.isfinite(M))
        assert np.array_equal(M, M.T)
    assert max(ref["kappa"]) <= 1e6, f"{what}: kappa {max(ref['kappa']):.3e}"
    assert e1 <= b, f"{what}: mean off by {e1:.3e}, bound {b:.3e}"
    assert e2 <= 2 * b, f"{what}: second moment off by {e2:.3e}, bound {2 * b:.3e}"
    assert ev <= 4 * rs * b, f"{what}: variance off by {ev:.3e}, bound {4 * rs * b:.3e}"
    assert rel_err(PC, ref["PC"]) < 1e-10 and rel_err(PC2, ref["PC2"]) < 1e-10
    p = PC.shape[0]
    assert np.array_equal(PC.diagonal(), np.full(p, saved / effsamp))
    assert np.array_equal(SD.diagonal(), np.zeros(p))
    assert np.all(np.abs(PC) <= saved / effsamp)
    c0, nc = r["c0"], r["nc"]
    for f in ("mean", "m2", "sd"):
        assert r[f + "_cols"].shape == (p, nc)
        assert np.array_equal(r[f + "_cols"], r[f][:, c0:c0 + nc]), f


@pytest.mark.parametrize("shape,rho", rc.SWEEP)
def test_stepwise_sweep(dcfm, shape, rho):
    """One iteration per run: the reference inverts the state the device held."""
    r = rc.run_pc(dcfm, shape, rho)
    assert r["saved"] == len(r["states"]) == len(pc.SAVED)
    ref = rc.dense_moments(r["states"], rho, pc.EFFSAMP)
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


@pytest.mark.parametrize("K", [6, 5])     # slot starts s*K = 6, 12 (16-byte aligned) and 5, 10 (5: 8-byte only)
def test_batched_flush_in_one_run(dcfm, K):
    """7 saved samples flushed in batches of 3, 3 and 1 by a single run, against the oracle's chain.  The
    device's chain agrees with the oracle's to the project's normwise 1e-10 (the parity tests), not to the
    rounding bound of one inversion, so the bars are the normwise one on the mean and the second moment and,
    on the variance, test_gpu_sigma_moments._check's 1e-10 max|M2_ref|."""
    n, p, g = 48, 64, 4
    burnin, mcmc, thin = 2, 14, 2
    c = make_case(n, p, g, K, seed=9)
    smp = _injected(dcfm, c, burnin, mcmc, thin, asm_batch=3, partial_corr=True)
    try:
        smp.run(1, burnin + mcmc)
        assert smp.saved_samples() == 7
        PC, PC2, SD = (smp.get_partial_corr(w) for w in ("mean", "m2", "sd"))
    finally:
        smp.close()
    sts = _oracle_states(c, burnin, mcmc, thin)
    assert len(sts) == 7
    ref = rc.dense_moments(sts, c["rho"], mcmc / thin)
    e1, e2 = rel_err(PC, ref["PC"]), rel_err(PC2, ref["PC2"])
    ev, scale = float(np.max(np.abs(SD * SD - ref["var"]))), float(np.max(np.abs(ref["PC2"])))
    print(f"batched K={K}: kappa max {max(ref['kappa']):.3e}, rel_err {e1:.3e} / {e2:.3e}, "
          f"max|SD^2 - var| = {ev:.3e} (bar {1e-10 * scale:.3e})")
    assert max(ref["kappa"]) <= 1e6 and e1 < 1e-10 and e2 < 1e-10
    assert ev <= 1e-10 * scale
    for M in (PC, PC2, SD):
        assert np.array_equal(M, M.T) and np.all(np.isfinite(M))
    assert np.all(SD >= 0)


def test_q8_scaling_and_mid_run(dcfm):
    """thin does not divide mcmc: effsamp = 2.5 while dc:180 saves iterations 2, 4 and 6.  Both moments carry
    1/effsamp as Sigmaout does; before the first saved sample they are all zeros and the SD is refused."""
    from dcfm_amd import _abi
    n, p, g, K = 30, 40, 4, 3
    burnin, mcmc, thin = 1, 5, 2
    effsamp = mcmc / thin
    c = make_case(n, p, g, K)
    smp = _injected(dcfm, c, burnin, mcmc, thin, partial_corr=True)
    sts = []
    try:
        for it in range(1, burnin + mcmc + 1):
            if not sts:                                           # before any saved sample
                for w in ("mean", "m2"):
                    assert np.array_equal(smp.get_partial_corr(w), np.zeros((p, p)))
                    assert np.array_equal(smp.get_partial_corr_cols(w, 3, 9), np.zeros((p, 9)))
                for call in (lambda: smp.get_partial_corr("sd"), lambda: smp.get_partial_corr_cols("sd", 3, 9)):
                    with pytest.raises(dcfm.DcfmError) as e:
                        call()
                    assert e.value.code == _abi.DCFM_ERR_INVALID and "no saved sample" in str(e.value)
            smp.run(it, 1)
            if not _saved(it, burnin, thin):
                continue
            sts.append(smp.get_state(("Lambda", "omega")))
            assert smp.saved_samples() == len(sts)
            _assert_moments(rc.read_all(smp), rc.dense_moments(sts, c["rho"], effsamp), len(sts), effsamp,
                            f"Q8 after {len(sts)} saved")
        PC = smp.get_partial_corr("mean")
    finally:
        smp.close()
    assert len(sts) == 3 != effsamp
    plain = rc.dense_moments(sts, c["rho"], len(sts))["PC"]       # the samples' plain mean
    assert rel_err(PC * (effsamp / len(sts)), plain) < 1e-10
    assert np.array_equal(PC.diagonal(), np.full(p, 3 / 2.5))


def test_flag_changes_nothing_that_exists(dcfm):
    from dcfm_amd import _abi
    n, p, g, K = 30, 200, 4, 5
    burnin, mcmc, thin = 1, 4, 1
    N = burnin + mcmc
    c = make_case(n, p, g, K, seed=4)
    res = {}
    for key, kw in (("rest", dict(sigma_m2=True, precision_mean=True)),
                    ("all", dict(sigma_m2=True, precision_mean=True, partial_corr=True)),
                    ("alone", dict(partial_corr=True))):
        smp = _injected(dcfm, c, burnin, mcmc, thin, asm_batch=3, **kw)
        try:
            smp.set_trace(N)
            smp.run(1, N)
            r = {"state": smp.get_state(), "Sig": smp.get_sigma(), "block": smp.sigma_block(), "trace": smp.get_trace()}
            if kw.get("sigma_m2"):
                r["sd"], r["T"] = smp.get_sigma_moment("sd"), smp.get_precision_mean()
            if kw.get("partial_corr"):
                r["pc"] = {w: smp.get_partial_corr(w) for w in ("mean", "m2", "sd")}
                with pytest.raises(dcfm.DcfmError) as e:
                    smp.get_partial_corr_cols("mean", 150, 51)     # past p
                assert e.value.code == _abi.DCFM_ERR_INVALID
                buf = np.zeros((p, 4), order="F")
                for c0, nc in ((-1, 4), (0, -1), (p, 1)):          # a bad column range
                    assert smp.lib.dcfm_get_partial_corr_cols(
                        smp.h, 0, c0, nc, buf.ctypes.data_as(C.POINTER(C.c_double))) == _abi.DCFM_ERR_INVALID, (c0, nc)
                assert smp.lib.dcfm_get_partial_corr(smp.h, 0, None) == _abi.DCFM_ERR_INVALID   # NULL out on rank 0
                assert smp.lib.dcfm_get_partial_corr_cols(smp.h, 0, 0, 4, None) == _abi.DCFM_ERR_INVALID
                for w in (3, -1):                                  # a bad `which`
                    with pytest.raises(dcfm.DcfmError) as e:
                        smp.get_partial_corr(w)
                    assert e.value.code == _abi.DCFM_ERR_INVALID
            else:
                for call in (smp.get_partial_corr, lambda: smp.get_partial_corr_cols("m2", 0, 8)):
                    with pytest.raises(dcfm.DcfmError) as e:
                        call()
                    assert e.value.code == _abi.DCFM_ERR_INVALID and "DCFM_FLAG_PARTIAL_CORR" in str(e.value)
            if key == "alone":                                     # no precision accumulator, no second moment
                for call in (smp.get_precision_mean, lambda: smp.get_sigma_moment("sd")):
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
    for w in ("mean", "m2", "sd"):
        assert al["pc"][w].tobytes() == alone["pc"][w].tobytes(), w
    assert np.any(al["pc"]["mean"] != 0) and np.any(al["pc"]["sd"] != 0)
    three = rest["block"]["bytes"]
    assert three % 3 == 0 and al["block"]["bytes"] == three // 3 * 5 and alone["block"]["bytes"] == three
    # the contrast with the plug-in of the precision mean (informational): two different quantities
    plug = dcfm.partial_correlations(al["T"])
    gap = float(np.max(np.abs(al["pc"]["mean"] * ((mcmc / thin) / mcmc) - plug)))
    print(f"max |PC_mean effsamp / saved - partial_correlations(Theta)| = {gap:.3e}")
    assert np.isfinite(gap)


def test_two_ranks_loopback(dcfm):
    """Two ranks on one device (in-process loopback): p = 300, the three tile rows split [0, 2) | [2, 3).  Each
    rank forms and scales the factor panels of all four shards.  Rank 0's gathered moments are bitwise the
    one-rank run's (same tiles, same factor bytes, same arithmetic)."""
    from sharded_protocol import sigma_split
    n, p, g, K, nr = 32, 300, 4, 6, 2
    burnin, mcmc, thin, asm_batch = 1, 4, 1, 3
    N = burnin + mcmc
    assert sigma_split(-(-p // 128), nr) == [0, 2, 3]
    c = make_case(n, p, g, K, seed=13)
    G = g // nr
    draws = stacked_draws(c["src"], 1, N)
    smps = [dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], burnin, mcmc, thin, inject_draws=True, nranks=nr, rank=r,
                         device=0, asm_batch=asm_batch, partial_corr=True) for r in range(nr)]
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
                out[r] = {w: smps[r].get_partial_corr(w) for w in ("mean", "m2", "sd")}
                out[r]["cols"] = smps[r].get_partial_corr_cols("sd", 100, 150)
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
    finally:
        for smp in smps:
            smp.close()
    assert (out[1]["block"]["row0"], out[1]["block"]["row1"]) == (256, 300)
    assert all(out[1][f] is None for f in ("mean", "m2", "sd", "cols"))       # rank 1 passed NULL
    one = _injected(dcfm, c, burnin, mcmc, thin, asm_batch=asm_batch, partial_corr=True)
    try:
        one.run(1, N)
        ref1 = {w: one.get_partial_corr(w) for w in ("mean", "m2", "sd")}
        total = one.sigma_block()["bytes"]
    finally:
        one.close()
    assert out[0]["block"]["bytes"] + out[1]["block"]["bytes"] == total
    for w in ("mean", "m2", "sd"):
        assert out[0][w].tobytes() == ref1[w].tobytes(), w
    assert np.array_equal(out[0]["cols"], ref1["sd"][:, 100:250])
    ref = rc.dense_moments(_oracle_states(c, burnin, mcmc, thin), c["rho"], mcmc / thin)
    assert rel_err(out[0]["mean"], ref["PC"]) < 1e-10 and rel_err(out[0]["m2"], ref["PC2"]) < 1e-10


def test_same_bits_on_a_second_run(dcfm):
    shape = (37, 300, 3, 7)
    a = rc.run_pc(dcfm, shape, states=False)
    b = rc.run_pc(dcfm, shape, states=False)
    for f in ("mean", "m2", "sd", "mean_cols", "m2_cols", "sd_cols"):
        assert a[f].tobytes() == b[f].tobytes(), f
    assert np.any(a["sd"] != 0)


def test_driver_returns_the_partial_correlations(dcfm):
    import oracle
    from dcfm_amd import driver as D
    n, p, g, K, rho = 40, 48, 4, 3, 0.5
    burnin, mcmc, thin, seed = 2, 6, 2, 31
    Y, _ = oracle.synth.make_data(n, p + 2, k0=4, zero_cols=2)
    p_orig = Y.shape[1]
    S, R, info = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, rho, seed=seed, return_partial=True,
                                    return_info=True)
    S2, SD, T, R2, pcs = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, rho, seed=seed, return_sd=True,
                                            return_precision=True, return_partial=True, n_components=2)
    plain = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, rho, seed=seed)
    assert set(R) == {"mean", "sd"} and R["mean"].shape == R["sd"].shape == (p_orig, p_orig)
    assert isinstance(info, dict) and set(pcs) >= {"values", "vectors"} and SD.shape == T.shape == S.shape
    assert np.array_equal(S, plain) and np.array_equal(S2, plain)
    for f in ("mean", "sd"):
        assert R[f].tobytes() == R2[f].tobytes(), f
    # the same chain at the Sampler level
    nn, pk, P, Kk, keep = D.preprocess_device(Y, g, K * g)
    smp = dcfm.Sampler(nn, P, g, Kk, rho, burnin, mcmc, thin, seed=seed, partial_corr=True)
    try:
        smp.set_data_raw(Y, D.shard_columns(keep, info["varind"], P, 0, g))
        smp.init_state()
        smp.run(1, burnin + mcmc)
        assert np.array_equal(smp.get_sigma(), S)
        Rm, Rs = smp.get_partial_corr("mean"), smp.get_partial_corr("sd")
    finally:
        smp.close()
    assert R["mean"].tobytes() == dcfm.unpermute_partial(Rm, info["keep"], info["varind"], p_orig).tobytes()
    assert R["sd"].tobytes() == dcfm.unpermute_partial(Rs, info["keep"], info["varind"], p_orig, diag=0.0).tobytes()
    cols = D.output_columns(info["keep"], info["varind"])
    assert cols.size < p_orig                                   # a column was dropped
    a, b = 3, 17
    assert R["mean"][cols[a], cols[b]] == Rm[a, b] and R["sd"][cols[a], cols[b]] == Rs[a, b]
    dropped = np.setdiff1d(np.arange(p_orig), cols)
    assert np.isnan(R["mean"][dropped[0], cols[0]]) and R["mean"][dropped[0], dropped[0]] == 1.0
    assert np.isnan(R["sd"][dropped[0], cols[0]]) and R["sd"][dropped[0], dropped[0]] == 0.0
    e = dcfm.partial_correlation_edges(R["mean"], R["sd"])
    assert e["edges"].shape == (p_orig, p_orig) and not e["edges"][dropped].any()
