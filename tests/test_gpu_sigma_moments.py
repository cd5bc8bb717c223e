"""Posterior second moment and standard deviation of Sigma's entries (DCFM_FLAG_SIGMA_M2,
k_assemble_m2, dcfm_get_sigma_moment[_cols]).

The reference is built here, in NumPy, from oracle.dc_oracle.assemble_sample applied to the
state of every saved iteration (dc:180-192) — the library's own moment output is never its
own reference:
    M2_ref  = (1/effsamp) sum_s Sigma(s)**2                     (effsamp = mcmc/thin, quirk Q8)
    var_ref = population variance of the saved Sigma(s), entry by entry.
Bars: M2 normwise to the project's 1e-10 (helpers.rel_err); SD**2 against var_ref to the
absolute 1e-10 max|M2_ref| (the square root is ill-conditioned at 0, so the variance is compared,
absolutely); symmetry exact, as the suite asks of Sigmaout.
"""
import threading
from types import SimpleNamespace

import numpy as np
import pytest

from helpers import STATE_CMP, make_case, rel_err, stacked_draws, state_dict
from oracle import dc_oracle as F

pytestmark = pytest.mark.gpu


def _saved(it, burnin, thin):
    return it % thin == 0 and it > burnin                          # dc:180


class _Ref:
    """Host accumulation of the saved samples' Sigma(s)."""

    def __init__(self, effsamp):
        self.effsamp, self.samples = effsamp, []

    def add(self, Lambda, omega, rho):
        self.samples.append(F.assemble_sample(SimpleNamespace(Lambda=np.asarray(Lambda), omega=np.asarray(omega)),
                                              rho))

    @property
    def m2(self):
        return sum(S * S for S in self.samples) / self.effsamp

    @property
    def mean(self):
        return sum(self.samples) / self.effsamp

    @property
    def var(self):
        mu = sum(self.samples) / len(self.samples)
        return sum((S - mu) ** 2 for S in self.samples) / len(self.samples)


def _check(M2, SD, ref, label=""):
    m2_ref = ref.m2
    scale = float(np.max(np.abs(m2_ref)))
    e_m2 = rel_err(M2, m2_ref)
    e_var = float(np.max(np.abs(SD * SD - ref.var)))
    print(f"{label} rel_err(M2) = {e_m2:.3e}, max|SD^2 - var| = {e_var:.3e} (bar {1e-10 * scale:.3e})")
    assert e_m2 < 1e-10
    assert e_var <= 1e-10 * scale
    assert np.array_equal(M2, M2.T) and np.array_equal(SD, SD.T)
    assert np.all(SD >= 0) and np.all(np.isfinite(SD))


def _injected(dcfm, c, burnin, mcmc, thin, **kw):
    """A sampler at the case's initial state with injected draws for every iteration."""
    N = burnin + mcmc
    smp = dcfm.Sampler(c["n"], c["P"], c["g"], c["K"], c["rho"], burnin, mcmc, thin, inject_draws=True, **kw)
    smp.set_data(c["Yd"])
    smp.set_state({f: v for f, v in state_dict(c["st"]).items() if f != "eta"})
    smp.set_draws(stacked_draws(c["src"], 1, N), 1, N)
    return smp


# (n, p, g, K)
SWEEP = [
    (30, 48, 4, 5),        # one partial tile, K odd
    (30, 36, 3, 1),        # K = 1: slots one column wide
    (37, 300, 3, 7),       # ragged P = 100: shard edges inside tiles, mixed tiles
    (64, 384, 3, 30),      # P = 128: tile (1, 0) purely cross-shard, diagonal tiles purely same-shard; c3's K
    (50, 128, 2, 32),      # K = 32, aligned
    (40, 99, 3, 33),       # the wide-K state layout feeding the same Lb
    (32, 1152, 9, 3),      # 9 tile rows: crosses an 8 x 8 supertile
]


@pytest.mark.parametrize("n,p,g,K", SWEEP)
def test_second_moment_stepwise(dcfm, n, p, g, K):
    """Generated draws, one iteration per run: the reference squares the state the device held."""
    burnin, mcmc, thin = 1, 3, 1
    N = burnin + mcmc
    c = make_case(n, p, g, K, seed=5)
    ref = _Ref(mcmc / thin)
    smp = dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], burnin, mcmc, thin, seed=21, sigma_m2=True)
    try:
        smp.set_data(c["Yd"])
        smp.set_state({f: v for f, v in state_dict(c["st"]).items() if f != "eta"})
        for it in range(1, N + 1):
            smp.run(it, 1)
            if _saved(it, burnin, thin):
                s = smp.get_state(("Lambda", "omega"))
                ref.add(s["Lambda"], s["omega"], c["rho"])
        assert smp.saved_samples() == len(ref.samples) >= 3
        M2, SD = smp.get_sigma_moment("m2"), smp.get_sigma_moment("sd")
        mean = smp.get_sigma_moment("mean")
        assert np.array_equal(mean, smp.get_sigma())
    finally:
        smp.close()
    assert rel_err(mean, ref.mean) < 1e-10
    _check(M2, SD, ref, f"{(n, p, g, K)}")


@pytest.mark.parametrize("K", [6, 5])     # slot starts s*K = 6, 12 (16-byte aligned) and 5, 10 (5: 8-byte only)
def test_batched_flush_in_one_run(dcfm, K):
    """7 saved samples flushed in batches of 3, 3 and 1 by a single run."""
    n, p, g = 48, 64, 4
    burnin, mcmc, thin = 2, 14, 2
    N = burnin + mcmc
    c = make_case(n, p, g, K, seed=9)
    smp = _injected(dcfm, c, burnin, mcmc, thin, asm_batch=3, sigma_m2=True)
    try:
        smp.run(1, N)
        assert smp.saved_samples() == 7
        M2, SD = smp.get_sigma_moment("m2"), smp.get_sigma_moment("sd")
        S = smp.get_sigma()
    finally:
        smp.close()
    ref, st = _Ref(mcmc / thin), c["st"].copy()
    for it in range(1, N + 1):
        F.run_chain(c["Yd"], st, c["rho"], c["hyper"], c["src"].iteration, it, 1, burnin, mcmc, thin)
        if _saved(it, burnin, thin):
            ref.add(st.Lambda, st.omega, c["rho"])
    assert len(ref.samples) == 7
    assert rel_err(S, ref.mean) < 1e-10
    _check(M2, SD, ref, f"batched K={K}")


def test_q8_scaling_and_mid_run(dcfm):
    """thin does not divide mcmc (tests/test_gpu_parity.py's thin_not_dividing shape): effsamp =
    2.5 while dc:180 saves iterations 2, 4 and 6.  M2 carries 1/effsamp as the mean does; SD is
    the population sd of the samples saved so far, whatever effsamp is."""
    n, p, g, K = 30, 40, 4, 3
    burnin, mcmc, thin = 1, 5, 2
    N = burnin + mcmc
    effsamp = mcmc / thin
    c = make_case(n, p, g, K)
    ref, st = _Ref(effsamp), c["st"].copy()
    smp = _injected(dcfm, c, burnin, mcmc, thin, sigma_m2=True)
    try:
        from dcfm_amd import _abi
        for it in range(1, N + 1):
            if not ref.samples:                                   # before any saved sample
                with pytest.raises(dcfm.DcfmError) as e:
                    smp.get_sigma_moment("sd")
                assert e.value.code == _abi.DCFM_ERR_INVALID
                assert np.array_equal(smp.get_sigma_moment("m2"), np.zeros((p, p)))
            smp.run(it, 1)
            F.run_chain(c["Yd"], st, c["rho"], c["hyper"], c["src"].iteration, it, 1, burnin, mcmc, thin)
            if not _saved(it, burnin, thin):
                continue
            ref.add(st.Lambda, st.omega, c["rho"])
            assert smp.saved_samples() == len(ref.samples)
            M2, SD = smp.get_sigma_moment("m2"), smp.get_sigma_moment("sd")
            _check(M2, SD, ref, f"Q8 after {len(ref.samples)} saved")
            if len(ref.samples) == 1:                             # one sample: no spread
                assert float(np.max(SD * SD)) <= 1e-12 * float(np.max(np.abs(M2)))
        assert len(ref.samples) == sum(_saved(it, burnin, thin) for it in range(1, N + 1)) != effsamp
        # the 1/effsamp scaling: M2 times effsamp / saved is the samples' plain mean square
        plain = sum(S * S for S in ref.samples) / len(ref.samples)
        assert rel_err(M2 * (effsamp / len(ref.samples)), plain) < 1e-10
    finally:
        smp.close()


def test_flag_changes_nothing_that_exists(dcfm):
    n, p, g, K = 30, 200, 4, 5
    burnin, mcmc, thin = 1, 4, 1
    N = burnin + mcmc
    c = make_case(n, p, g, K, seed=4)
    from dcfm_amd import _abi
    res = {}
    for on in (False, True):
        smp = _injected(dcfm, c, burnin, mcmc, thin, asm_batch=3, sigma_m2=on)
        try:
            smp.run(1, N)
            r = {"state": smp.get_state(), "Sig": smp.get_sigma(), "block": smp.sigma_block(),
                 "mean": smp.get_sigma_moment("mean"), "mean_cols": smp.get_sigma_moment_cols("mean", 37, 70),
                 "cols": smp.get_sigma_cols(37, 70)}
            if on:
                r["m2"] = smp.get_sigma_moment("m2")
                r["m2_cols"] = smp.get_sigma_moment_cols("m2", 37, 70)     # starts and ends off a 32 boundary
                r["sd_cols"] = smp.get_sigma_moment_cols(_abi.DCFM_SIGMA_SD, 101, 99)
                r["sd"] = smp.get_sigma_moment("sd")
                with pytest.raises(dcfm.DcfmError) as e:
                    smp.get_sigma_moment_cols("m2", 150, 51)               # past p
                assert e.value.code == _abi.DCFM_ERR_INVALID
                with pytest.raises(dcfm.DcfmError) as e:
                    smp.get_sigma_moment(3)
                assert e.value.code == _abi.DCFM_ERR_INVALID
            else:
                for w in ("m2", "sd"):
                    with pytest.raises(dcfm.DcfmError) as e:
                        smp.get_sigma_moment(w)
                    assert e.value.code == _abi.DCFM_ERR_INVALID and "DCFM_FLAG_SIGMA_M2" in str(e.value)
                    with pytest.raises(dcfm.DcfmError) as e:
                        smp.get_sigma_moment_cols(w, 0, 8)
                    assert e.value.code == _abi.DCFM_ERR_INVALID
            res[on] = r
        finally:
            smp.close()
    off, on = res[False], res[True]
    assert np.array_equal(off["Sig"], on["Sig"])
    for f in STATE_CMP:
        assert np.array_equal(off["state"][f], on["state"][f]), f
    for r in (off, on):
        assert np.array_equal(r["mean"], r["Sig"])
        assert np.array_equal(r["mean_cols"], r["cols"]) and np.array_equal(r["cols"], r["Sig"][:, 37:107])
    assert np.array_equal(on["m2_cols"], on["m2"][:, 37:107])
    assert np.array_equal(on["sd_cols"], on["sd"][:, 101:200])
    assert on["block"]["bytes"] == 2 * off["block"]["bytes"] > 0
    assert (on["block"]["row0"], on["block"]["row1"]) == (off["block"]["row0"], off["block"]["row1"])


def test_two_ranks_loopback(dcfm):
    """Two ranks on one device (in-process loopback): 3 tile rows split [0, 2) | [2, 3), so rank 1
    accumulates from T0 = 2 and the per-sample omega travels in the flush's all-gather.  Rank 0's
    gathered M2 and SD are bitwise the one-rank run's (same tiles, same arithmetic), the standard
    tests/test_gpu_loopback.py holds Sigmaout to."""
    from sharded_protocol import sigma_split
    n, p, g, K, nr = 32, 384, 4, 6, 2
    burnin, mcmc, thin, asm_batch = 1, 4, 1, 3
    N = burnin + mcmc
    assert sigma_split(-(-p // 128), nr) == [0, 2, 3]
    c = make_case(n, p, g, K, seed=13)
    G = g // nr
    draws = stacked_draws(c["src"], 1, N)
    smps = [dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], burnin, mcmc, thin, inject_draws=True, nranks=nr, rank=r,
                         device=0, asm_batch=asm_batch, sigma_m2=True) for r in range(nr)]
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
                out[r] = {"Sig": smps[r].get_sigma(), "m2": smps[r].get_sigma_moment("m2"),
                          "sd": smps[r].get_sigma_moment("sd"),
                          "sd_cols": smps[r].get_sigma_moment_cols("sd", 100, 200),
                          "block": smps[r].sigma_block()}
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
    assert all(out[1][f] is None for f in ("Sig", "m2", "sd", "sd_cols"))
    one = _injected(dcfm, c, burnin, mcmc, thin, asm_batch=asm_batch, sigma_m2=True)
    try:
        one.run(1, N)
        ref1 = {"Sig": one.get_sigma(), "m2": one.get_sigma_moment("m2"), "sd": one.get_sigma_moment("sd")}
        total = one.sigma_block()["bytes"]
    finally:
        one.close()
    assert out[0]["block"]["bytes"] + out[1]["block"]["bytes"] == total
    for f in ("Sig", "m2", "sd"):
        assert np.array_equal(out[0][f], ref1[f]), f
    assert np.array_equal(out[0]["sd_cols"], ref1["sd"][:, 100:300])
    # and against the oracle's samples
    ref, st = _Ref(mcmc / thin), c["st"].copy()
    for it in range(1, N + 1):
        F.run_chain(c["Yd"], st, c["rho"], c["hyper"], c["src"].iteration, it, 1, burnin, mcmc, thin)
        if _saved(it, burnin, thin):
            ref.add(st.Lambda, st.omega, c["rho"])
    _check(out[0]["m2"], out[0]["sd"], ref, "two ranks")


def test_driver_returns_the_standard_deviation(dcfm):
    import oracle
    from dcfm_amd import driver as D
    n, p, g, K, rho = 40, 48, 4, 3, 0.5
    burnin, mcmc, thin, seed = 2, 6, 2, 31
    Y, _ = oracle.synth.make_data(n, p, k0=4)
    S, SD, info = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, rho, seed=seed, return_sd=True,
                                     return_info=True)
    S2, SD2 = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, rho, seed=seed, return_sd=True)
    plain = dcfm.divideconquer(Y, g, K * g, burnin, mcmc, thin, rho, seed=seed)
    assert S.shape == SD.shape == (p, p) and isinstance(info, dict)
    assert np.array_equal(S, S2) and np.array_equal(SD, SD2) and np.array_equal(S, plain)
    # the same chain at the Sampler level
    nn, pk, P, Kk, keep = D.preprocess_device(Y, g, K * g)
    smp = dcfm.Sampler(nn, P, g, Kk, rho, burnin, mcmc, thin, seed=seed, sigma_m2=True)
    try:
        smp.set_data_raw(Y, D.shard_columns(keep, info["varind"], P, 0, g))
        smp.init_state()
        smp.run(1, burnin + mcmc)
        assert np.array_equal(smp.get_sigma(), S)
        assert np.array_equal(smp.get_sigma_moment("sd"), SD)
    finally:
        smp.close()
    assert np.array_equal(SD, SD.T) and np.all(SD >= 0) and np.any(SD > 0)
    # back in the input's coordinates a standard deviation rescales like the entry (unpermute_sigma)
    sd_cols = np.asarray(Y)[:, D.output_columns(info["keep"], info["varind"])].std(axis=0, ddof=1)
    full = dcfm.unpermute_sigma(SD, info["keep"], info["varind"], Y.shape[1], sd=sd_cols)
    a, b = 3, 17
    ca, cb = D.output_columns(info["keep"], info["varind"])[[a, b]]
    assert full[ca, cb] == SD[a, b] * sd_cols[a] * sd_cols[b]
