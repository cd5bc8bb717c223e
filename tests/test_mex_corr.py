"""The MEX gateway's `corr` and `communality` commands (matlab/dcfm_mex.c) through the mock MEX runtime
(tests/mexmock).  CPU: malformed calls — missing or bad handle, a bad `which`, a column range that is negative,
fractional or of the wrong class, a column range on `communality` — are rejected with their error ids before the
library sees a pointer.  GPU: both commands return what the Python host twin returns, bit for bit, for the whole
matrix and for a column range, refuse a range past p, and without cfg.corr pass the library's refusal on."""
import numpy as np
import pytest

from helpers import make_case, stacked_draws, state_dict
from mexmock import driver as mm


@pytest.fixture(scope="module")
def mex(tmp_path_factory):
    return mm.Mex(mm.build(tmp_path_factory.mktemp("mexmock_corr")))


def test_malformed_corr_calls_are_rejected(mex):
    for args in ((), (0.0,), (0.0, "mean", 0.0), (0.0, "mean", 0.0, 1.0, 2.0)):
        with pytest.raises(mm.MexError) as e:
            mex.call("corr", *args)                            # no handle / no which / col0 alone / one too many
        assert e.value.id == "dcfm:nargs", args
    for args in ((), (0.0,), (0.0, "mean", 0.0), (0.0, "mean", 0.0, 1.0)):
        with pytest.raises(mm.MexError) as e:
            mex.call("communality", *args)                     # a vector: handle and which, nothing else
        assert e.value.id == "dcfm:nargs", args
    for cmd in ("corr", "communality"):
        for which in ("var", "", 2.0, "meanmeanmean"):
            with pytest.raises(mm.MexError) as e:
                mex.call(cmd, 0.0, which)                      # not 'mean' | 'm2' | 'sd'
            assert e.value.id == "dcfm:arg", (cmd, which)
        for h in (7.0, -1.0, 0.5, 64.0):                       # no such handle
            with pytest.raises(mm.MexError) as e:
                mex.call(cmd, h, "sd")
            assert e.value.id == "dcfm:handle", (cmd, h)
        with pytest.raises(mm.MexError) as e:
            mex.call(cmd, np.zeros(2), "mean")                 # handle not a scalar
        assert e.value.id == "dcfm:arg", cmd
    for c0, nc in ((-1.0, 4.0), (0.0, -2.0), (0.5, 4.0), (0.0, 1.5), (np.zeros(2), 1.0), ("0", 1.0)):
        with pytest.raises(mm.MexError) as e:
            mex.call("corr", 0.0, "m2", c0, nc)                # bad column range
        assert e.value.id == "dcfm:arg", (c0, nc)
    assert mex.locks() == 0


@pytest.mark.gpu
def test_corr_through_the_gateway_matches_the_host_twin(mex, dcfm):
    n, p, g, K = 40, 48, 4, 5
    burnin, mcmc, thin = 1, 3, 1
    N = burnin + mcmc
    c = make_case(n, p, g, K, seed=11)
    P = c["P"]
    st = state_dict(c["st"])
    d = stacked_draws(c["src"], 1, N)
    cfg = dict(n=float(n), P=float(P), g=float(g), K=float(K), rho=c["rho"], burnin=float(burnin),
               mcmc=float(mcmc), thin=float(thin), inject=1.0)

    def feed(h):
        mex.call("set_data", h, c["Yd"])
        mex.call("set_state", h, st["Lambda"], st["ps"], st["omega"], st["psi"], st["Plam"], st["X"], st["Z"],
                 st["delta"], st["tauh"])
        mex.call("set_draws", h, d["NZ"], d["NX"], d["NL"], d["Gpsi"], d["Gdelta"], d["Gps"], 1.0, float(N))

    got = {}
    h = mex.call("create", dict(cfg, corr=1.0))
    try:
        feed(h)
        assert not mex.call("corr", h, "mean").any()           # no saved sample yet: zeros
        assert not mex.call("communality", h, "m2").any()
        for cmd in ("corr", "communality"):
            with pytest.raises(mm.MexError) as e:
                mex.call(cmd, h, "sd")                         # ... and no standard deviation
            assert e.value.id == "dcfm:call"
        mex.call("run", h, 1.0, float(N))
        for w in ("mean", "m2", "sd"):
            got[w] = mex.call("corr", h, w)
            got[w + "_cols"] = mex.call("corr", h, w, 5.0, 9.0)
            got["h" + w] = mex.call("communality", h, w)
        got["S"] = mex.call("get_sigma", h)
        for c0, nc in ((0.0, float(p + 1)), (float(p), 1.0), (40.0, 9.0)):
            with pytest.raises(mm.MexError) as e:
                mex.call("corr", h, "mean", c0, nc)            # past p: never reaches the library
            assert e.value.id == "dcfm:arg"
    finally:
        mex.call("destroy", h)
    h = mex.call("create", cfg)                                # without cfg.corr
    try:
        for cmd in ("corr", "communality"):
            with pytest.raises(mm.MexError) as e:
                mex.call(cmd, h, "mean")
            assert e.value.id == "dcfm:call" and "DCFM_FLAG_CORR" in e.value.msg
    finally:
        mex.call("destroy", h)
    assert mex.locks() == 0

    smp = dcfm.Sampler(n, P, g, K, c["rho"], burnin, mcmc, thin, inject_draws=True, corr=True)
    try:
        smp.set_data(c["Yd"])
        smp.set_state({f: v for f, v in st.items() if f != "eta"})
        smp.set_draws(d, 1, N)
        smp.run(1, N)
        ref = {w: smp.get_corr(w) for w in ("mean", "m2", "sd")}
        href = {w: smp.get_communality(w) for w in ("mean", "m2", "sd")}
        S = smp.get_sigma()
    finally:
        smp.close()
    assert np.array_equal(got["S"], S)
    for w in ("mean", "m2", "sd"):
        assert got[w].shape == (p, p) and np.array_equal(got[w], ref[w]), w
        assert np.array_equal(got[w + "_cols"], ref[w][:, 5:14]), w
        assert got["h" + w].size == p and np.array_equal(np.ravel(got["h" + w]), href[w]), w
    assert np.array_equal(ref["mean"].diagonal(), np.ones(p)) and not ref["sd"].diagonal().any()
    assert np.all(href["mean"] > 0) and np.all(href["mean"] < 1)
