"""The MEX gateway's `set_missing` and `imputed` commands (matlab/dcfm_mex.c) through the mock MEX runtime
(tests/mexmock).  CPU: malformed calls -- wrong argument counts, a missing or bad handle, a capacity that is
negative, fractional or of the wrong class -- are rejected with their error ids before the library sees a
pointer.  GPU: `imputed` returns what the Python host twin returns, bit for bit."""
import numpy as np
import pytest

import missing_cases as mc
from helpers import make_case, stacked_draws, state_dict
from mexmock import driver as mm


@pytest.fixture(scope="module")
def mex(tmp_path_factory):
    return mm.Mex(mm.build(tmp_path_factory.mktemp("mexmock_missing")))


def test_malformed_calls_are_rejected(mex):
    mk = np.zeros((4, 2, 1))
    for args in ((), (0.0,), (0.0, mk, 2.0, 1.0)):
        with pytest.raises(mm.MexError) as e:
            mex.call("set_missing", *args)                     # h, mask and at most capacity
        assert e.value.id == "dcfm:nargs", args
    for args in ((), (0.0, 1.0)):
        with pytest.raises(mm.MexError) as e:
            mex.call("imputed", *args)                         # takes exactly h
        assert e.value.id == "dcfm:nargs", args
    for h in (7.0, -1.0, 0.5, 64.0):                           # no such handle
        with pytest.raises(mm.MexError) as e:
            mex.call("set_missing", h, mk)
        assert e.value.id == "dcfm:handle", h
        with pytest.raises(mm.MexError) as e:
            mex.call("imputed", h)
        assert e.value.id == "dcfm:handle", h
    with pytest.raises(mm.MexError) as e:
        mex.call("imputed", np.zeros(2))                       # handle not a scalar
    assert e.value.id == "dcfm:arg"
    for cap in (-1.0, 2.5, np.nan, "3", np.zeros(2)):
        with pytest.raises(mm.MexError) as e:
            mex.call("set_missing", 0.0, mk, cap)              # checked before the handle is looked up
        assert e.value.id == "dcfm:arg", cap
    assert mex.locks() == 0


@pytest.mark.gpu
def test_commands_through_the_gateway_match_the_host_twin(mex, dcfm):
    n, p, g, K = 40, 48, 4, 5
    burnin, mcmc, thin = 1, 4, 2
    N = burnin + mcmc
    c = make_case(n, p, g, K, seed=11)
    P = c["P"]
    st = state_dict(c["st"])
    d = stacked_draws(c["src"], 1, N)
    mask = mc.make_mask("random", n, P, g)
    cfg = dict(n=float(n), P=float(P), g=float(g), K=float(K), rho=c["rho"], burnin=float(burnin),
               mcmc=float(mcmc), thin=float(thin), inject=1.0, seed=float(mc.CHAIN_SEED))
    h = mex.call("create", cfg)
    try:
        with pytest.raises(mm.MexError) as e:
            mex.call("set_missing", h, mask.astype(np.float64))    # the mask before the data
        assert e.value.id == "dcfm:call" and "set_data first" in str(e.value)
        mex.call("set_data", h, c["Yd"])
        mex.call("set_state", h, st["Lambda"], st["ps"], st["omega"], st["psi"], st["Plam"], st["X"], st["Z"],
                 st["delta"], st["tauh"])
        mex.call("set_draws", h, d["NZ"], d["NX"], d["NL"], d["Gpsi"], d["Gdelta"], d["Gps"], 1.0, float(N))
        out = mex.call("imputed", h, nlhs=4)                   # nothing set
        assert out[0].size == 0 and out[2].size == 0 and np.asarray(out[3]).item() == 0.0
        for bad in (np.zeros((n + 1, P, g)), np.zeros(n * P)):
            with pytest.raises(mm.MexError) as e:
                mex.call("set_missing", h, bad)
            assert e.value.id == "dcfm:arg"
        mex.call("set_missing", h, mask.astype(np.float64))    # default capacity mcmc / thin
        mex.call("run", h, 1.0, float(N))
        mean, m2, nvar, cnt = mex.call("imputed", h, nlhs=4)
        assert mex.call("imputed", h).shape == mean.shape      # one output: mean
        mex.call("set_missing", h, np.zeros((0, 0)))           # []: off
        assert mex.call("imputed", h).size == 0
    finally:
        mex.call("destroy", h)
    assert mex.locks() == 0

    smp = dcfm.Sampler(n, P, g, K, c["rho"], burnin, mcmc, thin, inject_draws=True, seed=mc.CHAIN_SEED)
    try:
        smp.set_data(c["Yd"])
        smp.set_state({f: v for f, v in st.items() if f != "eta"})
        smp.set_draws(d, 1, N)
        smp.set_missing(mask)
        smp.run(1, N)
        rmean, rm2, rnvar, rcnt = smp.imputed_raw()
    finally:
        smp.close()
    assert np.asarray(cnt).item() == rcnt == mcmc // thin and np.all(np.isfinite(rmean)) and np.all(rnvar[mask.any(axis=0)] > 0)
    assert mean.shape == (n, P, g) and nvar.shape == (P, g)
    assert np.array_equal(mean, rmean) and np.array_equal(m2, rm2) and np.array_equal(nvar, rnvar)
    assert not np.array_equal(rmean[mask], c["Yd"][mask])
