"""The MEX gateway's `set_predict` and `predict` commands (matlab/dcfm_mex.c) through the mock MEX runtime
(tests/mexmock).  CPU: malformed calls -- wrong argument counts, a missing or bad handle, a capacity that is
negative, fractional or of the wrong class -- are rejected with their error ids before the library sees a
pointer.  GPU: `predict` returns what the Python host twin returns, in MATLAB's order, bit for bit."""
import numpy as np
import pytest

import predict_cases as dc
from helpers import make_case, stacked_draws, state_dict
from mexmock import driver as mm


@pytest.fixture(scope="module")
def mex(tmp_path_factory):
    return mm.Mex(mm.build(tmp_path_factory.mktemp("mexmock_predict")))


def test_malformed_calls_are_rejected(mex):
    Y, ob = np.zeros((4, 1)), np.ones(4)
    for args in ((), (0.0,), (0.0, Y), (0.0, Y, ob, 2.0, 1.0)):
        with pytest.raises(mm.MexError) as e:
            mex.call("set_predict", *args)                     # h, Ynew, observed and at most capacity
        assert e.value.id == "dcfm:nargs", args
    for args in ((), (0.0, 1.0)):
        with pytest.raises(mm.MexError) as e:
            mex.call("predict", *args)                         # takes exactly h
        assert e.value.id == "dcfm:nargs", args
    for h in (7.0, -1.0, 0.5, 64.0):                           # no such handle
        with pytest.raises(mm.MexError) as e:
            mex.call("set_predict", h, Y, ob)
        assert e.value.id == "dcfm:handle", h
        with pytest.raises(mm.MexError) as e:
            mex.call("predict", h)
        assert e.value.id == "dcfm:handle", h
    with pytest.raises(mm.MexError) as e:
        mex.call("predict", np.zeros(2))                       # handle not a scalar
    assert e.value.id == "dcfm:arg"
    for cap in (-1.0, 2.5, np.nan, "3", np.zeros(2)):
        with pytest.raises(mm.MexError) as e:
            mex.call("set_predict", 0.0, Y, ob, cap)           # checked before the handle is looked up
        assert e.value.id == "dcfm:arg", cap
    assert mex.locks() == 0


@pytest.mark.gpu
def test_commands_through_the_gateway_match_the_host_twin(mex, dcfm):
    n, p, g, K, nt = 40, 48, 4, 5, 3
    burnin, mcmc, thin = 1, 4, 2
    N = burnin + mcmc
    c = make_case(n, p, g, K, seed=11)
    P = c["P"]
    st = state_dict(c["st"])
    d = stacked_draws(c["src"], 1, N)
    Y, ob = dc.new_rows(p, nt), dc.mask("random", P, g)
    cfg = dict(n=float(n), P=float(P), g=float(g), K=float(K), rho=c["rho"], burnin=float(burnin),
               mcmc=float(mcmc), thin=float(thin), inject=1.0)
    h = mex.call("create", cfg)
    try:
        mex.call("set_data", h, c["Yd"])
        mex.call("set_state", h, st["Lambda"], st["ps"], st["omega"], st["psi"], st["Plam"], st["X"], st["Z"],
                 st["delta"], st["tauh"])
        mex.call("set_draws", h, d["NZ"], d["NX"], d["NL"], d["Gpsi"], d["Gdelta"], d["Gps"], 1.0, float(N))
        out = mex.call("predict", h, nlhs=5)                   # nothing set
        assert out[0].shape == (p, 0) and out[3].shape == (0, 0) and out[4].size == 0 and out[2].size == 0
        for bad in (np.zeros((p + 1, nt)), np.zeros((p, 33))):
            with pytest.raises(mm.MexError) as e:
                mex.call("set_predict", h, bad, ob.astype(np.float64))
            assert e.value.id == "dcfm:arg"
        with pytest.raises(mm.MexError) as e:
            mex.call("set_predict", h, Y, np.ones(p - 1))
        assert e.value.id == "dcfm:arg"
        mex.call("set_predict", h, Y, ob.astype(np.float64))   # default capacity mcmc / thin
        mex.call("run", h, 1.0, float(N))
        mean, m2, cvar, maha, ld = mex.call("predict", h, nlhs=5)
        assert mex.call("predict", h).shape == mean.shape      # one output: mean
        mex.call("set_predict", h, Y, ob.astype(np.float64), 1.0)   # capacity 1: the count resets
        assert mex.call("predict", h, nlhs=5)[4].size == 0
        mex.call("run", h, 2.0, 1.0)                           # one more saved iteration
        one = mex.call("predict", h, nlhs=5)
        assert one[3].shape == (nt, 1) and one[4].size == 1 and np.isfinite(one[4]).all()
        mex.call("set_predict", h, Y, ob.astype(np.float64), 0.0)   # off
        assert mex.call("predict", h).shape == (p, 0)
    finally:
        mex.call("destroy", h)
    assert mex.locks() == 0

    smp = dcfm.Sampler(n, P, g, K, c["rho"], burnin, mcmc, thin, inject_draws=True)
    try:
        smp.set_data(c["Yd"])
        smp.set_state({f: v for f, v in st.items() if f != "eta"})
        smp.set_draws(d, 1, N)
        smp.set_predict(Y, ob)
        smp.run(1, N)
        rmean, rm2, rcvar, rmaha, rld, cnt = smp.predict_raw()
    finally:
        smp.close()
    assert cnt == mcmc // thin and np.all(np.isfinite(rmean)) and np.all(rcvar > 0)
    assert np.array_equal(mean, rmean) and np.array_equal(m2, rm2) and np.array_equal(np.asarray(cvar).reshape(-1), rcvar)
    assert maha.shape == (nt, cnt) and np.array_equal(maha, rmaha.T)
    assert np.array_equal(np.asarray(ld).reshape(-1), rld)
