"""The MEX gateway's `set_loglik` and `loglik` commands (matlab/dcfm_mex.c) through the mock MEX runtime
(tests/mexmock).  CPU: malformed calls -- wrong argument counts, a missing or bad handle, a capacity that is
negative, fractional or of the wrong class -- are rejected with their error ids before the library sees a
pointer.  GPU: `loglik` returns what the Python host twin returns, transposed into MATLAB's order, bit for
bit."""
import numpy as np
import pytest

from helpers import make_case, stacked_draws, state_dict
from mexmock import driver as mm


@pytest.fixture(scope="module")
def mex(tmp_path_factory):
    return mm.Mex(mm.build(tmp_path_factory.mktemp("mexmock_loglik")))


def test_malformed_calls_are_rejected(mex):
    for args in ((), (0.0, 2.0, 1.0)):
        with pytest.raises(mm.MexError) as e:
            mex.call("set_loglik", *args)                      # h and at most capacity
        assert e.value.id == "dcfm:nargs", args
    for args in ((), (0.0, 1.0)):
        with pytest.raises(mm.MexError) as e:
            mex.call("loglik", *args)                          # takes exactly h
        assert e.value.id == "dcfm:nargs", args
    for h in (7.0, -1.0, 0.5, 64.0):                           # no such handle
        with pytest.raises(mm.MexError) as e:
            mex.call("set_loglik", h)
        assert e.value.id == "dcfm:handle", h
        with pytest.raises(mm.MexError) as e:
            mex.call("loglik", h)
        assert e.value.id == "dcfm:handle", h
    with pytest.raises(mm.MexError) as e:
        mex.call("loglik", np.zeros(2))                        # handle not a scalar
    assert e.value.id == "dcfm:arg"
    for cap in (-1.0, 2.5, np.nan, "3", np.zeros(2)):
        with pytest.raises(mm.MexError) as e:
            mex.call("set_loglik", 0.0, cap)                   # checked before the handle is looked up
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
    cfg = dict(n=float(n), P=float(P), g=float(g), K=float(K), rho=c["rho"], burnin=float(burnin),
               mcmc=float(mcmc), thin=float(thin), inject=1.0)
    h = mex.call("create", cfg)
    try:
        mex.call("set_data", h, c["Yd"])
        mex.call("set_state", h, st["Lambda"], st["ps"], st["omega"], st["psi"], st["Plam"], st["X"], st["Z"],
                 st["delta"], st["tauh"])
        mex.call("set_draws", h, d["NZ"], d["NX"], d["NL"], d["Gpsi"], d["Gdelta"], d["Gps"], 1.0, float(N))
        q, ld = mex.call("loglik", h, nlhs=2)                  # nothing set
        assert q.shape == (n, 0) and ld.size == 0
        mex.call("set_loglik", h)                              # default capacity mcmc / thin
        mex.call("run", h, 1.0, float(N))
        q, ld = mex.call("loglik", h, nlhs=2)
        assert mex.call("loglik", h).shape == q.shape          # one output: maha
        mex.call("set_loglik", h, 1.0)                         # capacity 1: the count resets
        assert mex.call("loglik", h).shape == (n, 0)
        mex.call("run", h, 2.0, 1.0)                           # one more saved iteration
        q0, ld0 = mex.call("loglik", h, nlhs=2)
        assert q0.shape == (n, 1) and ld0.size == 1 and np.isfinite(ld0).all() and np.all(q0 > 0)
        mex.call("set_loglik", h, 0.0)                         # off
        assert mex.call("loglik", h).shape == (n, 0)
    finally:
        mex.call("destroy", h)
    assert mex.locks() == 0

    smp = dcfm.Sampler(n, P, g, K, c["rho"], burnin, mcmc, thin, inject_draws=True)
    try:
        smp.set_data(c["Yd"])
        smp.set_state({f: v for f, v in st.items() if f != "eta"})
        smp.set_draws(d, 1, N)
        smp.set_loglik()
        smp.run(1, N)
        _, ref, rld = smp.loglik_draws(parts=True)
    finally:
        smp.close()
    assert ref.shape == (mcmc // thin, n) and np.all(np.isfinite(ref)) and np.all(ref > 0)
    assert q.shape == (n, mcmc // thin) and np.array_equal(q, ref.T)
    assert np.array_equal(np.asarray(ld).reshape(-1), rld)
