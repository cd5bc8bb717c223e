"""The MEX gateway's `sigma_apply` and `sigma_eigs` commands (matlab/dcfm_mex.c) through the mock MEX
runtime (tests/mexmock).  CPU: malformed calls -- wrong argument counts, a missing or bad handle, an
r / tol / max_passes / seed that is out of range, fractional or of the wrong class -- are rejected with
their error ids before the library sees a pointer.  GPU: a V of the wrong shape is refused against the
handle's own p, and both commands return what the Python host twin returns, bit for bit (the pointers
and sizes go through unchanged)."""
import numpy as np
import pytest

from helpers import make_case, stacked_draws, state_dict
from mexmock import driver as mm


@pytest.fixture(scope="module")
def mex(tmp_path_factory):
    return mm.Mex(mm.build(tmp_path_factory.mktemp("mexmock_apply")))


def test_malformed_calls_are_rejected(mex):
    for args in ((), (0.0,), (0.0, np.zeros((4, 1)), 1.0)):
        with pytest.raises(mm.MexError) as e:
            mex.call("sigma_apply", *args)                     # takes exactly h, V
        assert e.value.id == "dcfm:nargs", args
    for h in (7.0, -1.0, 0.5, 64.0):                           # no such handle
        with pytest.raises(mm.MexError) as e:
            mex.call("sigma_apply", h, np.zeros((4, 1)))
        assert e.value.id == "dcfm:handle", h
        with pytest.raises(mm.MexError) as e:
            mex.call("sigma_eigs", h, 2.0)
        assert e.value.id == "dcfm:handle", h
    with pytest.raises(mm.MexError) as e:
        mex.call("sigma_apply", np.zeros(2), np.zeros((4, 1)))  # handle not a scalar
    assert e.value.id == "dcfm:arg"
    for args in ((), (0.0,), (0.0, 2.0, 1e-8, 4.0, 1.0, 0.0)):
        with pytest.raises(mm.MexError) as e:
            mex.call("sigma_eigs", *args, nlhs=3)              # h, r and at most tol, max_passes, seed
        assert e.value.id == "dcfm:nargs", args
    bad = [(0.0,), (33.0,), (2.5,), (-1.0,), ("2",), (np.zeros(2),),                 # r
           (2.0, 0.0), (2.0, -1e-8), (2.0, np.nan), (2.0, "tol"),                    # tol
           (2.0, 1e-8, 0.0), (2.0, 1e-8, 2.5), (2.0, 1e-8, -3.0),                    # max_passes
           (2.0, 1e-8, 4.0, -1.0), (2.0, 1e-8, 4.0, 0.5), (2.0, 1e-8, 4.0, 2.0 ** 60)]   # seed
    for args in bad:
        with pytest.raises(mm.MexError) as e:
            mex.call("sigma_eigs", 0.0, *args, nlhs=3)         # checked before the handle is looked up
        assert e.value.id == "dcfm:arg", args
    assert mex.locks() == 0


@pytest.mark.gpu
def test_commands_through_the_gateway_match_the_host_twin(mex, dcfm):
    n, p, g, K = 40, 48, 4, 5
    burnin, mcmc, thin = 1, 3, 1
    N = burnin + mcmc
    c = make_case(n, p, g, K, seed=11)
    P = c["P"]
    st = state_dict(c["st"])
    d = stacked_draws(c["src"], 1, N)
    cfg = dict(n=float(n), P=float(P), g=float(g), K=float(K), rho=c["rho"], burnin=float(burnin),
               mcmc=float(mcmc), thin=float(thin), inject=1.0)
    rng = np.random.default_rng(8)
    V = rng.standard_normal((p, 35))
    h = mex.call("create", cfg)
    try:
        mex.call("set_data", h, c["Yd"])
        mex.call("set_state", h, st["Lambda"], st["ps"], st["omega"], st["psi"], st["Plam"], st["X"], st["Z"],
                 st["delta"], st["tauh"])
        mex.call("set_draws", h, d["NZ"], d["NX"], d["NL"], d["Gpsi"], d["Gdelta"], d["Gps"], 1.0, float(N))
        with pytest.raises(mm.MexError) as e:
            mex.call("sigma_eigs", h, 3.0, nlhs=3)             # no saved sample yet: the library refuses
        assert e.value.id == "dcfm:call" and "saved sample" in e.value.msg
        mex.call("run", h, 1.0, float(N))
        for badV in (np.zeros((p + 1, 2)), np.zeros((p - 1, 1)), np.zeros((p, 0)), V.astype(np.int64), "V"):
            with pytest.raises(mm.MexError) as e:
                mex.call("sigma_apply", h, badV)               # never reaches the library
            assert e.value.id == "dcfm:arg"
        with pytest.raises(mm.MexError) as e:
            mex.call("sigma_apply", h, mex.arr(V, cplx=True), raw=(1,))
        assert e.value.id == "dcfm:arg"
        Y = mex.call("sigma_apply", h, V)
        y1 = mex.call("sigma_apply", h, V[:, 3])               # a column vector
        d3 = mex.call("sigma_eigs", h, 4.0, nlhs=3)
        d1 = mex.call("sigma_eigs", h, 4.0, 1e-6, 5.0, 9.0)    # one output: the values
    finally:
        mex.call("destroy", h)
    assert mex.locks() == 0

    smp = dcfm.Sampler(n, P, g, K, c["rho"], burnin, mcmc, thin, inject_draws=True)
    try:
        smp.set_data(c["Yd"])
        smp.set_state({f: v for f, v in st.items() if f != "eta"})
        smp.set_draws(d, 1, N)
        smp.run(1, N)
        refY = smp.sigma_apply(V)
        ref3 = smp.sigma_eigs(4)
        ref1 = smp.sigma_eigs(4, tol=1e-6, max_passes=5, seed=9)
    finally:
        smp.close()
    assert Y.shape == (p, 35) and np.array_equal(Y, refY)
    assert y1.shape == (p, 1) and np.array_equal(y1[:, 0], refY[:, 3])
    vals, vecs, res = d3
    assert vals.shape == (4, 1) and vecs.shape == (p, 4) and res.shape == (4, 1)
    assert np.array_equal(vals[:, 0], ref3["values"]) and np.array_equal(vecs, ref3["vectors"])
    assert np.array_equal(res[:, 0], ref3["resid"])
    assert d1.shape == (4, 1) and np.array_equal(d1[:, 0], ref1["values"])
