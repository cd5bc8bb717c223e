"""The K <= 32 chain's trimmed launches at the shapes where they can go wrong:
  * k_xdraw deals the generated X normals (dc:126) over waves 0..3, behind their message loads;
  * k_lambda writes a saved iteration's sample into the assembly batch itself (no k_save launch);
  * the W pass reduces over ceil(P / 8) chunks of columns, not PP / 8.
None of them may change a bit of any output; what is checked here is each against an independent
reference (the CPU oracle, the other launch layout, a Sigma formed on the host from the states the
device held), at the suite's 1e-10 bar, on shapes chosen for the edges: a partial last row block,
odd K, every source-sum chunking of k_xdraw, both Lb buffers with full batches, a whole padding
chunk / a partial last chunk / no padding at all in the W pass.
"""
import numpy as np
import pytest

import test_gpu_loopback as TL
from helpers import STATE_CMP, make_case, rel_err, stacked_draws, state_dict
from oracle import dc_oracle as F
from oracle import philox_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-10   # the project's parity bar (tests/test_gpu_parity.py)
UNFUSED, EXACT_RESIDUAL, GUARD_ALL = 0x2, 0x10, 0x40


def _init_state(c):
    return {f: v for f, v in state_dict(c["st"]).items() if f != "eta"}


# ---- X draw: n = 37 (10 row blocks of 4, the last with one row), odd K and a pair tail; g = 3: three
# single-slice chunks (the plain-load path); g = 16: 4 chunks of 4 slices, one slice per lane part;
# g = 64: c3's chunking, 4 chunks of 16, four slices per part; g = 10: one chunk of 10 summed whole,
# two load batches (the draw sits behind the first)
@pytest.mark.parametrize("K,g", [(30, 3), (7, 3), (30, 16), (7, 16), (7, 64), (7, 10)])
def test_xdraw_generated_normals(dcfm, K, g):
    n, P, seed, N = 37, 8, 77, 3
    c = make_case(n, P * g, g, K)
    assert (c["n"], c["P"]) == (n, P)
    got = {}
    for flags in (0, UNFUSED):
        smp = dcfm.Sampler(n, P, g, K, c["rho"], 0, N, 1, seed=seed, inject_draws=False, flags=flags)
        try:
            smp.set_data(c["Yd"])
            smp.set_state(_init_state(c))
            smp.run(1, N)
            got[flags] = smp.get_state()
        finally:
            smp.close()
    # tests/test_gpu_alt_paths.py holds the two layouts to 1e-10 of the oracle, not to each other's bits
    for f in ("X", "Z", "Lambda"):
        e = rel_err(got[0][f], got[UNFUSED][f])
        print(f"K={K} g={g} {f}: fused vs unfused {e:.3e}")
        assert e < TOL, f"{f}: fused vs unfused rel err {e:.3e}"
    src = R.PhiloxSource(seed, n, c["p"], g, K, c["hyper"])
    ref = c["st"].copy()
    F.run_chain(c["Yd"], ref, c["rho"], c["hyper"], src.iteration, 1, N, 0, N, 1)
    for f in STATE_CMP:
        e = rel_err(got[0][f], getattr(ref, f))
        print(f"K={K} g={g} {f}: vs oracle {e:.3e}")
        assert e < TOL, f"{f} rel err {e:.3e}"


# ---- sample save: 9 saved samples (iterations 4, 6, .., 20) in three full batches of 3, so both Lb
# buffers are written, the first one twice, and no partial flush ends the run
def _host_sigma(samples, rho, effsamp, square=False):
    """(1 / effsamp) sum_s Sigma(s) [squared entrywise]: Sigma(s) = Lambda Lambda' with coefficient 1 inside
    a shard's block and rho across blocks, omega on the diagonal (dc:182-192)."""
    out = 0.0
    for Lam, om in samples:                                   # P x K x g, P x g
        P, K, g = Lam.shape
        L = np.moveaxis(Lam, 2, 0).reshape(g * P, K)          # row a = m P + j
        shard = np.repeat(np.arange(g), P)
        S = (L @ L.T) * np.where(shard[:, None] == shard[None, :], 1.0, rho)
        S[np.diag_indices(g * P)] += np.moveaxis(om, 1, 0).reshape(-1)
        out = out + (S * S if square else S)
    return out / effsamp


@pytest.mark.parametrize("K,flags,m2", [(7, 0, False), (30, 0, False), (7, 0, True), (30, 0, True),
                                        (7, EXACT_RESIDUAL, False), (30, EXACT_RESIDUAL, False),
                                        (30, GUARD_ALL, False),       # omega saved from the residual fallback's store
                                        (40, 0, False)],
                         ids=["K7", "K30", "K7_m2", "K30_m2", "K7_exact", "K30_exact", "K30_guard_all", "K40_wide"])
def test_sample_save(dcfm, K, flags, m2):
    n, P, g, seed = 37, 20, 3, 31
    burnin, thin, asm_batch, N = 3, 2, 3, 20
    mcmc = N - burnin
    p = P * g
    c = make_case(n, p, g, K, seed=5)
    assert (c["n"], c["P"]) == (n, P)

    def sampler():
        smp = dcfm.Sampler(n, P, g, K, c["rho"], burnin, mcmc, thin, seed=seed, asm_batch=asm_batch, flags=flags,
                           sigma_m2=m2)
        smp.set_data(c["Yd"])
        smp.set_state(_init_state(c))
        return smp

    def read(smp):
        assert smp.saved_samples() == 9
        return smp.get_sigma_cols(0, p), (smp.get_sigma_moment_cols("m2", 0, p) if m2 else None)

    a = sampler()
    try:
        a.run(1, N)
        SA, MA = read(a)
    finally:
        a.close()
    b, samples = sampler(), []
    try:
        for it in range(1, N + 1):
            b.run(it, 1)
            if it % thin == 0 and it > burnin:
                s = b.get_state(("Lambda", "omega"))
                samples.append((np.array(s["Lambda"], dtype=np.float64), np.array(s["omega"], dtype=np.float64)))
        SB, MB = read(b)
    finally:
        b.close()
    assert len(samples) == 9
    S_ref = _host_sigma(samples, c["rho"], mcmc / thin)
    for name, S in (("A (one run)", SA), ("B (stepped)", SB)):
        e = rel_err(S, S_ref)
        print(f"K={K} flags={flags:#x} chain {name}: Sigma rel err {e:.3e}")
        assert e < TOL, f"chain {name}: Sigma rel err {e:.3e}"
    if m2:
        M_ref = _host_sigma(samples, c["rho"], mcmc / thin, square=True)
        for name, M in (("A (one run)", MA), ("B (stepped)", MB)):
            e = rel_err(M, M_ref)
            print(f"K={K} chain {name}: second moment rel err {e:.3e}")
            assert e < TOL, f"chain {name}: second moment rel err {e:.3e}"


# ---- W-pass bound: P = 24 (PP = 32, the last chunk all padding: skipped), P = 20 (the last chunk half
# data, kept), P = 8 (one chunk); K = 40: the wide pass through the same reduction
@pytest.mark.parametrize("P,K", [(24, 30), (20, 30), (8, 30), (24, 40)])
def test_wpass_bound_against_oracle(dcfm, P, K):
    n, g, N = 37, 2, 2
    c = make_case(n, P * g, g, K)
    assert (c["n"], c["P"]) == (n, P)
    smp = dcfm.Sampler(n, P, g, K, c["rho"], 0, N, 1, inject_draws=True)
    try:
        smp.set_data(c["Yd"])
        smp.set_state(_init_state(c))
        smp.set_draws(stacked_draws(c["src"], 1, N), 1, N)
        ref, Sref = c["st"].copy(), None
        for it in range(1, N + 1):
            smp.run(it, 1)
            Sref = F.run_chain(c["Yd"], ref, c["rho"], c["hyper"], c["src"].iteration, it, 1, 0, N, 1, Sigmaout=Sref)
            got = smp.get_state()
            for f in STATE_CMP:
                e = rel_err(got[f], getattr(ref, f))
                print(f"P={P} K={K} it={it} {f}: {e:.3e}")
                assert e < TOL, f"iteration {it} {f} rel err {e:.3e}"
        e = rel_err(smp.get_sigma(), Sref)
        assert e < TOL, f"Sigmaout rel err {e:.3e}"
    finally:
        smp.close()


def test_wpass_bound_two_ranks_loopback(dcfm):
    """One shard per rank at P = 24: the 64-row W tiles of the few-shards launch skip the same chunk, and
    rank 0's gathered Sigmaout is bitwise the one-rank run's."""
    n, P, g, K, nr = 37, 24, 2, 30, 2
    burnin, mcmc, thin = 1, 4, 2
    c = make_case(n, P * g, g, K, seed=13)
    assert (c["n"], c["P"]) == (n, P)
    out, N = TL._run_ranks(dcfm, c, g, K, burnin, mcmc, thin, nr)
    one = TL._one_rank_sigma(dcfm, c, g, K, burnin, mcmc, thin)
    assert out[1]["Sig"] is None
    assert np.array_equal(out[0]["Sig"], one)
    ref = c["st"].copy()
    S_ref = F.run_chain(c["Yd"], ref, c["rho"], c["hyper"], c["src"].iteration, 1, N, burnin, mcmc, thin)
    assert rel_err(one, S_ref) < TOL
