"""k_assemble at every shape of its chunk loop: the k extent of a flush (batch x K, rounded up to the
MFMA k-step of 4) decides how many whole 16-column chunks the tile loop runs and how many k-steps
(1 .. 4) its last chunk has.

A chain with injected draws, burnin 0 and thin 1 saves every iteration; dcfm_run flushes the open batch
before it returns, so a run of b iterations (b <= asm_batch) is one flush of b samples, kext =
round_up(b K, 4).  The plans below list the runs; PLAN_KEXT pins the extents they reach:

    kext    4   12   16   20   24   60  124 |  32   60  120
    whole   0    0    0    1    1    3    7 |   1    3    7     chunks in the loop
    last    1    3    4    1    2    3    3 |   4    3    2     k-steps of the last chunk

p = 150 = 3 x 50: tile rows 0 and 1 (22 live rows), tiles (0, 0) and (1, 1) diagonal with same-shard and
cross-shard pairs, tile (1, 0) with both kinds as well (rows 128 .. 149 are shard 2, columns 100 .. 127
too).  p = 256 = 2 x 128: no partial tile, tile (1, 0) purely cross-shard (accumulators start from the old
Sigma), the diagonal tiles purely same-shard.

Reference: the NumPy oracle's chain (oracle.dc_oracle.run_chain) on the same draws, its Sigmaout; bar:
the suite's 1e-10 normwise (helpers.rel_err, as tests/test_gpu_sigma_moments.py and the parity tests).
The same chain flushed sample by sample (asm_batch = 1) must agree with the batched one to the same bar,
and a sampler with DCFM_FLAG_SIGMA_M2 (k_assemble_m2 reads the same batch) must pass that kernel's own
check (test_gpu_sigma_moments._check) on these plans.
"""
import numpy as np
import pytest

from helpers import make_case, rel_err, stacked_draws, state_dict
from oracle import dc_oracle as F
from test_gpu_sigma_moments import _Ref, _check

pytestmark = pytest.mark.gpu

TOL = 1e-10

# name: (n, g, P, K, asm_batch, run lengths)
PLANS = {
    "p150_K3": (40, 3, 50, 3, 41, (1, 4, 5, 6, 8, 20, 41)),
    "p150_K30": (40, 3, 50, 30, 4, (1, 2, 4)),
    "p256_K3": (40, 2, 128, 3, 8, (1, 5, 6, 8)),
}
PLAN_KEXT = {
    "p150_K3": [4, 12, 16, 20, 24, 60, 124],
    "p150_K30": [32, 60, 120],
    "p256_K3": [4, 16, 20, 24],
}


def _kexts(K, runs):
    return [-(-(b * K) // 4) * 4 for b in runs]


_cache = {}


def _case(name):
    """The case, the oracle's Sigmaout and its saved states (computed once, never modified)."""
    if name not in _cache:
        n, g, P, K, _, runs = PLANS[name]
        N = sum(runs)
        c = make_case(n, g * P, g, K, seed=17)
        assert (c["p"], c["P"]) == (g * P, P)
        st, rec = c["st"].copy(), []
        S = F.run_chain(c["Yd"], st, c["rho"], c["hyper"], c["src"].iteration, 1, N, 0, N, 1, record=rec)
        assert len(rec) == N
        S.setflags(write=False)
        _cache[name] = (c, S, rec)
    return _cache[name]


def _run(dcfm, name, asm_batch, runs, **kw):
    n, g, P, K, _, plan = PLANS[name]
    N = sum(plan)
    assert sum(runs) == N
    c, _, _ = _case(name)
    smp = dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], 0, N, 1, inject_draws=True, asm_batch=asm_batch, **kw)
    try:
        smp.set_data(c["Yd"])
        smp.set_state({f: v for f, v in state_dict(c["st"]).items() if f != "eta"})
        smp.set_draws(stacked_draws(c["src"], 1, N), 1, N)
        it = 1
        for b in runs:
            smp.run(it, b)
            it += b
        assert smp.saved_samples() == N
        out = {"cols": smp.get_sigma_cols(0, c["p"])}
        if kw.get("sigma_m2"):
            out["m2"], out["sd"] = smp.get_sigma_moment("m2"), smp.get_sigma_moment("sd")
    finally:
        smp.close()
    return out


_batched = {}


def _batched_sigma(dcfm, name):
    if name not in _batched:
        _, _, _, _, B, runs = PLANS[name]
        _batched[name] = _run(dcfm, name, B, runs)["cols"]
    return _batched[name]


@pytest.mark.parametrize("name", list(PLANS))
def test_plan_reaches_the_extents(name):
    _, _, _, K, B, runs = PLANS[name]
    assert max(runs) <= B
    assert _kexts(K, runs) == PLAN_KEXT[name]


def test_every_last_chunk_length_is_reached():
    ks = sorted({k for v in PLAN_KEXT.values() for k in v})
    assert {4, 12, 16, 20, 60, 124} <= set(ks)
    last = {(k - 1) % 16 // 4 + 1 for k in ks}
    assert last == {1, 2, 3, 4}
    assert {k for k in ks if k > 16} and {k for k in ks if k <= 16}     # with and without whole chunks in the loop


@pytest.mark.parametrize("name", list(PLANS))
def test_batched_flushes_against_oracle(dcfm, name):
    c, S_ref, _ = _case(name)
    S = _batched_sigma(dcfm, name)
    e = rel_err(S, S_ref)
    print(f"{name}: kext {PLAN_KEXT[name]}, Sigmaout rel err {e:.3e} (bar {TOL:.0e})")
    assert S.shape == (c["p"], c["p"])
    assert e < TOL
    assert np.array_equal(S, S.T)


@pytest.mark.parametrize("name", list(PLANS))
def test_single_sample_flushes_agree(dcfm, name):
    """The same chain flushed as 1 + 1 + ... (asm_batch = 1, one run) and in the plan's batches."""
    c, S_ref, _ = _case(name)
    N = sum(PLANS[name][5])
    one = _run(dcfm, name, 1, (N,))["cols"]
    e_ref, e_pair = rel_err(one, S_ref), rel_err(one, _batched_sigma(dcfm, name))
    print(f"{name}: single-sample flushes vs oracle {e_ref:.3e}, vs batched {e_pair:.3e} (bar {TOL:.0e})")
    assert e_ref < TOL
    assert e_pair < TOL


@pytest.mark.parametrize("name", list(PLANS))
def test_second_moment_on_the_same_batches(dcfm, name):
    """DCFM_FLAG_SIGMA_M2: k_assemble_m2 behind k_assemble on the same batch, its own check unchanged."""
    c, S_ref, rec = _case(name)
    _, _, _, _, B, runs = PLANS[name]
    N = sum(runs)
    out = _run(dcfm, name, B, runs, sigma_m2=True)
    ref = _Ref(N / 1)
    for st in rec:
        ref.add(st.Lambda, st.omega, c["rho"])
    assert rel_err(out["cols"], S_ref) < TOL
    assert np.array_equal(out["cols"], _batched_sigma(dcfm, name))     # the flag changes nothing that exists
    _check(out["m2"], out["sd"], ref, name)
