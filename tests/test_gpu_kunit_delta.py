"""Device primitives on their own (tests/kunit/kunit.hip), part 5: suffix_sum_nv + delta_chain<1> and <2> of
csrc/delta.h (the delta / tau chain as an affine wave scan), staged as delta_shard stages them.

delta_new is compared with the K-step recurrence of the header in mpmath (60 digits): per (NV, K, P),
max over seeds of the relative error <= 8 x that of the serial float64 recurrence, floor 8 K 2^-53.
Idle indices (idx >= K) return exactly 1.  test_kunit_ref.py checks on the CPU that the serial recurrence is
finite on every input here, the K = 128 case whose running product of alpha underflows included."""
import numpy as np
import pytest

import kunit_ref as R

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 100, 127, 128)
PS = (20, 1250)
SEEDS = (0, 1)
BD1, BD2 = 1.0, 2.5             # distinct: b_0 = bd1 belongs to index 0 of the first slice only


def _cases(nv):
    out = [(K, P, s, False) for K in KS if K <= 64 * nv for P in PS for s in SEEDS]
    if nv == 2:
        out += [(128, 1250, s, True) for s in SEEDS]
    return out


@pytest.mark.parametrize("nv", [1, 2])
def test_delta_chain(nv):
    cases = _cases(nv)
    W = 64 * nv
    arrs = [np.full((len(cases), W), np.nan) for _ in range(4)]           # idle slots are never read
    inputs = []
    for c, (K, P, s, uf) in enumerate(cases):
        inp = R.delta_inputs(K, P, s, underflow=uf)
        inputs.append(inp)
        for a, v in zip(arrs, inp):
            a[c, :K] = v
    Ks = np.array([c[0] for c in cases], dtype=np.int32)
    dnew = np.zeros((len(cases), W))
    assert R.lib().kunit_delta(nv, *(R.ptr(a) for a in arrs), R.ptr(Ks), len(cases), R.c_double(BD1), R.c_double(BD2),
                               R.ptr(dnew)) == 0
    e_dev, e_ser = {}, {}
    for c, ((K, P, s, uf), inp) in enumerate(zip(cases, inputs)):
        assert np.all(dnew[c, K:] == 1.0), "an idle index did not return exactly 1"
        assert np.isfinite(dnew[c, :K]).all() and np.all(dnew[c, :K] > 0)
        ref = R.delta_serial(*inp, BD1, BD2, mp=True)
        key = (K, P, uf)
        e_dev[key] = max(e_dev.get(key, 0.0), R.rel_err_mp(dnew[c, :K], ref))
        e_ser[key] = max(e_ser.get(key, 0.0), R.rel_err_mp(R.delta_serial(*inp, BD1, BD2), ref))
    worst = max(e_dev[k] / max(e_ser[k], k[0] * R.EPS53) for k in e_dev)
    print(f"delta_chain<{nv}>: worst dev / max(serial, K 2^-53) = {worst:.3g}; "
          + "  ".join(f"K={k[0]},P={k[1]}{'u' if k[2] else ''}: {e_dev[k] / R.EPS53:.1f}u vs {e_ser[k] / R.EPS53:.1f}u"
                      for k in e_dev))
    fails = [(k, e_dev[k], e_ser[k]) for k in e_dev if not e_dev[k] <= R.bar(e_ser[k], k[0])]
    assert not fails, f"(K, P, underflow), dev, serial over the bar: {fails}"
