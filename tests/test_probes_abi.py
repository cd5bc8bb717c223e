"""CPU tests of the probe draws' boundary (dcfm_set_probes / dcfm_get_probe_draws): the binding lists and
resolves both symbols with their four and three arguments, a null handle is refused with nothing
written, the ABI version and the kernel-id count stay (the change is additive), the Sampler methods
exist, and diagnostics.summarize_probes gives the correlations and quantiles worked out by hand -- all
without a GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "dcfm.h"


def _define(name):
    m = re.search(rf"^#define\s+{name}\s+(0x[0-9a-fA-F]+|\d+)u?\b", HEADER.read_text(), re.M)
    assert m, f"{name} not defined in include/dcfm.h"
    return int(m.group(1), 0)


def test_library_resolves_the_new_symbols(dcfm):
    lib = dcfm.load_library()
    for name, nargs in (("dcfm_set_probes", 4), ("dcfm_get_probe_draws", 3)):
        assert name in dcfm.EXPORTS
        assert re.search(rf"\bint\s+{name}\s*\(", HEADER.read_text()), f"{name} not declared in include/dcfm.h"
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs


def test_the_change_is_additive(dcfm):
    from dcfm_amd import _abi
    lib = dcfm.load_library()
    assert _define("DCFM_ABI_VERSION") == 2 == lib.dcfm_abi_version()
    assert _define("DCFM_K_COUNT") == _abi.K_COUNT == 15 == len(_abi.KERNEL_IDS)


def test_null_handle_is_invalid(dcfm):
    from dcfm_amd import _abi
    lib = dcfm.load_library()
    V = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    assert lib.dcfm_set_probes(None, V, 1, 3) == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)
    assert list(V) == [1.0, 2.0, 3.0, 4.0]
    out = (C.c_double * 4)()
    cnt = C.c_int64(-7)
    assert lib.dcfm_get_probe_draws(None, out, C.byref(cnt)) == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)
    assert list(out) == [0.0] * 4 and cnt.value == -7


def test_sampler_methods_exist(dcfm):
    assert callable(dcfm.Sampler.set_probes) and callable(dcfm.Sampler.probe_draws)
    assert "summarize_probes" in dcfm.__all__ and dcfm.summarize_probes is dcfm.diagnostics.summarize_probes
    assert "sd[:, None]" in dcfm.divideconquer.__doc__                  # the unstandardised-covariance recipe


def test_summarize_probes_by_hand(dcfm):
    """Three draws of a 2 x 2 block.  Variances (4, 9), (1, 4), (16, 1) with covariances 3, -1, 2: the
    per-draw correlations are 3/6, -1/2, 2/4 = 0.5, -0.5, 0.5."""
    Q = np.array([[[4.0, 3.0], [3.0, 9.0]], [[1.0, -1.0], [-1.0, 4.0]], [[16.0, 2.0], [2.0, 1.0]]])
    s = dcfm.summarize_probes(Q, q=(0.0, 0.5, 0.75, 1.0))
    assert np.array_equal(s["mean"], np.array([[7.0, 4.0 / 3.0], [4.0 / 3.0, 14.0 / 3.0]]))
    # population sd of (4, 1, 16): mean 7, squared deviations 9 + 36 + 81 = 126 -> sqrt(42)
    assert s["sd"][0, 0] == pytest.approx(np.sqrt(42.0), rel=1e-15)
    assert s["sd"][0, 1] == pytest.approx(np.sqrt(((3 - 4 / 3) ** 2 + (-1 - 4 / 3) ** 2 + (2 - 4 / 3) ** 2) / 3), rel=1e-15)
    # quantiles of (1, 4, 16) at 0, .5, .75, 1 with linear interpolation: 1, 4, 10, 16
    assert np.allclose(s["quantiles"][:, 0, 0], [1.0, 4.0, 10.0, 16.0], rtol=1e-15, atol=0)
    assert np.allclose(s["quantiles"][:, 0, 1], [-1.0, 2.0, 2.5, 3.0], rtol=1e-15, atol=0)
    assert s["corr"].shape == (3, 2, 2)
    assert np.array_equal(s["corr"][:, 0, 1], [0.5, -0.5, 0.5]) and np.array_equal(s["corr"][:, 1, 0], [0.5, -0.5, 0.5])
    assert np.array_equal(s["corr"][:, 0, 0], [1.0] * 3) and np.array_equal(s["corr"][:, 1, 1], [1.0] * 3)
    # quantiles of (-0.5, 0.5, 0.5): -0.5, 0.5, 0.5, 0.5
    assert np.array_equal(s["corr_quantiles"][:, 0, 1], [-0.5, 0.5, 0.5, 0.5])
    # the default levels, a single draw, and an all-zero probe (variance 0: its correlations are NaN)
    one = dcfm.summarize_probes(Q[0])
    assert one["quantiles"].shape == (3, 2, 2) and np.array_equal(one["quantiles"][1], Q[0]) and not one["sd"].any()
    Z = Q.copy()
    Z[:, 1, :] = 0.0
    Z[:, :, 1] = 0.0
    z = dcfm.summarize_probes(Z)
    assert np.array_equal(z["corr"][:, 0, 0], [1.0] * 3) and np.all(np.isnan(z["corr"][:, 0, 1])) and np.all(np.isnan(z["corr"][:, 1, 1]))
    with pytest.raises(ValueError):
        dcfm.summarize_probes(np.zeros((3, 2, 3)))
