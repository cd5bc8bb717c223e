"""CPU tests of the log-likelihood draws' boundary (dcfm_set_loglik / dcfm_get_loglik): the binding lists and
resolves both symbols (two and four arguments), a null handle is refused with nothing written, the ABI version
and the kernel-id count stay (the change is additive), and the Sampler methods, the driver's argument and the
diagnostics export exist -- all without a GPU."""
import ctypes as C
import inspect
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "dcfm.h"


def _define(name):
    m = re.search(rf"^#define\s+{name}\s+(0x[0-9a-fA-F]+|\d+)u?\b", HEADER.read_text(), re.M)
    assert m, f"{name} not defined in include/dcfm.h"
    return int(m.group(1), 0)


def test_library_resolves_the_new_symbols(dcfm):
    lib = dcfm.load_library()
    for name, nargs in (("dcfm_set_loglik", 2), ("dcfm_get_loglik", 4)):
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
    assert lib.dcfm_set_loglik(None, 3) == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)
    q, ld = (C.c_double * 4)(), (C.c_double * 2)()
    cnt = C.c_int64(-7)
    assert lib.dcfm_get_loglik(None, q, ld, C.byref(cnt)) == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)
    assert list(q) == [0.0] * 4 and list(ld) == [0.0] * 2 and cnt.value == -7


def test_python_surface_exists(dcfm):
    assert callable(dcfm.Sampler.set_loglik) and callable(dcfm.Sampler.loglik_draws)
    assert "waic" in dcfm.__all__ and dcfm.waic is dcfm.diagnostics.waic
    assert "loglik" in inspect.signature(dcfm.divideconquer).parameters
    assert inspect.signature(dcfm.divideconquer).parameters["loglik"].default is False
    assert "set_loglik" in dcfm.divideconquer.__doc__
    for word in ("sum(log sd)", "same Y", "0.4"):                 # units, comparability, the warning sign
        assert word in dcfm.waic.__doc__, word
