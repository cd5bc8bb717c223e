"""CPU tests of the missing-data boundary (dcfm_set_missing / dcfm_get_imputed): the header, the binding and the
library agree on both symbols (three and five arguments), a null handle is refused with nothing written, the ABI
version and the kernel-id count stay (the change is additive), the Philox site is the free one the header names,
and the Sampler methods, the driver's argument and the package exports exist -- all without a GPU."""
import ctypes as C
import inspect
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "dcfm.h"
PHILOX = next(ROOT.glob("*_amd/csrc/philox.h"))


def _define(name):
    m = re.search(rf"^#define\s+{name}\s+(0x[0-9a-fA-F]+|\d+)u?\b", HEADER.read_text(), re.M)
    assert m, f"{name} not defined in include/dcfm.h"
    return int(m.group(1), 0)


def test_library_resolves_the_new_symbols(dcfm):
    lib = dcfm.load_library()
    for name, nargs in (("dcfm_set_missing", 3), ("dcfm_get_imputed", 5)):
        assert name in dcfm.EXPORTS
        assert re.search(rf"\bint\s+{name}\s*\(", HEADER.read_text()), f"{name} not declared in include/dcfm.h"
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
    assert lib.dcfm_set_missing.argtypes[1] is C.POINTER(C.c_uint8) and lib.dcfm_set_missing.argtypes[2] is C.c_int64


def test_the_change_is_additive(dcfm):
    from dcfm_amd import _abi
    lib = dcfm.load_library()
    assert _define("DCFM_ABI_VERSION") == 2 == lib.dcfm_abi_version()
    assert _define("DCFM_K_COUNT") == _abi.K_COUNT == 15 == len(_abi.KERNEL_IDS)


def test_null_handle_is_invalid(dcfm):
    from dcfm_amd import _abi
    lib = dcfm.load_library()
    mk = (C.c_uint8 * 4)(1, 0, 0, 1)
    assert lib.dcfm_set_missing(None, mk, 3) == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)
    bufs = [(C.c_double * 4)() for _ in range(3)]
    cnt = C.c_int64(-7)
    assert lib.dcfm_get_imputed(None, *bufs, C.byref(cnt)) == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)
    assert all(list(b) == [0.0] * 4 for b in bufs) and cnt.value == -7


def test_the_site_is_the_one_the_header_names():
    import missing_cases as mc
    m = re.search(r"SITE_IMPUTE\s*=\s*(\d+)", PHILOX.read_text())
    assert m and int(m.group(1)) == mc.SITE_IMPUTE == 13
    sites = [int(x) for x in re.findall(r"SITE_\w+\s*=\s*(\d+)", PHILOX.read_text())]
    assert len(sites) == len(set(sites))                         # no site is used twice
    assert "site 13" in HEADER.read_text() and "DCFM_FLAG_INJECT_DRAWS these normals still come from Philox" in HEADER.read_text()


def test_python_surface_exists(dcfm):
    assert callable(dcfm.Sampler.set_missing) and callable(dcfm.Sampler.imputed)
    par = inspect.signature(dcfm.Sampler.set_missing).parameters
    assert list(par) == ["self", "mask", "capacity"] and par["capacity"].default is None
    for word in ("mean", "sd_between", "sd_total", "count", "mask"):
        assert word in dcfm.Sampler.imputed.__doc__, word
    assert "DCFM_ERR_UNSUPPORTED" in dcfm.Sampler.set_missing.__doc__
    par = inspect.signature(dcfm.divideconquer).parameters
    assert "impute" in par and par["impute"].default is False
    assert list(par)[list(par).index("predict") + 1] == "impute"
    assert "set_missing" in dcfm.divideconquer.__doc__ and "device_ingest" in dcfm.divideconquer.__doc__
    for name in ("preprocess_missing", "partition_standardize_missing", "observed_moments", "unstandardize_imputation"):
        assert name in dcfm.__all__ and getattr(dcfm, name) is getattr(dcfm.driver, name)
