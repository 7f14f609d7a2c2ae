"""The sparsity reweighting entry points are declared in include/fasst_hip.h,
exported by libfasst_hip.so and bound by the ctypes table with matching
signatures.

CPU-only: no compute call is made."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# symbol -> the ctypes signature its declaration translates to
_vp, _ip, _dp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
NEW = {
    "fasst_sf_set_sparsity": [_vp, _ip],
    "fasst_sf_reweigh": [_vp, ctypes.c_double],
    "fasst_sf_run_sparse": [_vp, ctypes.c_int, _dp, ctypes.c_double, _dp, _dp, _ip, _ip],
}
CTYPE = {"fasst_ctx *": _vp, "const int *": _ip, "int *": _ip, "const double *": _dp,
         "double *": _dp, "int": ctypes.c_int, "double": ctypes.c_double}


def declarations():
    """{name: [argument type, ...]} of every int prototype in include/fasst_hip.h."""
    src = open(os.path.join(ROOT, "include", "fasst_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(\w+)\s*\(([^)]*)\)\s*;", src):
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            types.append(re.sub(r"\s*\w+$", "", a) if not a.endswith("*") else a)
        out[name] = types
    return out


@pytest.mark.parametrize("name", sorted(NEW))
def test_declared_exported_and_bound(name):
    from pyfasst_amd import _lib
    decl = declarations()
    assert name in decl, name
    assert [CTYPE[t] for t in decl[name]] == NEW[name], decl[name]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int
    assert list(argtypes) == NEW[name]
    fn = getattr(_lib.lib, name)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == NEW[name]


def test_run_sparse_is_run_with_a_sigma_row():
    decl = declarations()
    run, sparse = decl["fasst_sf_run"], decl["fasst_sf_run_sparse"]
    assert sparse[:4] == run[:4] and sparse[4] == "const double *" and sparse[5:] == run[4:]


def test_refusals_need_no_device():
    """A null context or a context without a two-factor model is refused with
    FASST_ERR_SHAPE before any device call."""
    from pyfasst_amd import _lib
    lib = _lib.lib
    assert lib.fasst_sf_set_sparsity(None, None) == _lib.FASST_ERR_SHAPE
    assert lib.fasst_sf_reweigh(None, 9.0) == _lib.FASST_ERR_SHAPE
    assert "two-factor" in _lib.last_error()
    assert lib.fasst_sf_run_sparse(None, 1, None, 1.0, None, None, None, None) == \
        _lib.FASST_ERR_SHAPE


def test_engine_and_kernel_slots():
    from pyfasst_amd import _lib
    from pyfasst_amd.engine import Engine
    for meth in ("sf_set_sparsity", "sf_reweigh", "sf_run_sparse"):
        assert callable(getattr(Engine, meth))
    names = [_lib.lib.fasst_kernel_name(i).decode() for i in range(32)]
    assert {"k_sf_bary", "k_sf_sparsify"} <= set(names)
