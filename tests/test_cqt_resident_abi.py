"""The entry points that keep a MinQT / CQT model on the device are declared in
include/fasst_cqt.h, exported by libfasst_hip.so and bound by the ctypes table
with the declared number of arguments.

CPU-only: no compute call is made."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# symbol -> number of arguments
NEW = {
    "fasst_set_audio_cqt": 4,
    "fasst_separate_waveforms_cqt": 5,
    "fasst_sf_separate_waveforms_cqt": 7,
    "fasst_spatial_filter_waveforms_cqt": 4,
    "cqt_batch_info": 3,
}


def declarations():
    """{name: argument list} of every prototype in include/fasst_cqt.h."""
    src = open(os.path.join(ROOT, "include", "fasst_cqt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(\w+)\s*\(([^)]*)\)\s*;", src):
        out[name] = [a.strip() for a in args.split(",") if a.strip() and a.strip() != "void"]
    return out


@pytest.mark.parametrize("name", sorted(NEW))
def test_declared_exported_and_bound(name):
    from pyfasst_amd import _lib
    decl = declarations()
    assert name in decl, name
    assert len(decl[name]) == NEW[name], decl[name]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name)
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int
    assert len(argtypes) == len(decl[name])
    # contexts are opaque pointers, lengths are C longs
    for arg, ct in zip(decl[name], argtypes):
        if arg.startswith(("fasst_ctx *", "cqt_ctx *")):
            assert ct is ctypes.c_void_p, (name, arg)
        if arg.startswith("long ") and "*" not in arg:
            assert ct is ctypes.c_long, (name, arg)


def test_model_entry_points_take_both_contexts():
    decl = declarations()
    for name in NEW:
        if name.startswith("fasst_"):
            assert decl[name][0].startswith("fasst_ctx *"), name
            assert decl[name][1].startswith("cqt_ctx *"), name


def test_refusals_need_no_device():
    """Null contexts are refused with FASST_ERR_SHAPE before any device call."""
    from pyfasst_amd import _lib
    lib = _lib.lib
    assert lib.fasst_set_audio_cqt(None, None, None, 10) == _lib.FASST_ERR_SHAPE
    assert lib.fasst_separate_waveforms_cqt(None, None, None, 10, None) == _lib.FASST_ERR_SHAPE
    assert lib.fasst_spatial_filter_waveforms_cqt(None, None, 10, None) == _lib.FASST_ERR_SHAPE
    assert lib.cqt_batch_info(None, None, None) == _lib.FASST_ERR_SHAPE
