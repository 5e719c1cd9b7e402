"""CPU-side checks of simulst_mma_retire_rows (offline decode with hypotheses finalised at EOS): declared, exported and bound,
and bad arguments are refused before anything reaches the device."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "simulst_mma_retire_rows"


def test_declared_exported_and_bound():
    from simulst_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "simulst_hip.h")).read(), flags=re.S)
    assert re.search(r"\b" + NAME + r"\s*\(", src)
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME]) == 14
    so = os.path.join(ROOT, "simulst_amd", "libsimulst_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert NAME in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert hasattr(_lib.load(), NAME)


@pytest.fixture
def handle():
    from simulst_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.simulst_create(ctypes.byref(h), None) == 0
    yield lib, h
    assert lib.simulst_destroy(h) == 0


def _args(lib_mod, n_layers=2):
    """a descriptor and per-slot arrays of host memory: every pointer non-null, never dereferenced by a refused call"""
    d = lib_mod.DecoderDesc()
    d.B, d.D, d.H, d.n_layers, d.cap, d.S_cap, d.dtype = 64, 256, 4, n_layers, 32, 64, lib_mod.BF16
    buf = (ctypes.c_int64 * 4096)()
    p = ctypes.addressof(buf)
    d.n_prev = d.enc_len = p
    layers = (lib_mod.DecLayer * n_layers)()
    for L in layers:
        L.k_cache = L.v_cache = L.Kmono = L.V = L.head_step = p
    return d, layers, buf, p


def _call(lib, h, d, layers, p, *, n_steps=8, rows=64, B=64, U=40, null=None):
    ptr = {k: (None if k == null else p) for k in ("chunk", "slot_row", "row_cap", "last", "hyp", "result")}
    return lib.simulst_mma_retire_rows(h, None if null == "desc" else ctypes.byref(d), None if null == "layers" else layers,
                                       ptr["chunk"], n_steps, rows, B, ptr["slot_row"], ptr["row_cap"], ptr["last"], ptr["hyp"],
                                       U, None, ptr["result"])


def test_bad_arguments_are_refused(handle):
    from simulst_amd import _lib
    lib, h = handle
    d, layers, buf, p = _args(_lib)
    assert lib.simulst_mma_retire_rows(None, ctypes.byref(d), layers, p, 8, 64, 64, p, p, p, p, 40, None, p) == -1
    for null in ("desc", "layers", "chunk", "slot_row", "row_cap", "last", "hyp", "result"):
        assert _call(lib, h, d, layers, p, null=null) == -1, null
        assert b"null pointer" in lib.simulst_last_error(h)
    assert _call(lib, h, d, layers, p, rows=65, B=64) == -2 and b"rows" in lib.simulst_last_error(h)
    assert _call(lib, h, d, layers, p, rows=0) == -2
    assert _call(lib, h, d, layers, p, n_steps=0) == -2 and b"n_steps" in lib.simulst_last_error(h)
    assert _call(lib, h, d, layers, p, n_steps=-3) == -2
    assert _call(lib, h, d, layers, p, U=0) == -2
    d.dtype = 7
    assert _call(lib, h, d, layers, p) == -3
    d.dtype = _lib.BF16
    d.H = 3                                                   # head_dim not a multiple of 8
    assert _call(lib, h, d, layers, p) == -2
    d.H = 4
    d.n_prev = None
    assert _call(lib, h, d, layers, p) == -1
    d.n_prev = p
    layers[1].head_step = None
    assert _call(lib, h, d, layers, p) == -1 and b"head_step" in lib.simulst_last_error(h)
    d2, layers2, buf2, p2 = _args(_lib, n_layers=17)         # more layers than the kernels carry pointers for
    assert _call(lib, h, d2, layers2, p2) == -2
