"""CPU-side checks of the transducer entry points (csrc/transducer.hip): declared in the header, exported, bound, and refusing bad
arguments with SIMULST_E_ARG before any pointer is looked at (every pointer below is host memory or null)."""
import ctypes
import os
import re
import subprocess

import pytest

import abi_pins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("simulst_transducer_pool", "simulst_joiner_scan", "simulst_joiner_emit", "simulst_joiner_mask_blank")
E_NULL, E_ARG = -1, -4


def test_declared_exported_and_bound():
    from simulst_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "simulst_hip.h")).read(), flags=re.S)
    so = os.path.join(ROOT, "simulst_amd", "libsimulst_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), n
        assert re.search(r"\b" + n + r"$", exported, flags=re.M), n
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert re.search(r"global:\s*simulst_\*;", open(os.path.join(ROOT, "simulst_amd", "csrc", "exports.map")).read())
    assert lib.simulst_version() == abi_pins.VERSION == _lib.ABI_VERSION


@pytest.fixture
def handle():
    from simulst_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.simulst_create(ctypes.byref(h), None) == 0
    yield lib, h
    assert lib.simulst_destroy(h) == 0


def test_refusals_on_host_buffers(handle):
    lib, h = handle
    buf = (ctypes.c_int64 * 4096)()
    p = ctypes.addressof(buf)

    def scan(B=2, S=4, D=32, V=64, blank=0, n_split=1, dtype=0):
        return lib.simulst_joiner_scan(h, *[p] * 8, B, S, D, V, blank, n_split, dtype)

    def emit(B=2, S=4, D=32, V=64, blank=0, n_split=1, dtype=0):
        return lib.simulst_joiner_emit(h, *[p] * 9, B, S, D, V, blank, n_split, dtype)

    def pool(B=2, S_in=8, D=32, bs=256, T=8, k=4, dtype=0):
        return lib.simulst_transducer_pool(h, p, p, p, p, B, S_in, D, bs, T, k, dtype)

    for f in (scan, emit):
        assert f(D=48) == E_ARG and b"D % 32" in lib.simulst_last_error(h)
        assert f(D=0) == E_ARG
        assert f(V=3) == E_ARG and b"V >= 4" in lib.simulst_last_error(h)
        assert f(S=0) == E_ARG and b"S' >= 1" in lib.simulst_last_error(h)
        assert f(dtype=2) == E_ARG and b"dtype" in lib.simulst_last_error(h)
        assert f(dtype=-1) == E_ARG
        assert f(blank=64) == E_ARG and f(blank=-1) == E_ARG
        assert f(n_split=0) == E_ARG and f(n_split=65) == E_ARG
        assert f(B=0) == 0                                   # an empty batch is no error and launches nothing
    assert pool(k=0) == E_ARG and b"k >= 1" in lib.simulst_last_error(h)
    assert pool(T=0) == E_ARG and b"S' >= 1" in lib.simulst_last_error(h)
    assert pool(D=40) == E_ARG and b"D % 32" in lib.simulst_last_error(h)
    assert pool(dtype=7) == E_ARG and b"dtype" in lib.simulst_last_error(h)
    assert pool(T=9) == E_ARG                                # T beyond the buffer's rows
    assert pool(bs=100) == E_ARG                             # rows of one utterance overlapping the next
    assert pool(B=0) == 0
    assert lib.simulst_joiner_mask_blank(h, p, p, 2, 3, 0) == E_ARG
    assert lib.simulst_joiner_mask_blank(h, p, p, 2, 64, 64) == E_ARG
    assert lib.simulst_joiner_mask_blank(h, p, p, 0, 64, 0) == 0
    # valid arguments with a null pointer: E_NULL, still before any launch
    assert lib.simulst_joiner_scan(h, None, p, p, p, p, p, p, p, 2, 4, 32, 64, 0, 1, 0) == E_NULL
    assert lib.simulst_transducer_pool(h, p, None, p, p, 2, 8, 32, 256, 8, 4, 0) == E_NULL
    assert lib.simulst_joiner_scan(None, *[p] * 8, 2, 4, 32, 64, 0, 1, 0) == E_NULL
