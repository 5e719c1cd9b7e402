"""CPU-side checks of the transducer's beam-search entry points (csrc/transducer.hip): declared in the header, exported, bound, and
refusing bad arguments with SIMULST_E_ARG before any pointer is looked at (every pointer below is host memory or null)."""
import ctypes
import os
import re
import subprocess

import pytest

import abi_pins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"simulst_joiner_scan_beam": 18, "simulst_joiner_emit_beam": 20, "simulst_transducer_beam_reorder": 11}
E_NULL, E_ARG = -1, -4


def test_declared_exported_and_bound():
    from simulst_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "simulst_hip.h")).read(), flags=re.S)
    so = os.path.join(ROOT, "simulst_amd", "libsimulst_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    lib = _lib.load()
    for n, n_args in NAMES.items():
        m = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)", src)
        assert m and len(m.group(1).split(",")) == n_args, n
        assert re.search(r"\b" + n + r"$", exported, flags=re.M), n
        assert n in _lib.SIGNATURES and len(_lib.SIGNATURES[n]) == n_args and hasattr(lib, n)
    assert lib.simulst_version() == abi_pins.VERSION == _lib.ABI_VERSION           # no descriptor structure changed
    # the library's entry points: 76 before these three
    assert len(_lib.SIGNATURES) == abi_pins.N_SIGNATURES == len(re.findall(r"^\S+ T simulst_\w+$", exported, flags=re.M))


@pytest.fixture
def handle():
    from simulst_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.simulst_create(ctypes.byref(h), None) == 0
    yield lib, h
    assert lib.simulst_destroy(h) == 0


def test_scan_and_emit_refusals_on_host_buffers(handle):
    lib, h = handle
    buf = (ctypes.c_int64 * 4096)()
    p = ctypes.addressof(buf)

    def scan(R=6, group=3, S=4, D=32, V=64, blank=0, n_split=1, dtype=0, finished=p):
        return lib.simulst_joiner_scan_beam(h, p, p, p, p, p, finished, p, p, p, R, group, S, D, V, blank, n_split, dtype)

    def emit(R=6, group=3, S=4, D=32, V=64, blank=0, n_split=1, dtype=0, finished=p):
        return lib.simulst_joiner_emit_beam(h, p, p, p, p, p, p, p, finished, p, p, p, R, group, S, D, V, blank, n_split, dtype)

    for f in (scan, emit):
        # everything joiner_check refuses
        assert f(D=48) == E_ARG and b"D % 32" in lib.simulst_last_error(h)
        assert f(D=0) == E_ARG
        assert f(V=3) == E_ARG and b"V >= 4" in lib.simulst_last_error(h)
        assert f(S=0) == E_ARG and b"S' >= 1" in lib.simulst_last_error(h)
        assert f(dtype=2) == E_ARG and b"dtype" in lib.simulst_last_error(h)
        assert f(dtype=-1) == E_ARG
        assert f(blank=64) == E_ARG and f(blank=-1) == E_ARG
        assert f(n_split=0) == E_ARG and f(n_split=65) == E_ARG
        assert f(R=-3) == E_ARG
        # the row-to-source map
        assert f(group=0) == E_ARG and b"group" in lib.simulst_last_error(h)
        assert f(group=-1) == E_ARG
        assert f(R=7, group=3) == E_ARG and b"group" in lib.simulst_last_error(h)
        assert f(R=0) == 0 and f(R=0, finished=None) == 0      # an empty batch is no error and launches nothing
    # valid arguments with a null pointer: E_NULL, still before any launch; finished and emit_log may be null but P may not
    assert lib.simulst_joiner_scan_beam(h, None, p, p, p, p, None, p, p, p, 6, 3, 4, 32, 64, 0, 1, 0) == E_NULL
    assert lib.simulst_joiner_emit_beam(h, p, p, p, p, p, None, p, None, p, p, None, 6, 3, 4, 32, 64, 0, 1, 0) == E_NULL
    assert lib.simulst_joiner_scan_beam(None, p, p, p, p, p, p, p, p, p, 6, 3, 4, 32, 64, 0, 1, 0) == E_NULL


def test_reorder_refusals_on_host_buffers(handle):
    from simulst_amd import _lib
    lib, h = handle
    buf = (ctypes.c_int64 * 4096)()
    p = ctypes.addressof(buf)

    def desc(R=8, D=32, H=4, n_layers=2, cap=16, dtype=0):
        d = _lib.DecoderDesc()
        d.B, d.D, d.H, d.n_layers, d.cap, d.dtype = R, D, H, n_layers, cap, dtype
        return d

    def layers(n=2, k=p):
        arr = (_lib.DecLayer * 16)()
        for l in range(n):
            arr[l].k_cache, arr[l].v_cache = k, p          # head_step stays null: it is never looked at
        return arr

    def reorder(d, block=4, n_prev=5, src=None, dst=None, pe=p):
        return lib.simulst_transducer_beam_reorder(h, ctypes.byref(d), src or layers(), dst or layers(), pe, p, p, None, block, n_prev, p)

    assert reorder(desc(), block=0) == E_ARG and b"block" in lib.simulst_last_error(h)
    assert reorder(desc(), block=-2) == E_ARG
    assert reorder(desc(), block=3) == E_ARG and b"block" in lib.simulst_last_error(h)           # R % block
    assert reorder(desc(), block=16) == E_ARG                                                     # block > R
    assert reorder(desc(), n_prev=17) == E_ARG and b"n_prev" in lib.simulst_last_error(h)         # n_prev > cap
    assert reorder(desc(), n_prev=-1) == E_ARG
    assert reorder(desc(dtype=2)) == E_ARG and b"dtype" in lib.simulst_last_error(h)
    assert reorder(desc(n_layers=17)) == E_ARG and reorder(desc(n_layers=0)) == E_ARG
    assert reorder(desc(D=36)) == E_ARG                                                           # head_dim 9: no 16-byte copies
    assert reorder(desc(cap=0), n_prev=0) == E_ARG
    assert reorder(desc(R=-1)) == E_ARG
    assert reorder(desc(R=0)) == 0 and reorder(desc(R=0), block=40) == 0                          # no rows: nothing to do
    # valid arguments with a null pointer: E_NULL, before any launch
    assert reorder(desc(), pe=None) == E_NULL
    assert reorder(desc(), src=layers(k=None)) == E_NULL
    assert lib.simulst_transducer_beam_reorder(h, None, layers(), layers(), p, p, p, None, 4, 5, p) == E_NULL
    assert lib.simulst_transducer_beam_reorder(None, ctypes.byref(desc()), layers(), layers(), p, p, p, None, 4, 5, p) == E_NULL
