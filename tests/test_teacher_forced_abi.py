"""CPU-side checks of the whole-target (teacher-forced) entry points (csrc/teacher_forced.hip): declared, exported and bound, and
bad arguments are refused before anything reaches the device."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"simulst_decoder_self_attention_causal": 8, "simulst_mma_energy": 17, "simulst_mma_softmax": 7, "simulst_mma_context": 11}


def test_declared_exported_and_bound():
    from simulst_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "simulst_hip.h")).read(), flags=re.S)
    so = os.path.join(ROOT, "simulst_amd", "libsimulst_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = _lib.load()
    for name, n_args in NAMES.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name                  # the header's own arity
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == n_args, name
        assert name in exported, name
        assert hasattr(lib, name), name
    assert (_lib.ENERGY_SOFT, _lib.ENERGY_MONOTONIC, _lib.ENERGY_WAITK) == (0, 1, 2)


@pytest.fixture
def handle():
    from simulst_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.simulst_create(ctypes.byref(h), None) == 0
    yield lib, h
    assert lib.simulst_destroy(h) == 0


@pytest.fixture
def p():
    """host memory for every pointer argument: never dereferenced by a refused call"""
    buf = (ctypes.c_int64 * 4096)()
    yield ctypes.addressof(buf)
    del buf


def test_causal_self_attention_refuses_bad_arguments(handle, p):
    lib, h = handle
    f = lib.simulst_decoder_self_attention_causal
    assert f(None, p, p, 2, 9, 2, 16, 0) == -1
    assert f(h, None, p, 2, 9, 2, 16, 0) == -1 and b"null pointer" in lib.simulst_last_error(h)
    assert f(h, p, None, 2, 9, 2, 16, 0) == -1
    assert f(h, p, p, 2, 9, 2, 16, 7) == -3
    assert f(h, p, p, 2, 9, 2, 128, 0) == -2 and b"head_dim" in lib.simulst_last_error(h)
    assert f(h, p, p, 2, 9, 0, 16, 0) == -2
    assert f(h, p, p, -1, 9, 2, 16, 0) == -2
    assert f(h, p, p, 40000, 9, 2, 16, 0) == -2            # B * H beyond a grid dimension
    assert f(h, p, p, 0, 9, 2, 16, 0) == 0                 # nothing to do: no launch


def _energy(lib, h, p, *, q=True, K=True, out=True, B=2, U=9, S=21, S_cap=24, H=2, d=16, ratio=2, mode=1, k=3, dtype=0):
    return lib.simulst_mma_energy(h, p if q else None, p if K else None, p if out else None, None, 0.0, 0.3, B, U, S, S_cap, H, d, ratio,
                                  mode, k, dtype)


def test_energy_refuses_bad_arguments(handle, p):
    lib, h = handle
    assert lib.simulst_mma_energy(None, p, p, p, None, 0.0, 0.3, 2, 9, 21, 24, 2, 16, 2, 1, 3, 0) == -1
    assert _energy(lib, h, p, out=False) == -1 and b"null pointer" in lib.simulst_last_error(h)
    for mode in (0, 1):
        assert _energy(lib, h, p, q=False, mode=mode) == -1
        assert _energy(lib, h, p, K=False, mode=mode) == -1
    assert _energy(lib, h, p, mode=3) == -4 and _energy(lib, h, p, mode=-1) == -4
    assert _energy(lib, h, p, mode=2, k=0) == -4 and b"lagging" in lib.simulst_last_error(h)
    assert _energy(lib, h, p, dtype=5) == -3
    assert _energy(lib, h, p, S=25) == -2                   # S beyond the cache rows
    assert _energy(lib, h, p, S=0) == -2
    assert _energy(lib, h, p, ratio=0) == -2
    assert _energy(lib, h, p, d=65) == -2
    assert _energy(lib, h, p, S=5, ratio=-8) == -2          # 'last' pooling of a source shorter than one window
    assert _energy(lib, h, p, S_cap=5000, S=21) == -2
    assert _energy(lib, h, p, U=0) == 0
    assert _energy(lib, h, p, q=False, K=False, mode=2, B=0) == 0          # wait-k reads neither q nor K


def test_softmax_and_context_refuse_bad_arguments(handle, p):
    lib, h = handle
    assert lib.simulst_mma_softmax(None, p, None, 2, 9, 21, 2) == -1
    assert lib.simulst_mma_softmax(h, None, None, 2, 9, 21, 2) == -1
    assert lib.simulst_mma_softmax(h, p, None, 2, 9, 0, 2) == -2
    assert lib.simulst_mma_softmax(h, p, None, 2, 9, 21, 0) == -2
    assert lib.simulst_mma_softmax(h, p, None, 0, 9, 21, 2) == 0
    f = lib.simulst_mma_context
    assert f(None, p, p, p, 2, 9, 21, 24, 2, 16, 0) == -1
    for null in range(3):
        a = [p, p, p]
        a[null] = None
        assert f(h, *a, 2, 9, 21, 24, 2, 16, 0) == -1 and b"null pointer" in lib.simulst_last_error(h)
    assert f(h, p, p, p, 2, 9, 21, 24, 2, 16, 9) == -3
    assert f(h, p, p, p, 2, 9, 25, 24, 2, 16, 0) == -2
    assert f(h, p, p, p, 2, 9, 21, 24, 2, 80, 0) == -2
    assert f(h, p, p, p, 2, 0, 21, 24, 2, 16, 0) == 0
