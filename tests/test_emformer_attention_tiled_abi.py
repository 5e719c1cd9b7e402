"""CPU-side checks of simulst_emformer_attention's argument handling now that segments of more than 128 keys are served
(csrc/emformer_attn_tiled.hip): the geometry refusal is gone, every other refusal keeps its status and message, and the ABI version
did not move.  Every pointer below is host memory: each call returns before any launch."""
import ctypes

import pytest

import abi_pins

E_SHAPE, E_ARG = -2, -4
F32, BF16 = 0, 1


@pytest.fixture
def handle():
    from simulst_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.simulst_create(ctypes.byref(h), None) == 0
    yield lib, h
    assert lib.simulst_destroy(h) == 0


def _call(lib, h, *, lc_k=False, lc_v=False, **kw):
    from simulst_amd import _lib
    f = dict(B=0, T=130, D=128, H=2, S=64, R=8, Lc=64, M=5, n_mem=2, n_seg=3, use_summary=1, dtype=F32)
    f.update(kw)
    d = _lib.EmfAttnDesc(*(f[n] for n, _ in _lib.EmfAttnDesc._fields_))
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)
    return lib.simulst_emformer_attention(h, ctypes.byref(d), p, p, p if lc_k else None, p if lc_v else None, None, None, p)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_empty_batch_beyond_128_keys_is_accepted(handle, dtype):
    """S, R, Lc, M = 64, 8, 64, 5 is 141 keys per segment: refused with SIMULST_E_SHAPE before the blocked kernels existed."""
    lib, h = handle
    assert _call(lib, h, dtype=dtype) == 0
    assert _call(lib, h, dtype=dtype, T=64, n_seg=1, n_mem=5, lc_k=True, lc_v=True) == 0          # streaming form
    assert _call(lib, h, dtype=dtype, S=16, Lc=32, T=48) == 0                                      # 61 keys: as before


def test_other_refusals_keep_status_and_message(handle):
    lib, h = handle
    assert _call(lib, h, D=130) == E_SHAPE and b"head_dim must be <= 64" in lib.simulst_last_error(h)          # head_dim 65
    assert _call(lib, h, D=128, H=3) == E_SHAPE and b"head_dim must be <= 64" in lib.simulst_last_error(h)     # D % H
    assert _call(lib, h, n_seg=2) == E_SHAPE and b"n_seg != ceil(T/S)" in lib.simulst_last_error(h)
    assert _call(lib, h, n_seg=4) == E_SHAPE and b"n_seg != ceil(T/S)" in lib.simulst_last_error(h)
    assert _call(lib, h, T=64, n_seg=1, lc_k=True) == E_ARG and b"lc_k/lc_v" in lib.simulst_last_error(h)
    assert _call(lib, h, T=64, n_seg=1, lc_v=True) == E_ARG and b"lc_k/lc_v" in lib.simulst_last_error(h)
    assert _call(lib, h, lc_k=True, lc_v=True) == E_SHAPE and b"streaming needs one segment" in lib.simulst_last_error(h)
    assert _call(lib, h, dtype=2) == -3 and b"dtype" in lib.simulst_last_error(h)
    # the same refusals at a geometry the earlier kernels serve
    small = dict(S=16, Lc=32, T=48)
    assert _call(lib, h, D=130, **small) == E_SHAPE
    assert _call(lib, h, n_seg=2, **small) == E_SHAPE and b"n_seg != ceil(T/S)" in lib.simulst_last_error(h)


def test_version_unchanged():
    from simulst_amd import _lib
    assert _lib.load().simulst_version() == abi_pins.VERSION == _lib.ABI_VERSION
