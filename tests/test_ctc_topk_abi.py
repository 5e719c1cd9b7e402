"""CPU-side checks of simulst_linear's row top-k epilogue (SIMULST_EPI_ROW_TOPK = 11, csrc/gemm_pick.hip): every refusal is made before a
launch (all pointers below are host memory or null), empty calls are no error, epilogues 7 and 10 stay unknown, and the feature added
no entry point and changed no descriptor."""
import ctypes

import pytest

import abi_pins

E_NULL, E_SHAPE, E_ARG = -1, -2, -4
ROW_TOPK = 11


@pytest.fixture
def handle():
    from simulst_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.simulst_create(ctypes.byref(h), None) == 0
    yield lib, h
    assert lib.simulst_destroy(h) == 0


def _desc(batches=2, rpb=21, N=100, K=64, epi=ROW_TOPK, dtype=1, k=8, keep=0, **kw):
    from simulst_amd._lib import LinearDesc
    d = LinearDesc()
    kp = k + (keep >= 0)
    d.M_batches, d.rows_per_batch, d.N, d.K = batches, rpb, N, K
    d.a_batch_stride, d.a_row_stride, d.c_batch_stride, d.c_row_stride = rpb * K, K, rpb * kp, kp
    d.epilogue, d.dtype, d.scale = epi, dtype, 1.0
    d.aux_rows, d.n_main = k, keep
    for name, v in kw.items():
        setattr(d, name, v)
    return d


def test_row_topk_refusals_on_host_buffers(handle):
    from simulst_amd import _lib
    lib, h = handle
    assert _lib.EPI_ROW_TOPK == ROW_TOPK
    buf = (ctypes.c_int64 * 4096)()
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def call(d, R=None, aux=p):
        return lib.simulst_linear(h, ctypes.byref(d), p, p, None, R, p, aux)

    for dtype in (0, 1):
        # valid shapes, nowhere to put the log-probabilities: a null pointer, not an unknown epilogue
        assert call(_desc(dtype=dtype), aux=None) == E_NULL and b"aux" in lib.simulst_last_error(h)
        # what the epilogue has no meaning for: the row pick's set
        assert call(_desc(dtype=dtype), R=p) == E_ARG and b"residual" in lib.simulst_last_error(h)
        assert call(_desc(dtype=dtype, ln_gamma=p.value, ln_beta=p.value)) == E_ARG and b"LayerNorm" in lib.simulst_last_error(h)
        assert call(_desc(dtype=dtype, N=128, c_head_dim=32, c_head_stride=32 * 21)) == E_ARG and b"head-major" in lib.simulst_last_error(h)
        assert call(_desc(dtype=dtype, N=128, c_head_dim=32, c_tensor_heads=2)) == E_ARG and b"head-major" in lib.simulst_last_error(h)
        assert call(_desc(dtype=dtype, a_lead=8)) == E_ARG and b"a_lead" in lib.simulst_last_error(h)
        # k outside 1..8
        for k in (0, -1, 9, 64):
            assert call(_desc(dtype=dtype, k=k)) == E_SHAPE and b"aux_rows" in lib.simulst_last_error(h), k
        # keep outside [-1, N)
        for keep in (100, 4096, -2):
            assert call(_desc(dtype=dtype, keep=keep)) == E_SHAPE and b"n_main" in lib.simulst_last_error(h), keep
        # no rows: nothing is launched, with or without keep
        assert call(_desc(dtype=dtype, batches=0)) == 0 and call(_desc(dtype=dtype, batches=0, keep=-1, k=1)) == 0
    # the pick's fragment-major rule: bf16 with N % 16 == 0 and K % 32 == 0 only
    assert call(_desc(dtype=0, N=128, w_fragment_major=1)) == E_SHAPE and b"fragment-major" in lib.simulst_last_error(h)
    assert call(_desc(dtype=1, N=100, w_fragment_major=1)) == E_SHAPE and b"fragment-major" in lib.simulst_last_error(h)
    # the refusals of every simulst_linear call still come first
    assert call(_desc(K=60)) == E_SHAPE and call(_desc(dtype=2)) == -3 and call(_desc(N=0)) == E_SHAPE


@pytest.mark.parametrize("epi", [7, 10])
def test_epilogues_7_and_10_are_still_unknown(handle, epi):
    lib, h = handle
    buf = (ctypes.c_int64 * 4096)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    d = _desc(batches=1, rpb=512, N=200, K=64, epi=epi, dtype=0, a_batch_stride=16448, a_row_stride=32, c_batch_stride=102400,
              c_row_stride=200, k=0, keep=0)
    assert lib.simulst_linear(h, ctypes.byref(d), p, p, None, None, p, p) == E_ARG
    assert lib.simulst_last_error(h) == b"simulst_linear: unknown epilogue"


def test_no_new_entry_point_and_no_descriptor_change():
    from simulst_amd import _lib
    assert len(_lib.SIGNATURES) == abi_pins.N_SIGNATURES
    assert _lib.load().simulst_version() == abi_pins.VERSION == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.LinearDesc) == abi_pins.LINEAR_DESC_BYTES
