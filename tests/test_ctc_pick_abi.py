"""CPU-side checks of simulst_linear's row-pick epilogue (SIMULST_EPI_ROW_PICK = 8, csrc/gemm_pick.hip): every refusal is made before a
launch (all pointers below are host memory or null), an empty call is no error, epilogue 7 stays unknown, and the feature added no
entry point and changed no descriptor."""
import ctypes

import pytest

import abi_pins

E_NULL, E_ARG = -1, -4
ROW_PICK = 8


@pytest.fixture
def handle():
    from simulst_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.simulst_create(ctypes.byref(h), None) == 0
    yield lib, h
    assert lib.simulst_destroy(h) == 0


def _desc(batches=2, rpb=21, N=100, K=64, epi=ROW_PICK, dtype=1, **kw):
    from simulst_amd._lib import LinearDesc
    d = LinearDesc()
    d.M_batches, d.rows_per_batch, d.N, d.K = batches, rpb, N, K
    d.a_batch_stride, d.a_row_stride, d.c_batch_stride, d.c_row_stride = rpb * K, K, rpb, 1
    d.epilogue, d.dtype, d.scale = epi, dtype, 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_row_pick_refusals_on_host_buffers(handle):
    from simulst_amd import _lib
    lib, h = handle
    assert _lib.EPI_ROW_PICK == ROW_PICK
    buf = (ctypes.c_int64 * 4096)()
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def call(d, R=None, aux=p):
        return lib.simulst_linear(h, ctypes.byref(d), p, p, None, R, p, aux)

    for dtype in (0, 1):
        # valid shapes, no aux: a null pointer, not an argument error
        assert call(_desc(dtype=dtype), aux=None) == E_NULL and b"aux" in lib.simulst_last_error(h)
        # what the epilogue has no meaning for
        assert call(_desc(dtype=dtype), R=p) == E_ARG and b"residual" in lib.simulst_last_error(h)
        assert call(_desc(dtype=dtype, ln_gamma=p.value, ln_beta=p.value)) == E_ARG and b"LayerNorm" in lib.simulst_last_error(h)
        assert call(_desc(dtype=dtype, ln_gamma=p.value)) == E_ARG
        assert call(_desc(dtype=dtype, N=128, c_head_dim=32, c_head_stride=32 * 21)) == E_ARG and b"head-major" in lib.simulst_last_error(h)
        # no rows: nothing is launched
        assert call(_desc(dtype=dtype, batches=0)) == 0
    # the refusals of every simulst_linear call still come first
    assert call(_desc(K=60)) == -2 and call(_desc(dtype=2)) == -3 and call(_desc(N=0)) == -2
    # fragment-major weights only where simulst_pack_fragment_major's layout applies to the matrix-core form
    assert call(_desc(w_fragment_major=1)) == -2 and b"fragment-major" in lib.simulst_last_error(h)          # N = 100
    assert call(_desc(dtype=0, N=128, w_fragment_major=1)) == -2


def test_epilogue_7_is_still_unknown(handle):
    """the row of tests/golden/g26_linear_plan.json that records value 7 as refused: the new epilogue is 8"""
    lib, h = handle
    buf = (ctypes.c_int64 * 4096)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    d = _desc(batches=1, rpb=512, N=200, K=64, epi=7, dtype=0, a_batch_stride=16448, a_row_stride=32, c_batch_stride=102400,
              c_row_stride=200)
    assert lib.simulst_linear(h, ctypes.byref(d), p, p, None, None, p, p) == E_ARG
    assert lib.simulst_last_error(h) == b"simulst_linear: unknown epilogue"


def test_no_new_entry_point_and_no_descriptor_change():
    from simulst_amd import _lib
    assert len(_lib.SIGNATURES) == abi_pins.N_SIGNATURES
    assert _lib.load().simulst_version() == abi_pins.VERSION == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.LinearDesc) == abi_pins.LINEAR_DESC_BYTES
