"""CPU-side checks of the CTC scoring additions: simulst_linear's row-gather epilogue (SIMULST_EPI_ROW_GATHER = 9, csrc/gemm_pick.hip)
and the sum mode of simulst_ctc_best_alignment (out == NULL, csrc/ctc_align.hip).  Every refusal is made before a launch (all pointers
below are host memory or null), empty calls are no error, epilogues 7 and 10 stay unknown, and the feature added no entry point and
changed no descriptor."""
import ctypes

import pytest

import abi_pins

E_NULL, E_SHAPE, E_ARG = -1, -2, -4
ROW_GATHER = 9


@pytest.fixture
def handle():
    from simulst_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.simulst_create(ctypes.byref(h), None) == 0
    yield lib, h
    assert lib.simulst_destroy(h) == 0


def _desc(batches=2, rpb=21, N=100, K=64, epi=ROW_GATHER, dtype=1, aux_rows=5, **kw):
    from simulst_amd._lib import LinearDesc
    d = LinearDesc()
    d.M_batches, d.rows_per_batch, d.N, d.K = batches, rpb, N, K
    d.a_batch_stride, d.a_row_stride, d.c_batch_stride, d.c_row_stride = rpb * K, K, rpb * aux_rows, aux_rows
    d.epilogue, d.dtype, d.scale = epi, dtype, 1.0
    d.aux_rows, d.aux_batch_stride = aux_rows, aux_rows
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_row_gather_refusals_on_host_buffers(handle):
    from simulst_amd import _lib
    lib, h = handle
    assert _lib.EPI_ROW_GATHER == ROW_GATHER
    buf = (ctypes.c_int64 * 4096)()
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def call(d, R=None, aux=p):
        return lib.simulst_linear(h, ctypes.byref(d), p, p, None, R, p, aux)

    for dtype in (0, 1):
        # valid shapes, no labels: a null pointer, not an unknown epilogue
        assert call(_desc(dtype=dtype), aux=None) == E_NULL and b"aux" in lib.simulst_last_error(h)
        # what the epilogue has no meaning for: the row pick's set
        assert call(_desc(dtype=dtype), R=p) == E_ARG and b"residual" in lib.simulst_last_error(h)
        assert call(_desc(dtype=dtype, ln_gamma=p.value, ln_beta=p.value)) == E_ARG and b"LayerNorm" in lib.simulst_last_error(h)
        assert call(_desc(dtype=dtype, N=128, c_head_dim=32, c_head_stride=32 * 21)) == E_ARG and b"head-major" in lib.simulst_last_error(h)
        assert call(_desc(dtype=dtype, a_lead=8)) == E_ARG and b"a_lead" in lib.simulst_last_error(h)
        # row-major weights only, even where the row pick takes fragment-major ones (bf16, N % 16 == 0, K % 32 == 0)
        assert call(_desc(dtype=dtype, N=128, w_fragment_major=1)) == E_SHAPE and b"fragment-major" in lib.simulst_last_error(h)
        # no label to gather at
        assert call(_desc(dtype=dtype, aux_rows=0)) == E_SHAPE and b"aux_rows" in lib.simulst_last_error(h)
        assert call(_desc(dtype=dtype, aux_rows=-3)) == E_SHAPE
        # no rows: nothing is launched
        assert call(_desc(dtype=dtype, batches=0)) == 0
    # the refusals of every simulst_linear call still come first
    assert call(_desc(K=60)) == E_SHAPE and call(_desc(dtype=2)) == -3 and call(_desc(N=0)) == E_SHAPE


@pytest.mark.parametrize("epi", [7, 10])
def test_epilogues_7_and_10_are_still_unknown(handle, epi):
    lib, h = handle
    buf = (ctypes.c_int64 * 4096)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    d = _desc(batches=1, rpb=512, N=200, K=64, epi=epi, dtype=0, a_batch_stride=16448, a_row_stride=32, c_batch_stride=102400,
              c_row_stride=200)
    assert lib.simulst_linear(h, ctypes.byref(d), p, p, None, None, p, p) == E_ARG
    assert lib.simulst_last_error(h) == b"simulst_linear: unknown epilogue"


def test_sum_mode_of_ctc_best_alignment_on_host_buffers(handle):
    lib, h = handle
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def call(N, out, nll, scratch=None):
        return lib.simulst_ctc_best_alignment(h, p, 8, 4, 1, p, 3, p, p, 5, N, 3, 0, 0, scratch, out, nll)

    # no path and no place for the sum: nothing to compute
    assert call(2, None, None) == E_NULL and b"neg_log_likelihood" in lib.simulst_last_error(h)
    assert call(0, None, None) == E_NULL
    # the sum needs neither out nor scratch; no utterance: nothing is launched
    assert call(0, None, p) == 0
    # the path mode refuses as before
    assert call(0, p, None) == 0 and call(0, p, p) == 0
    # the shape refusals come before the mode
    assert lib.simulst_ctc_best_alignment(h, p, 8, 4, 1, p, 3, p, p, 5, 0, 1024, 0, 0, None, None, p) == E_SHAPE
    assert b"1023" in lib.simulst_last_error(h)


def test_no_new_entry_point_and_no_descriptor_change():
    from simulst_amd import _lib
    assert len(_lib.SIGNATURES) == abi_pins.N_SIGNATURES
    assert _lib.load().simulst_version() == abi_pins.VERSION == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.LinearDesc) == abi_pins.LINEAR_DESC_BYTES
