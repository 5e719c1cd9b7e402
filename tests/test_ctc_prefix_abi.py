"""CPU-side checks of simulst_ctc_prefix_beam (the prefix beam recursion of csrc/ctc_prefix.hip).  Every refusal is made before a
launch (all pointers below are host memory or null), no utterance is no error, simulst_ctc_best_alignment answers for a transcript
alone, and no descriptor changed."""
import ctypes

import pytest

import abi_pins

E_NULL, E_SHAPE = -1, -2


@pytest.fixture
def handle():
    from simulst_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.simulst_create(ctypes.byref(h), None) == 0
    yield lib, h
    assert lib.simulst_destroy(h) == 0


def _desc(p, **kw):
    from simulst_amd._lib import CtcPrefixDesc
    d = CtcPrefixDesc()
    d.cand_ids, d.id_stride_b, d.id_stride_t, d.k, d.pad, d.cap = p.value, 45, 9, 8, 1, 5
    d.lengths, d.p_b, d.p_nb = p.value, p.value, p.value
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_search_mode_refusals_on_host_buffers(handle):
    from simulst_amd import _lib
    lib, h = handle
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def call(d, beam=8, N=2, lp=p, il=p, out=p, S=5, blank=0):
        return lib.simulst_ctc_prefix_beam(h, lp, 18, 9, 1, il, S, N, beam, blank, ctypes.byref(d) if d is not None else None, out)

    err = lambda: lib.simulst_last_error(h)
    # null pointers: the descriptor, what it points to, and the call's own
    for field in ("cand_ids", "lengths", "p_b", "p_nb"):
        assert call(_desc(p, **{field: None})) == E_NULL and field.encode() in err()
    assert call(None) == E_NULL and b": desc" in err()
    assert call(_desc(p), out=None) == E_NULL and b": strings" in err()
    assert call(_desc(p), lp=None) == E_NULL and b"cand_log_probs" in err()
    assert call(_desc(p), il=None) == E_NULL and b"input_lengths" in err()
    # shapes (the function's own name holds "beam": the phrase names the argument)
    assert call(_desc(p), beam=17) == E_SHAPE and b"beam is 1..16" in err()
    assert call(_desc(p), beam=0) == E_SHAPE and b"beam is 1..16" in err()
    assert call(_desc(p), beam=2 ** 31) == E_SHAPE and b"beam is 1..16" in err()          # INT32_MIN
    assert call(_desc(p, k=9)) == E_SHAPE and b"k is" in err()
    assert call(_desc(p, k=-1)) == E_SHAPE and b"k is" in err()
    assert call(_desc(p, cap=0)) == E_SHAPE and b"cap is" in err()
    assert call(_desc(p), S=0) == E_SHAPE and call(_desc(p), blank=-1) == E_SHAPE
    for beam in (1, 8, 16):
        limit = _lib.ctc_prefix_cap(beam)
        assert limit % 4 == 0 and 8 * beam * limit <= _lib.CTC_PREFIX_STRING_BYTES < 8 * beam * (limit + 4)
        assert call(_desc(p, cap=limit + 1), beam=beam, N=0) == E_SHAPE and b"cap is" in err()
        assert call(_desc(p, cap=limit), beam=beam, N=0) == 0
    assert _lib.ctc_prefix_cap(16) == 1104 >= 1024
    # the refusals hold with no utterance too; a valid call with none launches nothing
    assert call(None, N=0) == E_NULL and call(_desc(p), beam=17, N=0) == E_SHAPE
    assert call(_desc(p), N=0) == 0 and call(_desc(p, k=0), beam=1, N=0) == 0 and call(_desc(p), N=-3) == 0


def test_modes_with_a_transcript_answer_as_before(handle):
    lib, h = handle
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def call(N, out, nll, mtl=3, targets=p, tl=p):
        return lib.simulst_ctc_best_alignment(h, p, 8, 4, 1, targets, 3, p, tl, 5, N, mtl, 0, 0, None, out, nll)

    assert call(2, None, None) == E_NULL and b"neg_log_likelihood" in lib.simulst_last_error(h)
    assert call(0, None, p) == 0 and call(0, p, None) == 0 and call(0, p, p) == 0
    assert call(0, None, p, mtl=0) == 0
    assert call(0, None, p, mtl=1024) == E_SHAPE and b"1023" in lib.simulst_last_error(h)
    assert call(0, p, p, targets=None) == E_NULL and b"targets" in lib.simulst_last_error(h)
    assert call(0, p, p, tl=None) == E_NULL and b"target_lengths" in lib.simulst_last_error(h)
    # no other operation hides behind the arguments: a negative max_target_length is a shape, NULL log_probs a null pointer
    for mtl in (-1, -8, -2 ** 31):
        assert call(0, p, p, mtl=mtl) == E_SHAPE and b"shape" in lib.simulst_last_error(h)
        assert call(0, p, p, mtl=mtl, targets=None) == E_NULL and b"targets" in lib.simulst_last_error(h)
    assert lib.simulst_ctc_best_alignment(h, None, 8, 4, 1, p, 3, p, p, 5, 2, 3, 0, 0, p, p, None) == E_NULL
    assert b"log_probs" in lib.simulst_last_error(h)


def test_descriptor_layout_and_pinned_counts():
    from simulst_amd import _lib
    d = _lib.CtcPrefixDesc
    assert ctypes.sizeof(d) == abi_pins.CTC_PREFIX_DESC_BYTES
    assert [getattr(d, n).offset for n in ("cand_ids", "id_stride_b", "id_stride_t", "k", "pad", "cap", "lengths", "p_b", "p_nb")] == \
        [0, 8, 16, 24, 28, 32, 40, 48, 56]
    assert len(_lib.SIGNATURES) == abi_pins.N_SIGNATURES
    assert _lib.load().simulst_version() == abi_pins.VERSION == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.LinearDesc) == abi_pins.LINEAR_DESC_BYTES


def test_python_surface_takes_ops_and_composed():
    """CPU tensors run the torch form whatever `composed` says; the state given is not written"""
    import torch

    import ctc_beam_ref as br
    import ctc_prefix_ref as pr
    from simulst_amd import ctc
    c = pr.case("reentry_V4_beam3_seed71")
    st0 = ctc.ctc_prefix_beam_init(1, c["beam"], "cpu")
    keep = [x.clone() for x in st0]
    a = ctc.ctc_prefix_beam_advance(c["ids"], c["lp"], torch.tensor([c["T"]]), st0, ops=None, composed=False)
    b = ctc.ctc_prefix_beam_advance(c["ids"], c["lp"], torch.tensor([c["T"]]), st0, composed=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(torch.equal(x, y) for x, y in zip(st0, keep))
    hyps, _ = c["ref"][0]
    n = int(a[1][0, 0])
    assert tuple(a[0][0, 0, :n].tolist()) == hyps[0][0]
    assert abs(br.lae(float(a[2][0, 0]), float(a[3][0, 0])) - hyps[0][1]) <= br.beam_bound(c["T"], hyps[0][1])
    import inspect
    assert "composed" in inspect.signature(ctc.ctc_prefix_beam_search).parameters
