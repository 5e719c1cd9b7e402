"""CPU-side checks of simulst_ctc_prefix_score (csrc/ctc_prefix_score.hip).  Every refusal is made before a launch (all pointers
below are host memory or null), no row is no error, simulst_ctc_best_alignment takes a transcript and nothing else, and no existing
descriptor changed."""
import ctypes

import pytest

import abi_pins

E_NULL, E_SHAPE = -1, -2
SCORE_FIELDS = ("blank_lp", "state", "psi", "cand_state", "cand_psi", "cand_lp", "cand_tok", "cand_slot")
COMMIT_FIELDS = ("cand_state", "cand_psi", "cand_tok", "cand_slot", "next_tok", "reorder", "state_out", "psi_out", "last_out", "len_out",
                 "result")


@pytest.fixture
def handle():
    from simulst_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.simulst_create(ctypes.byref(h), None) == 0
    yield lib, h
    assert lib.simulst_destroy(h) == 0


def _desc(p, op=0, **kw):
    from simulst_amd._lib import CtcScoreDesc
    d = CtcScoreDesc()
    d.op, d.G, d.eos, d.pad, d.weight, d.first_only, d.blank_stride_b = op, 2, 2, 1, 0.3, 0, 5
    for n in SCORE_FIELDS + COMMIT_FIELDS + ("finished",):
        setattr(d, n, p.value)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_scoring_mode_refusals_on_host_buffers(handle):
    lib, h = handle
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def call(d, K=4, N=4, lp=p, last=p, tl=p, il=p, S=5, blank=0):
        return lib.simulst_ctc_prefix_score(h, lp, 8, 40, 1, last, il, tl, S, N, K, blank, ctypes.byref(d) if d is not None else None)

    err = lambda: lib.simulst_last_error(h)      # noqa: E731
    # null pointers, by name: the descriptor, what it points to for each op, and the call's own
    assert call(None) == E_NULL and b": desc" in err()
    for field in SCORE_FIELDS:
        assert call(_desc(p, **{field: None})) == E_NULL and field.encode() in err(), field
    for field in COMMIT_FIELDS:
        assert call(_desc(p, op=1, **{field: None})) == E_NULL and field.encode() in err(), field
    assert call(_desc(p, finished=None), N=0) == 0                                  # finished is optional
    assert call(_desc(p), lp=None) == E_NULL and b"cand_log_probs" in err()
    assert call(_desc(p, op=1), lp=None, N=0) == 0                                  # commit reads no log-probabilities
    assert call(_desc(p), last=None) == E_NULL and b"last_labels" in err()
    assert call(_desc(p, op=1), last=None, N=0) == 0                                # ... and no last labels
    assert call(_desc(p), tl=None) == E_NULL and b"prefix_lengths" in err()
    assert call(_desc(p, op=1), tl=None) == E_NULL and b"prefix_lengths" in err()
    assert call(_desc(p), il=None) == E_NULL and b"input_lengths" in err()
    # shapes
    for K in (0, 33, 64, 2 ** 31):                                                  # (INT32_MIN)
        assert call(_desc(p), K=K) == E_SHAPE and b"K is 1..32" in err(), K
    assert call(_desc(p, G=0)) == E_SHAPE and b"G >= 1" in err()
    assert call(_desc(p, G=3), N=4) == E_SHAPE and b"multiple of G" in err()
    assert call(_desc(p), S=0) == E_SHAPE and call(_desc(p), blank=-1) == E_SHAPE
    assert call(_desc(p, op=2)) == E_SHAPE and b"op is 0" in err()
    # the refusals hold with no row too; a valid call with none launches nothing
    assert call(None, N=0) == E_NULL and call(_desc(p), K=33, N=0) == E_SHAPE and call(_desc(p, G=0), N=0) == E_SHAPE
    for K in (1, 32):
        assert call(_desc(p), K=K, N=0) == 0 and call(_desc(p, op=1), K=K, N=-2) == 0


def test_best_alignment_takes_a_transcript_and_nothing_else(handle):
    """what was the scoring call through simulst_ctc_best_alignment (max_target_length = -K, a descriptor as scratch) is a shape error"""
    lib, h = handle
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    d = _desc(p)
    for mtl in (-4, -32, -2 ** 31):
        assert lib.simulst_ctc_best_alignment(h, p, 8, 40, 1, p, 0, p, p, 5, 4, mtl, 0, 0, ctypes.addressof(d), None, p) == E_SHAPE
        assert b"shape" in lib.simulst_last_error(h)
    with_targets = lambda N, out, nll, mtl, lp=p: lib.simulst_ctc_best_alignment(h, lp, 8, 4, 1, p, 3, p, p, 5, N, mtl, 0, 0, None, out, nll)   # noqa: E731
    assert with_targets(0, p, p, 3, lp=None) == E_NULL and b"log_probs" in lib.simulst_last_error(h)
    assert with_targets(2, None, None, 3) == E_NULL and b"neg_log_likelihood" in lib.simulst_last_error(h)
    assert with_targets(0, None, p, 1024) == E_SHAPE and b"1023" in lib.simulst_last_error(h)
    assert with_targets(0, p, p, 3) == 0


def test_descriptor_layout_and_pinned_counts():
    from simulst_amd import _lib
    d = _lib.CtcScoreDesc
    assert ctypes.sizeof(d) == 160
    names = ("op", "G", "eos", "pad", "weight", "first_only", "blank_lp", "blank_stride_b", "state", "psi", "cand_state", "cand_psi",
             "cand_lp", "cand_tok", "cand_slot", "finished", "next_tok", "reorder", "state_out", "psi_out", "last_out", "len_out", "result")
    assert [n for n, _ in d._fields_] == list(names)
    assert [getattr(d, n).offset for n in names] == [0, 4, 8, 12, 16, 20] + list(range(24, 160, 8))
    assert len(_lib.SIGNATURES) == abi_pins.N_SIGNATURES
    assert _lib.load().simulst_version() == abi_pins.VERSION == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.LinearDesc) == abi_pins.LINEAR_DESC_BYTES
    assert ctypes.sizeof(_lib.CtcPrefixDesc) == abi_pins.CTC_PREFIX_DESC_BYTES
