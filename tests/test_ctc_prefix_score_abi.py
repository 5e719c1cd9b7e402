"""CPU-side checks of the scoring mode of simulst_ctc_best_alignment (max_target_length < 0 with targets: csrc/ctc_prefix_score.hip).
Every refusal is made before a launch (all pointers below are host memory or null), no row is no error, the other modes answer as
before, and the mode added no entry point and changed no existing descriptor."""
import ctypes

import pytest

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

    def call(d, K=4, N=4, lp=p, targets=p, tl=p, il=p, S=5, blank=0):
        return lib.simulst_ctc_best_alignment(h, lp, 8, 40, 1, targets, 0, il, tl, S, N, -K, blank, 0,
                                              ctypes.addressof(d) if d is not None else None, None, None)

    err = lambda: lib.simulst_last_error(h)      # noqa: E731
    # null pointers, by name: the descriptor, what it points to for each op, and the call's own
    assert call(None) == E_NULL and b"desc" in err()
    for field in SCORE_FIELDS:
        assert call(_desc(p, **{field: None})) == E_NULL and field.encode() in err(), field
    for field in COMMIT_FIELDS:
        assert call(_desc(p, op=1, **{field: None})) == E_NULL and field.encode() in err(), field
    assert call(_desc(p, finished=None), N=0) == 0                                  # finished is optional
    assert call(_desc(p), lp=None) == E_NULL and b"log_probs" in err()
    assert call(_desc(p, op=1), lp=None, N=0) == 0                                  # commit reads no log-probabilities
    assert call(_desc(p), tl=None) == E_NULL and b"target_lengths" in err()
    assert call(_desc(p), il=None) == E_NULL and b"input_lengths" in err()
    # shapes
    for K in (33, 64, 2 ** 31):                                                     # (INT32_MIN as max_target_length)
        assert call(_desc(p), K=K) == E_SHAPE and b"1..32" in err(), K
    assert call(_desc(p, G=0)) == E_SHAPE and b"G" in err()
    assert call(_desc(p, G=3), N=4) == E_SHAPE and b"multiple of G" in err()
    assert call(_desc(p), S=0) == E_SHAPE and call(_desc(p), blank=-1) == E_SHAPE
    assert call(_desc(p, op=2)) == E_SHAPE and b"op" in err()
    # the refusals hold with no row too; a valid call with none launches nothing
    assert call(None, N=0) == E_NULL and call(_desc(p), K=33, N=0) == E_SHAPE and call(_desc(p, G=0), N=0) == E_SHAPE
    for K in (1, 32):
        assert call(_desc(p), K=K, N=0) == 0 and call(_desc(p, op=1), K=K, N=-2) == 0
    # targets == NULL is the search mode, with its own refusals: this descriptor is not what it reads, but NULL `out` stops it first
    assert call(_desc(p), targets=None) == E_NULL and b"out" in err()


def test_the_other_modes_answer_as_before(handle):
    """two calls of tests/test_ctc_prefix_abi.py, repeated: the search mode (targets NULL) and the modes with a transcript"""
    from simulst_amd._lib import CtcPrefixDesc
    lib, h = handle
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    d = CtcPrefixDesc()
    d.cand_ids, d.id_stride_b, d.id_stride_t, d.k, d.pad, d.cap = p.value, 45, 9, 8, 1, 5
    d.lengths, d.p_b, d.p_nb = p.value, p.value, p.value
    search = lambda beam, N: lib.simulst_ctc_best_alignment(h, p, 18, 9, 1, None, 0, p, None, 5, N, -beam, 0, 0, ctypes.addressof(d), p,   # noqa: E731
                                                            None)
    assert search(17, 2) == E_SHAPE and b"beam" in lib.simulst_last_error(h)
    assert search(8, 0) == 0
    with_targets = lambda N, out, nll, mtl: lib.simulst_ctc_best_alignment(h, p, 8, 4, 1, p, 3, p, p, 5, N, mtl, 0, 0, None, out, nll)   # noqa: E731
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
    assert len(_lib.SIGNATURES) == 81
    assert _lib.load().simulst_version() == 108 == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.LinearDesc) == 152 and ctypes.sizeof(_lib.CtcPrefixDesc) == 64
