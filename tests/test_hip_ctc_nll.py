"""The sum mode of simulst_ctc_best_alignment (out == NULL; ctc_align.ctc_nll, csrc/ctc_align.hip ctc_nll_kernel) on the MI355X: the CTC
negative log-likelihood over random fp32 log-probabilities against torch.nn.functional.ctc_loss(reduction="none") on the CPU in fp64
of the same values.  GPU only.

Bound of row b: (S_b + 1) 2^-22 max(1, max |alpha_ref|) -- the form of tests/rnnt_ref.ll_bound: one rounding of the sum and one of the
log-add per frame; max |alpha_ref| is the largest finite |alpha| of an fp64 recursion over the row (tests/ctc_score_ref.py, held
to F.ctc_loss itself here).  A transcript that does not fit its frames is +inf in both, never NaN."""
import math

import pytest
import torch
import torch.nn.functional as F

import ctc_score_ref as sr
from conftest import load_golden as _load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _reference(lp, tg, il, tl, blank):
    """-> (fp64 F.ctc_loss per row, the bound per row)"""
    ref = F.ctc_loss(lp.double(), tg, il, tl, blank=blank, reduction="none", zero_infinity=False)
    bounds = []
    for b in range(lp.size(1)):
        nll, big = sr.alpha64(lp[:int(il[b]), b].double(), tg[b, :int(tl[b])].tolist(), blank)
        assert (nll == float(ref[b])) if math.isinf(nll) else abs(nll - float(ref[b])) <= 1e-9 * max(1.0, abs(nll))
        bounds.append(sr.nll_bound(int(il[b]), big))
    return ref, torch.tensor(bounds, dtype=torch.float64)


def _lp(S, N, V, seed, scale=3.0):
    return torch.log_softmax(torch.randn(S, N, V, generator=torch.Generator().manual_seed(seed)) * scale, -1)


def _edge_batch():
    """one row per edge: T = 0; T = 1; "aab"; frames exactly L + repeats; one frame fewer (no alignment); one frame with one label;
    one frame with two labels (no alignment)"""
    S, V = 9, 6
    lp = _lp(S, 7, V, 21)
    tg = torch.tensor([[1, 1, 1, 1], [3, 1, 1, 1], [2, 2, 5, 1], [4, 4, 2, 2], [4, 4, 2, 2], [5, 1, 1, 1], [5, 3, 1, 1]])
    tl = torch.tensor([0, 1, 3, 4, 4, 1, 2])
    il = torch.tensor([9, 9, 9, 6, 5, 1, 1])
    return lp, tg, il, tl, 0


def _ragged_batch():
    S, V = 40, 11
    lp = _lp(S, 5, V, 22)
    g = torch.Generator().manual_seed(23)
    tg = torch.randint(1, V, (5, 12), generator=g)
    tg[1, 3] = tg[1, 2]
    tg[4, 1] = tg[4, 0]
    return lp, tg, torch.tensor([40, 17, 3, 29, 8]), torch.tensor([12, 7, 0, 12, 3]), 0


def _long_batch():
    """1023 labels (the limit) over 1100 frames, V = 8: no label equals its neighbour, so the transcript fits"""
    S, V, L = 1100, 8, 1023
    lp = _lp(S, 2, V, 24, scale=1.0)
    g = torch.Generator().manual_seed(25)
    step = torch.randint(1, V - 1, (2, L), generator=g)
    tg = (step.cumsum(1) % (V - 1)) + 1                     # labels 1..7, consecutive ones differ
    assert bool((tg[:, 1:] != tg[:, :-1]).all())
    return lp, tg, torch.tensor([1100, 1023]), torch.tensor([1023, 1023]), 0


def _blank_batch():
    """blank = 4 of 7: labels avoid it"""
    S, V = 25, 7
    lp = _lp(S, 3, V, 26)
    tg = torch.tensor([[0, 1, 1, 6, 5, 5], [6, 0, 6, 0, 2, 3], [3, 3, 3, 3, 3, 3]])
    return lp, tg, torch.tensor([25, 20, 11]), torch.tensor([6, 6, 6]), 4


BATCHES = {"edges": _edge_batch, "ragged": _ragged_batch, "1023 labels": _long_batch, "blank=4": _blank_batch}
_REF = {}


def _get(name):
    if name not in _REF:
        lp, tg, il, tl, blank = BATCHES[name]()
        _REF[name] = (lp, tg, il, tl, blank) + _reference(lp, tg, il, tl, blank)
    return _REF[name]


def _compare(got, ref, bound, what):
    got = got.cpu().double()
    assert not bool(torch.isnan(got).any()), what
    inf = torch.isinf(ref)
    assert torch.equal(torch.isinf(got), inf) and bool((got[inf] > 0).all()), (what, got, ref)
    err = (got - ref)[~inf].abs()
    print(f"{what}: nll {got.tolist()}  |got - fp64| {err.tolist()}  bound {bound[~inf].tolist()}")
    assert bool((err <= bound[~inf]).all()), what


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_sum_against_fp64_ctc_loss(name):
    from simulst_amd.ctc_align import best_alignment, ctc_nll
    lp, tg, il, tl, blank, ref, bound = _get(name)
    if name == "edges":
        assert [math.isinf(float(v)) for v in ref] == [False, False, False, False, True, False, True]
    got = ctc_nll(lp.to(DEV), tg, il, tl, blank=blank)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (lp.size(1),)
    _compare(got, ref, bound, name)
    # the sum contains the best path
    _, best = best_alignment(lp.to(DEV), tg, il, tl, blank=blank, return_nll=True)
    assert bool((got.cpu().double() <= best.cpu().double() + bound).all()), (name, got, best)


def test_strided_log_probabilities():
    """(N, S, V) storage viewed as (S, N, V), and every other column of a 2 V wide matrix: all three strides are honoured"""
    from simulst_amd.ctc_align import ctc_nll
    lp, tg, il, tl, blank, ref, bound = _get("ragged")
    S, N, V = lp.shape
    nsv = lp.transpose(0, 1).contiguous().to(DEV).transpose(0, 1)
    assert nsv.stride() == (V, S * V, 1)
    _compare(ctc_nll(nsv, tg, il, tl, blank=blank), ref, bound, "(N, S, V) storage")
    wide = torch.full((S + 3, N, 2 * V), float("nan"))
    wide[1:1 + S, :, ::2] = lp
    view = wide.to(DEV)[1:1 + S, :, ::2]
    assert view.stride() == (N * 2 * V, 2 * V, 2)
    _compare(ctc_nll(view, tg, il, tl, blank=blank), ref, bound, "column stride 2")
    # a targets matrix wider than the longest transcript, read through its row stride
    wide_t = torch.cat([tg, torch.full((N, 5), 1)], 1)
    _compare(ctc_nll(lp.to(DEV), wide_t, il, tl, blank=blank), ref, bound, "wide targets")


def test_path_mode_is_what_it_was():
    """out != NULL: the states and labels of tests/golden/g16_best_alignment.npz, as tests/test_ctc_align.py compares them -- with and
    without the optional neg_log_likelihood, which there stays -log of the two final Viterbi scores' sum"""
    from simulst_amd.ctc_align import best_alignment
    g = {k: v.numpy() for k, v in _load_golden("g16_best_alignment")[0].items()}
    for c in sorted({k.split(".")[0] for k in g}):
        lp = torch.from_numpy(g[f"{c}.log_prob"]).to(DEV)
        args = (lp, torch.from_numpy(g[f"{c}.targets"]), torch.from_numpy(g[f"{c}.input_lengths"]),
                torch.from_numpy(g[f"{c}.target_lengths"]))
        assert torch.equal(best_alignment(*args).cpu(), torch.from_numpy(g[f"{c}.states"]))
        states, best = best_alignment(*args, return_nll=True)
        assert torch.equal(states.cpu(), torch.from_numpy(g[f"{c}.states"]))
        assert torch.equal(best_alignment(*args, as_labels=True).cpu(), torch.from_numpy(g[f"{c}.labels"]))
        assert not bool(torch.isnan(best).any())
