"""The column remapping of ctc.ctc_score (ctc.ctc_columns): the recursion is handed a matrix with one column per target POSITION and
column ids in place of labels, and must still compute the transcript's CTC likelihood.  Checked on the CPU in fp64 against a brute-force
sum over all alignments and against F.ctc_loss over the full log-probabilities.  No device."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

import ctc_ref as cr

BLANK, V = 0, 4
A, Bb, Cc = 1, 2, 3
TARGETS = {"a": [A], "aa": [A, A], "ab": [A, Bb], "aba": [A, Bb, A], "aab": [A, A, Bb], "abb": [A, Bb, Bb], "aaa": [A, A, A],
           "abc": [A, Bb, Cc], "": []}


def _brute_force_nll(lp, target):
    """lp [T, V] fp64 log-probabilities: -log of the summed probability of every frame labelling that collapses to target"""
    T = lp.size(0)
    total = 0.0
    for path in itertools.product(range(lp.size(1)), repeat=T):
        toks, _ = cr.collapse_loop(path, T, BLANK)
        if toks == list(target):
            total += math.exp(sum(float(lp[t, c]) for t, c in enumerate(path)))
    return -math.log(total) if total > 0 else float("inf")


def _gathered(lp, target, Lmax):
    """what ctc.ctc_score hands the recursion: the columns of lp at [blank, target..., blank padding] and the column ids"""
    from simulst_amd import ctc
    tgt = torch.full((1, Lmax), 1, dtype=torch.int64)
    tgt[0, :len(target)] = torch.tensor(target, dtype=torch.int64)
    lab = ctc._gather_labels(tgt, torch.tensor([len(target)]), BLANK)
    return lp[:, lab[0].long()], ctc.ctc_columns(tgt)


def test_column_ids():
    from simulst_amd.ctc import ctc_columns
    t = torch.tensor([[5, 5, 7, 7, 7, 5], [1, 2, 3, 4, 5, 6], [9, 9, 9, 9, 9, 9]])
    assert ctc_columns(t).tolist() == [[1, 1, 3, 3, 3, 6], [1, 2, 3, 4, 5, 6], [1, 1, 1, 1, 1, 1]]
    assert ctc_columns(torch.tensor([[4]])).tolist() == [[1]] and tuple(ctc_columns(torch.zeros(2, 0, dtype=torch.int64)).shape) == (2, 0)


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("name", sorted(TARGETS))
def test_remapped_gathered_matrix_gives_the_ctc_likelihood(name, T):
    target = TARGETS[name]
    g = torch.Generator().manual_seed(100 * T + len(name))
    lp = torch.randn(T, V, generator=g, dtype=torch.float64).log_softmax(-1)
    want = _brute_force_nll(lp, target)
    il, tl = torch.tensor([T]), torch.tensor([len(target)])
    full = float(F.ctc_loss(lp.unsqueeze(1), torch.tensor([target + [1] * (3 - len(target))]), il, tl, blank=BLANK, reduction="none"))
    gat, cols = _gathered(lp, target, 3)
    got = float(F.ctc_loss(gat.unsqueeze(1), cols, il, tl, blank=0, reduction="none"))
    feasible = len(target) + sum(a == b for a, b in zip(target, target[1:])) <= T
    if not feasible:
        assert want == full == got == float("inf")
        return
    assert abs(full - want) <= 1e-12 * max(1.0, abs(want))          # the reference agrees with the brute force
    assert abs(got - want) <= 1e-12 * max(1.0, abs(want))
    if name in ("aa", "aab", "abb", "aaa") and T > len(target):
        # a plain 1..L would count the skip across the repeated label: more alignments, a smaller nll
        plain = float(F.ctc_loss(gat.unsqueeze(1), torch.arange(1, 4).unsqueeze(0), il, tl, blank=0, reduction="none"))
        assert plain < want - 1e-9
