"""CPU: simulst_amd/ctc.py -- ctc_collapse against a plain Python loop, ctc_report against g28_ctc_report.npz (recorded from the
reference's calc_recall_precision and blank rate by tests/golden/gen_golden_ctc_report.py)."""
import os

import numpy as np
import pytest
import torch

from ctc_ref import collapse_loop
from simulst_amd.ctc import ctc_collapse, ctc_report

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "g28_ctc_report.npz"))
A, B_, BLANK, PAD = 5, 7, 0, 1

# (path, length): the cases of the issue, padded to one width below
PATHS = {
    "all blank": ([0, 0, 0, 0, 0, 0, 0], 7),
    "leading repeats": ([A, A, A, 0, B_, 0, 0], 7),
    "a _ a": ([A, 0, A, 0, 0, 0, 0], 3),
    "a a _ _ b b a": ([A, A, 0, 0, B_, B_, A], 7),
    "token on the last valid row": ([0, 0, 0, 0, B_, A, A], 5),
    "garbage past the length": ([A, 0, B_, B_, A, 9, 3], 4),
    "a run cut by the length": ([A, B_, B_, B_, B_, 0, 0], 3),
    "length 0": ([A, B_, A, B_, A, B_, A], 0),
    "no blank at all": ([A, B_, A, A, B_, B_, 9], 7),
}


@pytest.mark.parametrize("blank", [0, A])
def test_collapse_equals_the_loop(blank):
    path = torch.tensor([p for p, _ in PATHS.values()])
    lengths = torch.tensor([n for _, n in PATHS.values()])
    for dtype in (torch.int32, torch.int64):
        tokens, n, frames = ctc_collapse(path.to(dtype), lengths, blank, PAD)
        assert tokens.dtype == torch.int64 and frames.dtype == torch.int32 and tokens.shape == frames.shape
        want = [collapse_loop(p, ln, blank) for p, ln in PATHS.values()]
        assert tokens.size(1) == max(len(t) for t, _ in want)
        for b, (name, (toks, frs)) in enumerate(zip(PATHS, want)):
            k = int(n[b])
            assert tokens[b, :k].tolist() == toks and frames[b, :k].tolist() == frs, name
            assert bool((tokens[b, k:] == PAD).all()) and bool((frames[b, k:] == -1).all()), name
    if blank == 0:                                               # the cases say what they say
        got = {name: tokens[b, :int(n[b])].tolist() for b, name in enumerate(PATHS)}
        assert got["all blank"] == [] and got["a _ a"] == [A, A] and got["a a _ _ b b a"] == [A, B_, A] and got["length 0"] == []
        assert got["token on the last valid row"] == [B_] and got["garbage past the length"] == [A, B_]


def test_collapse_of_nothing():
    tokens, n, frames = ctc_collapse(torch.zeros(0, 5, dtype=torch.int32), torch.zeros(0, dtype=torch.int64), 0, 1)
    assert tokens.shape == (0, 0) and n.shape == (0,) and frames.shape == (0, 0)
    tokens, n, frames = ctc_collapse(torch.zeros(3, 0, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), 0, 1)
    assert tokens.shape == (3, 0) and n.tolist() == [0, 0, 0]


def test_report_equals_the_reference():
    for ci in range(int(G["n_cases"])):
        path, target = torch.from_numpy(G[f"c{ci}.path"]), torch.from_numpy(G[f"c{ci}.target"])
        blank, pad = (int(v) for v in G[f"c{ci}.blank_pad"])
        assert path.size(0) <= 6 and path.size(1) <= 12
        r = ctc_report(path, None, target, blank, pad)
        got = np.array([float(r["recall"]), float(r["precision"]), float(r["blank_rate"])])
        assert np.array_equal(got, G[f"c{ci}.out"]), (ci, got, G[f"c{ci}.out"])
        # int32 paths (what the kernel writes) report the same
        r32 = ctc_report(path.to(torch.int32), None, target, blank, pad)
        assert all(float(r32[k]) == float(r[k]) for k in r)


def test_report_counts_rows_past_the_length_as_blank():
    path, target = torch.from_numpy(G["c0.path"]), torch.from_numpy(G["c0.target"])
    lengths = torch.tensor([12, 7, 0, 3])
    masked = path.clone()
    masked[torch.arange(12).unsqueeze(0) >= lengths.unsqueeze(1)] = 0
    a, b = ctc_report(path, lengths, target, 0, 1), ctc_report(masked, None, target, 0, 1)
    assert all(float(a[k]) == float(b[k]) for k in a)
    full = ctc_report(path, torch.full((4,), 12), target, 0, 1)
    ref = ctc_report(path, None, target, 0, 1)
    assert all(float(full[k]) == float(ref[k]) for k in ref)
