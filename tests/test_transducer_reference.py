"""The fp64 restatement of the transducer's inference path (tests/transducer_ref.py) against fixture g25, the reference's own
TransducerDecoder: pooled states and teacher-forced step logits within 1e-5, emit positions and greedy tokens equal."""
import os

import numpy as np
import pytest
import torch

import transducer_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G25 = os.path.join(ROOT, "tests", "golden", "g25_transducer.npz")


@pytest.fixture(scope="module")
def g25():
    g = np.load(G25)
    w = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
    ref = tr.TransducerRef(w, heads=int(g["args.decoder_attention_heads"]), downsample=int(g["args.downsample"]))
    return g, ref


def test_pooling_matches_the_reference(g25):
    g, ref = g25
    y, n = tr.pool(torch.from_numpy(g["enc_out"]).transpose(0, 1), g["enc_len"], int(g["args.downsample"]))
    assert n.tolist() == g["pooled_len"].tolist() == [10, 10, 6, 1]
    assert (y - torch.from_numpy(g["pooled"]).transpose(0, 1)).abs().max() < 1e-5


def test_quirk_of_the_clipped_last_window():
    """T = 11, k = 4, len = 10: the shorter row's last window is also the batch's clipped one -> sum / 3 * 4 / 2 = 4/3 of the mean"""
    x = torch.ones(2, 11, 4)
    y, n = tr.pool(x, [11, 10], 4)
    assert n.tolist() == [3, 3]
    assert torch.allclose(y[0, 2], torch.ones(4, dtype=tr.F64)) and torch.allclose(y[1, 2], torch.full((4,), 4 / 3, dtype=tr.F64))
    # ... and a row's pooled states depend on the batch's T: alone (T = 10) the same row gives the plain mean
    y1, _ = tr.pool(x[1:, :10], [10], 4)
    assert torch.allclose(y1[0, 2], torch.ones(4, dtype=tr.F64))


def test_teacher_forced_steps_match_the_reference(g25):
    g, ref = g25
    ref.set_source(torch.from_numpy(g["enc_out"]).transpose(0, 1), g["enc_len"])
    logits, emits, margins = ref.run_forced(torch.from_numpy(g["forced"]))
    assert (logits - torch.from_numpy(g["step_logits"])).abs().max() < 1e-5
    assert emits.tolist() == g["step_emit"].tolist()
    assert min(min(m) for step in margins for m in step) >= 1e-3          # the fixture's decisions are clear ones


def test_greedy_matches_the_reference(g25):
    g, ref = g25
    ref.set_source(torch.from_numpy(g["enc_out"]).transpose(0, 1), g["enc_len"])
    toks, emits, margins = ref.run_greedy(g["greedy"].shape[1])
    assert toks.tolist() == g["greedy"].tolist()
    assert emits.tolist() == g["greedy_emit"].tolist()
    assert float(margins.min()) >= 1e-3
