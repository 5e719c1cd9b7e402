"""CPU-side checks of the transducer's scoring path: the two entry points simulst_joiner_lattice / simulst_rnnt_forward are declared,
exported, bound and refuse bad arguments before any pointer is looked at (every pointer below is host memory or null); the fp64
restatement tests/rnnt_ref.py against brute-force path enumeration, a closed form, and fixture g27 (the reference's own
TransducerDecoder.forward without an incremental state)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import rnnt_ref as rr
import transducer_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G25 = os.path.join(ROOT, "tests", "golden", "g25_transducer.npz")
G27 = os.path.join(ROOT, "tests", "golden", "g27_transducer_lattice.npz")
NAMES = ("simulst_joiner_lattice", "simulst_rnnt_forward")
E_NULL, E_SHAPE, E_ARG = -1, -2, -4


def test_declared_exported_and_bound():
    from simulst_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "simulst_hip.h")).read(), flags=re.S)
    so = os.path.join(ROOT, "simulst_amd", "libsimulst_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), n
        assert re.search(r"\b" + n + r"$", exported, flags=re.M), n
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    from simulst_amd.ops import Ops
    assert callable(Ops.joiner_lattice) and callable(Ops.rnnt_forward)
    assert lib.simulst_version() == _lib.ABI_VERSION          # adding symbols does not move the ABI version


@pytest.fixture
def handle():
    from simulst_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.simulst_create(ctypes.byref(h), None) == 0
    yield lib, h
    assert lib.simulst_destroy(h) == 0


def test_refusals_on_host_buffers(handle):
    lib, h = handle
    buf = (ctypes.c_int64 * 4096)()
    p = ctypes.addressof(buf)

    def lattice(B=2, S=4, U1=3, D=32, V=64, blank=0, n_split=1, dtype=0, ptrs=None):
        return lib.simulst_joiner_lattice(h, *(ptrs or [p] * 9), B, S, U1, D, V, blank, n_split, dtype)

    def forward(B=2, S=4, U1=3, ptrs=None):
        return lib.simulst_rnnt_forward(h, *(ptrs or [p] * 8), B, S, U1)

    assert lattice(D=48) == E_ARG and b"D % 32" in lib.simulst_last_error(h)
    assert lattice(D=0) == E_ARG
    assert lattice(V=3) == E_ARG and b"V >= 4" in lib.simulst_last_error(h)
    assert lattice(S=0) == E_ARG and b"S' >= 1" in lib.simulst_last_error(h)
    assert lattice(U1=0) == E_ARG and b"U1 >= 1" in lib.simulst_last_error(h)
    assert lattice(blank=64) == E_ARG and lattice(blank=-1) == E_ARG
    assert lattice(n_split=0) == E_ARG and lattice(n_split=65) == E_ARG
    assert lattice(dtype=2) == E_ARG and b"dtype" in lib.simulst_last_error(h)
    assert lattice(dtype=-1) == E_ARG
    assert lattice(D=48, ptrs=[None] * 9) == E_ARG            # the argument check comes before the pointers
    assert lattice(D=8192) == E_SHAPE                         # the row panel does not fit in LDS: refused
    assert lattice(B=0) == 0                                  # an empty batch is no error and launches nothing
    for i in range(9):                                        # valid arguments with a null pointer: E_NULL, before any launch
        assert lattice(ptrs=[None if j == i else p for j in range(9)]) == E_NULL, i
    assert lib.simulst_joiner_lattice(None, *[p] * 9, 2, 4, 3, 32, 64, 0, 1, 0) == E_NULL

    assert forward(S=0) == E_ARG and b"S' >= 1" in lib.simulst_last_error(h)
    assert forward(U1=0) == E_ARG and b"U1 >= 1" in lib.simulst_last_error(h)
    assert forward(B=-1) == E_ARG
    assert forward(S=0, ptrs=[None] * 8) == E_ARG
    assert forward(U1=4097) == E_SHAPE and b"diagonal" in lib.simulst_last_error(h)
    assert forward(B=0) == 0
    assert forward(B=0, ptrs=[p] * 5 + [None] * 3) == 0       # without the best alignment
    for i in range(5):
        assert forward(ptrs=[None if j == i else p for j in range(8)]) == E_NULL, i
    assert forward(ptrs=[p] * 5 + [p, None, p]) == E_NULL     # best_ll / emit / backptr come together
    assert lib.simulst_rnnt_forward(None, *[p] * 8, 2, 4, 3) == E_NULL


# ------------------------------------------------------------------------------------------------------------ tests/rnnt_ref.py
@pytest.mark.parametrize("S,n", [(S, n) for S in range(1, 5) for n in range(0, 4)])
def test_forward_recursion_equals_path_enumeration(S, n):
    lb, lt = rr.random_lattice(1, S, n + 1, seed=31 * S + n)
    ll, _ = rr.forward_ll(lb[0], lt[0], S, n)
    brute, brute_best = rr.enumerate_ll(lb[0], lt[0], S, n)
    assert abs(ll - brute) < 1e-12
    best, emit = rr.best_alignment(lb[0], lt[0], S, n)
    assert abs(best - brute_best) < 1e-12 and abs(rr.path_score(lb[0], lt[0], S, n, emit) - best) < 1e-12
    assert emit == sorted(emit) and all(0 <= e < S for e in emit) and best <= ll + 1e-12


@pytest.mark.parametrize("S,n", [(1, 1), (2, 3), (17, 33), (65, 130)])
def test_forward_recursion_closed_form(S, n):
    half = torch.full((S, n + 1), math.log(0.5), dtype=torch.float64)
    ll, _ = rr.forward_ll(half, half, S, n)
    assert abs(ll - rr.closed_form_ll(S, n)) < 1e-9 * max(1.0, abs(ll))


def test_lattice_inputs_follow_the_reference():
    prev = torch.tensor([[2, 7, 8, 9], [2, 5, 1, 1], [2, 1, 1, 1]])
    inp, labels, n = rr.lattice_inputs(prev)
    assert inp.tolist() == [[0, 7, 8, 9, 2], [0, 5, 2, 1, 1], [0, 2, 1, 1, 1]]
    assert labels.tolist() == [[7, 8, 9, 2, 1], [5, 2, 1, 1, 1], [2, 1, 1, 1, 1]] and n.tolist() == [4, 2, 1]


def _restated_lattice(g25, prev):
    w = {k[2:]: torch.from_numpy(g25[k]) for k in g25.files if k.startswith("w:")}
    ref = tr.TransducerRef(w, heads=int(g25["args.decoder_attention_heads"]), downsample=int(g25["args.downsample"]))
    inp, labels, n = rr.lattice_inputs(prev)
    logits, _, src_len = rr.model_lattice_logits(ref, torch.from_numpy(g25["enc_out"]).transpose(0, 1), g25["enc_len"], inp)
    return logits, src_len, n


def test_restatement_matches_g27():
    g25, g27 = np.load(G25), np.load(G27)
    logits, src_len, n = _restated_lattice(g25, torch.from_numpy(g27["prev_output_tokens"]))
    want = torch.from_numpy(g27["lattice_logits"]).double()
    assert tuple(want.shape) == (4, 10, 7, 64) == tuple(logits.shape)
    assert src_len.tolist() == g27["pooled_len"].tolist() and n.tolist() == g27["target_lengths"].tolist() == [6, 4, 1, 3]
    valid, _ = rr.valid_cells(src_len, n, 10, 7)
    assert int(valid.sum()) == 10 * 7 + 10 * 5 + 6 * 2 + 1 * 4
    assert float((logits - want)[valid].abs().max()) < 1e-5


def test_restatement_matches_the_live_reference(tmp_path):
    """the generator run again in a process of its own, where the reference is present (skipped elsewhere: g27 holds its output)"""
    import sys
    gen = os.path.join(ROOT, "tests", "golden", "gen_golden_transducer_lattice.py")
    ref_dir = re.search(r'^REF = "(.*)"$', open(os.path.join(ROOT, "tests", "golden", "gen_golden.py")).read(), flags=re.M).group(1)
    if not os.path.isdir(ref_dir):
        pytest.skip("the reference implementation is not on this machine")
    out = str(tmp_path / "live.npz")
    subprocess.run([sys.executable, gen, "--out", out], check=True, capture_output=True)
    live, g27 = np.load(out), np.load(G27)
    assert live["prev_output_tokens"].tolist() == g27["prev_output_tokens"].tolist()
    logits, src_len, n = _restated_lattice(np.load(G25), torch.from_numpy(live["prev_output_tokens"]))
    assert src_len.tolist() == live["pooled_len"].tolist()
    valid, _ = rr.valid_cells(src_len, n, logits.shape[1], logits.shape[2])
    assert float((logits - torch.from_numpy(live["lattice_logits"]).double())[valid].abs().max()) < 1e-5
