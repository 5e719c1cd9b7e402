"""CPU-side checks of the beam-search entry points (csrc/beam.hip): declared, exported and bound, and bad arguments are refused
before anything reaches the device."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"simulst_beam_topk": 12, "simulst_beam_select": 24, "simulst_beam_reorder": 9, "simulst_beam_backtrack": 19}


def test_declared_exported_and_bound():
    from simulst_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "simulst_hip.h")).read(), flags=re.S)
    so = os.path.join(ROOT, "simulst_amd", "libsimulst_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = _lib.load()
    for name, n_args in NAMES.items():
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == n_args, name
        assert name in exported, name
        assert hasattr(lib, name), name


@pytest.fixture
def handle():
    from simulst_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.simulst_create(ctypes.byref(h), None) == 0
    yield lib, h
    assert lib.simulst_destroy(h) == 0


@pytest.fixture
def host_buf():
    """host memory for every pointer argument: never dereferenced by a refused call"""
    buf = (ctypes.c_int64 * 4096)()
    return buf, ctypes.addressof(buf)


def _topk(lib, h, p, *, R=8, V=64, beam=4, step=0, null=None):
    a = {k: (None if k == null else p) for k in ("logits", "max_len", "lp", "tok")}
    return lib.simulst_beam_topk(h, a["logits"], R, V, beam, step, a["max_len"], None, 1, 2, a["lp"], a["tok"])


SELECT_PTRS = ("cand_lp", "cand_tok", "max_len", "cum", "next_tok", "reorder", "bp_parent", "bp_token", "bp_cum", "fin_step", "fin_row",
               "fin_score", "fin_raw", "fin_count", "finished", "result")


def _select(lib, h, p, *, Bs=2, beam=4, V=64, step=0, L=10, lenpen=1.0, null=None):
    a = {k: (None if k == null else p) for k in SELECT_PTRS}
    return lib.simulst_beam_select(h, a["cand_lp"], a["cand_tok"], Bs, beam, V, step, a["max_len"], L, lenpen, 2, a["cum"],
                                   a["next_tok"], a["reorder"], a["bp_parent"], a["bp_token"], a["bp_cum"], a["fin_step"], a["fin_row"],
                                   a["fin_score"], a["fin_raw"], a["fin_count"], a["finished"], a["result"])


BT_PTRS = ("bp_parent", "bp_token", "bp_cum", "fin_step", "fin_row", "fin_score", "fin_raw", "fin_count", "tokens", "lengths", "scores",
           "pos")


def _backtrack(lib, h, p, *, Bs=2, beam=4, nbest=2, L=10, null=None):
    a = {k: (None if k == null else p) for k in BT_PTRS}
    return lib.simulst_beam_backtrack(h, Bs, beam, nbest, L, a["bp_parent"], a["bp_token"], a["bp_cum"], a["fin_step"], a["fin_row"],
                                      a["fin_score"], a["fin_raw"], a["fin_count"], 1, 2, a["tokens"], a["lengths"], a["scores"],
                                      a["pos"])


def test_topk_refuses_bad_arguments(handle, host_buf):
    lib, h = handle
    _, p = host_buf
    assert lib.simulst_beam_topk(None, p, 8, 64, 4, 0, p, None, 1, 2, p, p) == -1
    for null in ("logits", "max_len", "lp", "tok"):
        assert _topk(lib, h, p, null=null) == -1, null
        assert b"null pointer" in lib.simulst_last_error(h)
    for beam in (0, 17):
        assert _topk(lib, h, p, beam=beam, R=beam * 2 or 2) == -2 and b"beam" in lib.simulst_last_error(h)
    assert _topk(lib, h, p, beam=4, V=8) == -2 and b"V - 1" in lib.simulst_last_error(h)      # 2 beam >= V
    assert _topk(lib, h, p, R=6, beam=4) == -2                                                 # rows not a multiple of beam
    assert _topk(lib, h, p, step=-1) == -2


def test_select_refuses_bad_arguments(handle, host_buf):
    lib, h = handle
    _, p = host_buf
    for null in SELECT_PTRS:
        assert _select(lib, h, p, null=null) == -1, null
        assert b"null pointer" in lib.simulst_last_error(h)
    for beam in (0, 17):
        assert _select(lib, h, p, beam=beam) == -2 and b"beam" in lib.simulst_last_error(h)
    assert _select(lib, h, p, beam=4, V=8) == -2
    assert _select(lib, h, p, Bs=0) == -2
    assert _select(lib, h, p, step=10, L=10) == -2 and b"step" in lib.simulst_last_error(h)
    assert _select(lib, h, p, lenpen=float("nan")) == -2


def test_reorder_refuses_bad_arguments(handle, host_buf):
    from simulst_amd import _lib
    lib, h = handle
    _, p = host_buf
    d = _lib.DecoderDesc()
    d.B, d.D, d.H, d.n_layers, d.cap, d.dtype = 8, 256, 4, 2, 32, _lib.BF16
    src, dst = (_lib.DecLayer * 2)(), (_lib.DecLayer * 2)()
    for L in list(src) + list(dst):
        L.k_cache = L.v_cache = L.head_step = p

    def call(beam=4, n_prev=5, desc=d, reorder=p, result=p, s=src, t=dst):
        return lib.simulst_beam_reorder(h, None if desc is None else ctypes.byref(desc), s, t, reorder, None, beam, n_prev, result)

    assert lib.simulst_beam_reorder(None, ctypes.byref(d), src, dst, p, None, 4, 5, p) == -1
    assert call(desc=None) == -1 and call(s=None) == -1 and call(t=None) == -1
    assert call(reorder=None) == -1 and call(result=None) == -1
    assert call(beam=0) == -2 and call(beam=17) == -2
    assert call(beam=3) == -2                                     # B = 8 rows: not a multiple of 3
    assert call(n_prev=33) == -2 and call(n_prev=-1) == -2
    dst[1].head_step = None
    assert call() == -1 and b"head_step" in lib.simulst_last_error(h)
    dst[1].head_step = p
    src[0].head_read = p                                          # head_read in one set only
    assert call() == -2
    src[0].head_read = None
    d.dtype = 7
    assert call() == -3
    d.dtype = _lib.BF16
    d.H = 3
    assert call() == -2                                           # head_dim not a multiple of 8


def test_backtrack_refuses_bad_arguments(handle, host_buf):
    lib, h = handle
    _, p = host_buf
    for null in BT_PTRS:
        assert _backtrack(lib, h, p, null=null) == -1, null
        assert b"null pointer" in lib.simulst_last_error(h)
    assert _backtrack(lib, h, p, beam=0, nbest=1) == -2
    assert _backtrack(lib, h, p, beam=17, nbest=1) == -2
    assert _backtrack(lib, h, p, beam=4, nbest=5) == -2 and b"nbest" in lib.simulst_last_error(h)
    assert _backtrack(lib, h, p, nbest=0) == -2
    assert _backtrack(lib, h, p, L=0) == -2


def test_python_surface_refuses_bad_arguments():
    from simulst_amd.beam import check_args
    check_args(16, 16, 33)
    for beam, nbest, V in ((0, 1, 64), (17, 1, 64), (4, 5, 64), (4, 0, 64), (4, 1, 8)):
        with pytest.raises(ValueError):
            check_args(beam, nbest, V)
