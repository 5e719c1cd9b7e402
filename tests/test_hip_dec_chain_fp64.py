"""The decoder layer-chain launches (csrc/dec_chain.hip: projection chain and its kk form, feed-forward chain, slab sum + QKV, slab sum +
vocabulary pick) against the float64 stages of tests/dec_chain_ref.py over the case table of tests/dec_chain_cases.py.

Stage-wise.  Every visible stage of a launch is compared with the float64 stage evaluated on the kernel's OWN visible input of that stage
(q against the x the launch wrote, a slab against the x_mid it wrote, ...), so a bound never has to cover an earlier stage's rounding:
  x, x_mid        |got - ref| <= (K + 3) 2^-23 S + half a bf16 spacing; the rows of exact operands bit for bit
  q, q2, qkv      flip term + (K + 3) 2^-23 S + half a bf16 spacing;  the kk form 1.13 (flip term + (K + 3) 2^-23 S) + 7.1e-7 + half a spacing
  slabs (fp32)    flip term of the GELU outputs + (256 + 3) 2^-23 sum |W2||h|
  slab sum        (n + 3) 2^-23 T + half a bf16 spacing; exact rows bit for bit
  pairs           column in its range and not skipped; |val - L[col]| <= bound[col]; no admissible column c with L[c] - bound[c] >
                  L[col] + bound[col]; of two columns with duplicated weight rows only the lowest is ever picked; the fold of the
                  kernel's pairs meets the same conditions over the whole row
All bounds are derived in the docstring of tests/dec_chain_ref.py, none is measured; tests/test_dec_chain_ref_cpu.py shows that they
are not vacuous and that they see every mutant.  The hand-off form of the feed-forward chain (x_mid == NULL) does not show x'; its slabs
and its x must equal the two-launch form's bit for bit (three times).

Guards.  Every output buffer (x, q, q2, qkv, x_mid, the slabs, pairs, sem) sits between 16 guard rows of a NaN bit pattern nobody
computes and is prefilled with it: afterwards the guards are untouched, every live element is finite (so exactly the live rows were
written), sem is zero, and the inputs the header says are left alone (ctx; x in the x_mid form; x_mid and the slabs in the two closing
launches) are unchanged bit for bit.  The slabs are one [splits][B][256] buffer: a write to row >= B of slab sp would land in slab sp + 1
and show as a value error there.

The module prints the worst |got - ref| / bound per (entry point, stage, row class); DESIGN.md records them.
"""
import numpy as np
import pytest
import torch

import dec_chain_cases as C
import dec_chain_ref as R

pytestmark = pytest.mark.gpu

G = 16                                 # guard rows on either side
SENT16, SENT32 = 0x7FB7, 0x7FB7C3A5    # NaN bit patterns nobody computes


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


@pytest.fixture(scope="module")
def worst():
    """worst |got - ref| / bound per (entry point, stage, row class)"""
    w = {}
    yield w
    for k, (r, name) in sorted(w.items()):
        print(f"\ndecoder chains, worst |got - ref| / bound: {k[0]}, {k[1]}, {k[2]} rows: {r:.3f} ({name})")


class Guarded:
    """a [rows, ...] device buffer between G guard rows, all of it prefilled with the sentinel (or, live rows, with `init`)"""

    def __init__(self, shape, dtype, init=None, zero=False):
        self.dtype, self.rows = dtype, shape[0]
        idt, self.sent = (torch.int16, SENT16) if dtype == torch.bfloat16 else (torch.int32, SENT32)
        self.bits = torch.full((shape[0] + 2 * G,) + tuple(shape[1:]), self.sent, dtype=idt, device="cuda")
        self.t = self.bits.view(dtype)[G:G + shape[0]]
        if zero:
            self.t.zero_()
        if init is not None:
            self.t.copy_(init)

    def check(self, what):
        assert bool((self.bits[:G] == self.sent).all()) and bool((self.bits[G + self.rows:] == self.sent).all()), f"{what}: a guard row was written"
        if self.dtype != torch.int32:
            assert bool(torch.isfinite(self.t.float()).all()), f"{what}: a live element is not finite (not written, or NaN / Inf)"

    def f64(self):
        return self.t.float().cpu().double().numpy()


def _bf(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).cuda().contiguous()


def _f(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).float().cuda().contiguous()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _compare(worst, fails, entry, stage, name, classes, got, val, bound, exact_bits=False, axis=0):
    """got / val / bound [..rows..]: per row class, bits (exact rows of a bf16 sum) or the worst |got - ref| / bound"""
    for cls, rows in C.class_rows(classes).items():
        g, v, b = (np.take(a, rows, axis=axis) for a in (got, val, bound))
        if exact_bits and cls in C.EXACT_CLASSES:
            ref = R.round_once(v)
            assert np.array_equal(ref, v), "an exact row whose sum is not a bf16 number"
            same = np.array_equal(g, ref) and np.array_equal(np.signbit(g), np.signbit(ref))
            print(f"{name}: {entry}, {stage}, {cls} rows: {'bit for bit' if same else 'DIFFERENT BITS'}")
            if not same:
                fails.append((name, entry, stage, cls, "bits", int((g != ref).sum())))
            continue
        ratio = float((np.abs(g - v) / b).max())
        print(f"{name}: {entry}, {stage}, {cls} rows: max |got - ref| = {float(np.abs(g - v).max()):.3e}, / bound = {ratio:.3f}")
        key = (entry, stage, cls)
        if ratio > worst.get(key, (-1.0, ""))[0]:
            worst[key] = (ratio, name)
        if not ratio <= 1.0:
            fails.append((name, entry, stage, cls, ratio))


# ======================================================================================================================================
@pytest.mark.parametrize("name", [c["name"] for c in C.PROJ_CASES])
def test_projection_chain_vs_fp64(ops, worst, name):
    c = C.BY_NAME[name]
    o = C.proj_operands(c)
    B, kk = c["B"], o["kk"] is not None
    entry = "proj_chain_kk" if kk else "proj_chain"
    pk = lambda W: ops.pack_fragment_major(_bf(W))
    ctx = _bf(o["ctx"])
    ctx0 = ctx.clone()
    x = Guarded((B, 256), torch.bfloat16, init=_bf(o["x"]))
    q = Guarded((B, 256), torch.bfloat16)
    q2 = Guarded((B, 256), torch.bfloat16) if o["Wq2"] is not None else None
    ln = (_f(o["gamma"]), _f(o["beta"]))
    if kk:
        kkd = _bf(o["kk"])
        kk0 = kkd.clone()
        ops.decoder_proj_chain_kk(ctx, x.t, pk(o["Wo"]), _f(o["bo"]), ln, pk(o["Wq"]), _f(o["bq"]), kkd, q=q.t)
    else:
        ops.decoder_proj_chain(ctx, x.t, pk(o["Wo"]), _f(o["bo"]), ln, pk(o["Wq"]), _f(o["bq"]), q=q.t,
                               wq2_fm=pk(o["Wq2"]) if q2 else None, bq2=_f(o["bq2"]), q2=q2.t if q2 else None)
    torch.cuda.synchronize()
    for buf, what in ((x, "x"), (q, "q"), (q2, "q2")):
        if buf is not None:
            buf.check(f"{name}: {what}")
    assert torch.equal(_bits(ctx), _bits(ctx0)) and (not kk or torch.equal(_bits(kkd), _bits(kk0)))
    st = C.proj_stages(o, seen={"x": x.f64()})
    fails = []
    _compare(worst, fails, entry, "x", name, o["classes"], x.f64(), *st["x"], exact_bits=True)
    _compare(worst, fails, entry, "q", name, o["classes"], q.f64(), *st["q"])
    if q2:
        _compare(worst, fails, entry, "q2", name, o["classes"], q2.f64(), *st["q2"])
    assert not fails, fails


@pytest.mark.parametrize("name", [c["name"] for c in C.FFN_CASES])
def test_feed_forward_chain_vs_fp64(ops, worst, name):
    c = C.BY_NAME[name]
    o = C.ffn_operands(c)
    B, F = c["B"], c["F"]
    n = F // 256
    pk = lambda W: ops.pack_fragment_major(_bf(W))
    ctx, x_in = _bf(o["ctx"]), _bf(o["x"])
    ctx0 = ctx.clone()
    ln = (_f(o["gamma"]), _f(o["beta"]))
    args = (pk(o["Wco"]), _f(o["bco"]), ln, pk(o["W1"]), _f(o["b1"]), pk(o["W2"]), _f(o["b2"]))
    # ---- the two-launch form: x' to x_mid, x left alone, the slabs added by the slab-sum launch
    x = Guarded((B, 256), torch.bfloat16, init=x_in)
    x_mid = Guarded((B, 256), torch.bfloat16)
    slabs = Guarded((n * B, 256), torch.float32)
    ops.decoder_ffn_chain(ctx, x.t, *args, partial=slabs.t.view(n, B, 256), x_mid=x_mid.t)
    torch.cuda.synchronize()
    for buf, what in ((x, "x"), (x_mid, "x_mid"), (slabs, "slabs")):
        buf.check(f"{name}: {what}")
    assert torch.equal(_bits(x.t), _bits(x_in)), "x written in the x_mid form"
    assert torch.equal(_bits(ctx), _bits(ctx0))
    x2 = Guarded((B, 256), torch.bfloat16)
    xm0, sl0 = x_mid.t.clone(), slabs.t.clone()
    ops.decoder_slab_sum_qkv(x_mid.t, x2.t, slabs.t.view(n, B, 256), _f(o["b2"]))
    torch.cuda.synchronize()
    for buf, what in ((x2, "x (slab sum)"), (x_mid, "x_mid"), (slabs, "slabs")):
        buf.check(f"{name}: {what}")
    assert torch.equal(_bits(x_mid.t), _bits(xm0)) and torch.equal(_bits(slabs.t), _bits(sl0)), "the slab sum wrote one of its inputs"
    got_slabs = slabs.f64().reshape(n, B, 256)
    st = C.ffn_stages(o, seen={"x_mid": x_mid.f64(), "slabs": got_slabs})
    fails = []
    _compare(worst, fails, "ffn_chain", "x_mid", name, o["classes"], x_mid.f64(), *st["x_mid"], exact_bits=True)
    _compare(worst, fails, "ffn_chain", "slabs", name, o["classes"], got_slabs, *st["slabs"], axis=1)
    _compare(worst, fails, "slab_sum", "x after ffn_chain", name, o["classes"], x2.f64(), *st["x"])
    # ---- the hand-off form: x' is not visible; slabs and x bit for bit the two-launch form's, sem zero on return
    tiles = (B + 15) // 16
    for rep in range(3):
        xh = Guarded((B, 256), torch.bfloat16, init=x_in)
        sh = Guarded((n * B, 256), torch.float32)
        sem = Guarded((tiles,), torch.int32, zero=True)
        ops.decoder_ffn_chain(ctx, xh.t, *args, partial=sh.t.view(n, B, 256), sem=sem.t)
        torch.cuda.synchronize()
        for buf, what in ((xh, "x"), (sh, "slabs"), (sem, "sem")):
            buf.check(f"{name}: hand-off form, repeat {rep}: {what}")
        assert int(sem.t.abs().sum()) == 0, "sem not zero on return"
        assert torch.equal(_bits(sh.t), _bits(slabs.t)), (name, rep, "slabs differ from the two-launch form's")
        assert torch.equal(_bits(xh.t), _bits(x2.t)), (name, rep, "x differs from the two-launch form's")
    assert not fails, fails


@pytest.mark.parametrize("name", [c["name"] for c in C.SUM_CASES])
def test_slab_sum_qkv_vs_fp64(ops, worst, name):
    c = C.BY_NAME[name]
    o = C.sum_operands(c)
    B, n = c["B"], c["n"]
    x_mid, slabs = _bf(o["x_mid"]), _f(o["slabs"])
    xm0, sl0 = x_mid.clone(), slabs.clone()
    x = Guarded((B, 256), torch.bfloat16)
    qkv = Guarded((B, 768), torch.bfloat16) if c["qkv"] else None
    if c["qkv"]:
        ops.decoder_slab_sum_qkv(x_mid, x.t, slabs, _f(o["b2"]), (_f(o["gamma"]), _f(o["beta"])), ops.pack_fragment_major(_bf(o["Wqkv"])),
                                 _f(o["bqkv"]), qkv=qkv.t)
    else:
        ops.decoder_slab_sum_qkv(x_mid, x.t, slabs, _f(o["b2"]))
    torch.cuda.synchronize()
    x.check(f"{name}: x")
    if qkv:
        qkv.check(f"{name}: qkv")
    assert torch.equal(_bits(x_mid), _bits(xm0)) and torch.equal(_bits(slabs), _bits(sl0))
    st = C.sum_stages(o, seen={"x": x.f64()})
    fails = []
    _compare(worst, fails, "slab_sum_qkv", "x", name, o["classes"], x.f64(), *st["x"], exact_bits=True)
    if qkv:
        _compare(worst, fails, "slab_sum_qkv", "qkv", name, o["classes"], qkv.f64(), *st["qkv"])
    assert not fails, fails


@pytest.mark.parametrize("name", [c["name"] for c in C.VOCAB_CASES])
def test_vocabulary_chain_vs_fp64(ops, worst, name):
    c = C.BY_NAME[name]
    o = C.vocab_operands(c)
    B, V, split = c["B"], c["V"], c["split"]
    x_mid, slabs = _bf(o["x_mid"]), _f(o["slabs"])
    xm0, sl0 = x_mid.clone(), slabs.clone()
    x = Guarded((B, 256), torch.bfloat16)
    pairs = Guarded((B, split * 2), torch.float32)
    ops.decoder_vocab_chain(x_mid, x.t, slabs, _f(o["b2"]), (_f(o["gamma"]), _f(o["beta"])), ops.pack_fragment_major(_bf(o["Wout"])), V, split,
                            o["skip_a"], o["skip_b"], row_bias=_f(o["row_bias"]), row_bias_col=c["row_bias_col"] if c["row_bias"] else -1,
                            pairs=pairs.t.view(B, split, 2))
    torch.cuda.synchronize()
    x.check(f"{name}: x")
    pairs.check(f"{name}: pairs")
    assert torch.equal(_bits(x_mid), _bits(xm0)) and torch.equal(_bits(slabs), _bits(sl0))
    pr = pairs.t.view(B, split, 2)
    vals = pr[..., 0].cpu().double().numpy()
    cols = pr[..., 1].contiguous().view(torch.int32).cpu().numpy().astype(np.int64)
    assert np.isfinite(vals).all(), f"{name}: a pair was not written"
    st = C.vocab_stages(o, seen={"x": x.f64()})
    fails = []
    _compare(worst, fails, "vocab_chain", "x", name, o["classes"], x.f64(), *st["x"], exact_bits=True)
    Lb, bound = st["logits"]
    bad, ratio = C.check_pairs(c, o, vals, cols, Lb, bound)
    print(f"{name}: vocab_chain, pairs: worst |val - L[col]| / bound[col] = {ratio:.3f}")
    key = ("vocab_chain", "pair value", "all")
    if ratio > worst.get(key, (-1.0, ""))[0]:
        worst[key] = (ratio, name)
    assert not bad and not fails, (bad, fails)
