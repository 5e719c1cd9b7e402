"""The bf16 encoder against the fp64 oracle at the row counts the bench runs.

At thousands of rows the encoder takes kernels no smaller test reaches: the 256 x 256 subsampler tiles (simulst_linear ->
tile256_ring_kernel), the weight-stationary Q|K|V and out-proj products (wstat_kernel) and, from layer 1 on, the feed-forward
launch that also writes the next layer's LayerNorm, summaries and Q|K|V rows (ffn_pipe_kernel).  Each form of that path, and
the lockstep streaming encoder, is held here to the fp64 oracle with bars derived from a bf16 emulation of the same oracle.

Reference and error model (module-scoped, computed once per case):
  ref -- oracle.emformer.encoder_forward / encoder_infer in fp64, on bf16-rounded weights and fbank (what the kernels get);
  emu -- the same call with bf16 rounding wherever the HIP path stores a bf16 tensor between launches or feeds one to an MFMA
         (bf16_emulation below).  `oracle/` itself is not changed: the context manager swaps module attributes and restores them.

Bars (fixed; statistics over valid frames f < enc_len[b] only; e = per-frame relative error ||y - ref|| / ||ref||):
  (a) mean(e) <= 1.5 x emu's   -- emu's per-frame errors are a sum of ~10^3 independent roundings per frame: their mean over
                                  ~10^4 frames is stable to a few %, so 1.5x leaves room for fp32 accumulation order and the
                                  GELU/rsqrt approximations, and rejects a left context 4 frames short (2.5x emu's mean).
  (b) max(e)  <= 2 x emu's     -- the max of ~10^4 frame errors sits ~1.35x above the mean for emu; 2x is that spread again.
  (c) in every utterance max(e) <= 2.5 x the global median(e)  -- emu's worst utterance is 1.36x; one wrong segment, memory row
                                  or tail tile puts its frames far above it (one segment of keys missing: 7.5x).
  (d) every channel's mean signed error <= 6 x RMS / sqrt(valid frames)  -- unbiased rounding gives a channel mean of
                                  ~RMS / sqrt(frames) (emu: 3.4-4.6x at worst over 256 channels); a systematic offset grows
                                  with the frame count instead of shrinking.
Encoder padding masks and lengths are exact.

If the HIP path misses a bar the factor is not raised: either a kernel rounds where the emulation does not (then the
emulation gains that rounding, citing the kernel line), or it is a bug.
"""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import causal_conv as occ
from oracle import emformer as oem

MEAN_FACTOR, MAX_FACTOR, LOC_FACTOR, BIAS_FACTOR = 1.5, 2.0, 2.5, 6.0

# 40 ragged utterances: the bench's per-copy mix (tests below tile it x 32 to the bench's 1 280); 17 frames and 50 frames are
# both shorter than one 64-frame segment.  Longest 1003 frames -> 251 encoder frames, 16 segments: 40 x 251 = 10 040 rows at the
# second convolution, 40 x (128 + 251) = 15 160 rows per layer.
LENGTHS_40 = [1000, 1003, 999, 640, 311, 17, 50] + [int(v) for v in torch.randint(
    100, 1001, (33,), generator=torch.Generator().manual_seed(40))]
SEED = 999


def _bf16(t):
    """Round to bf16 (through fp32, as the kernels' fp32 accumulators are rounded) and back to t's dtype."""
    return t.float().to(torch.bfloat16).to(t.dtype)


@contextlib.contextmanager
def bf16_emulation(ffn_out_rounded):
    """The oracle with the HIP encoder's bf16 stores.  ffn_out_rounded: the fused feed-forward launches (simulst_emformer_ffn*,
    ffn_pipe.hip:595) round fc2 + bias to bf16 before adding the residual; the two-launch fc2 (gemm.hip:283, gemm_panel.hip) adds
    it in fp32 and rounds once."""
    saved = dict(lin=oem._lin, ln=oem._ln, post=oem._post_attention, pool=oem.avg_pool_ceil,
                 sub=occ.subsampler, pos=occ.conv_pos)
    lin0, ln0, pool0 = oem._lin, oem._ln, oem.avg_pool_ceil

    def lin(w, name, x):
        # A operand of every projection is a bf16 buffer: Z (Q|K|V input: normalised rows and the memory rows Zn that the
        # out-proj's tanh epilogue stores), CTX (out-proj input), the FFN LayerNorm output and the fc1 + GELU hidden Hf
        y = lin0(w, name, _bf16(x))
        if name.endswith(".emb_to_query") or name.endswith(".emb_to_key_value"):
            y = _bf16(y)                          # QKV
        return y                                  # out-proj, fc1, fc2: rounded after their epilogues (post_attention)

    def ln(w, name, x):
        return _bf16(ln0(w, name, x))             # Z (pre-attention LN), Y / the fc1 prologue's MFMA operand, the final LN output

    def pool(x, seg):
        # mems0 (simulst_segment_mean) and the summary rows of Z.  The kernels average the fp32 normalised rows
        # (rowops.hip emformer_prenorm_kernel, ffn_pipe.hip pass 4); here the rounded ones: below a tenth of an ulp
        return _bf16(pool0(x, seg))

    def post_attention(w, p, rc_output, utterance, right_context):
        x = _bf16(rc_output + torch.cat([right_context, utterance]))     # X1: out-proj + bias + residual, one rounding
        h = oem._ln(w, p + ".pos_ff.0", x)
        h = oem._lin(w, p + ".pos_ff.4", F.gelu(oem._lin(w, p + ".pos_ff.1", h)))
        if ffn_out_rounded:
            h = _bf16(h)                          # ffn_pipe.hip:595: fc2 + bias staged as bf16 before the residual add
        x = _bf16(h + x)                          # X: the layer output (residual stream)
        R = right_context.size(0)
        return x[R:], x[:R]

    def subsampler(w, prefix, src_tokens, src_lengths, states=None):
        # occ.subsampler with its GLU outputs rounded: the first convolution's output and the second's (x sqrt(D) in the
        # kernel's epilogue, a power of two: the same rounding)
        n_layers = len([k for k in w if k.startswith(prefix + ".conv_layers.") and k.endswith(".weight")])
        x = src_tokens.transpose(1, 2).contiguous()
        if states is not None:
            prev_len = states[0]["prev_feat"].size(2) if "prev_feat" in states[0] else 0
            x = x[..., prev_len:]
            src_lengths = (src_lengths - prev_len).clamp(min=0)
        ks = []
        for i in range(n_layers):
            wt = w[f"{prefix}.conv_layers.{i}.weight"]
            ks.append(wt.size(2))
            x = occ.causal_conv1d(x, wt, w[f"{prefix}.conv_layers.{i}.bias"], stride=2,
                                  state=None if states is None else states[i])
            x = _bf16(F.glu(x, dim=1))
        return x.transpose(1, 2).transpose(0, 1).contiguous(), occ.subsampler_out_lens(src_lengths, ks)

    def conv_pos(w, prefix, x, groups, state=None):
        # EncoderWeights.pos_w: the folded weight_norm weight is stored in bf16
        wt = _bf16(occ.weight_norm_weight(w[prefix + ".conv.weight_g"], w[prefix + ".conv.weight_v"]))
        y = F.gelu(occ.causal_conv1d(x, wt, w[prefix + ".conv.bias"], stride=1, groups=groups, state=state))
        # the conv-pos kernel stores x + GELU(conv(x)) once; the caller adds x back (exact in fp64)
        return _bf16(x + y) - x

    oem._lin, oem._ln, oem._post_attention, oem.avg_pool_ceil = lin, ln, post_attention, pool
    occ.subsampler, occ.conv_pos = subsampler, conv_pos
    try:
        yield
    finally:
        oem._lin, oem._ln, oem._post_attention, oem.avg_pool_ceil = saved["lin"], saved["ln"], saved["post"], saved["pool"]
        occ.subsampler, occ.conv_pos = saved["sub"], saved["pos"]


# ------------------------------------------------------------------ bars
def bar_stats(y, ref, lengths):
    """y, ref [B, T, D] (any float dtype / device), lengths [B]: the statistics the bars read, over valid frames only."""
    y, ref = y.double(), ref.double().to(y.device)
    lengths = [int(v) for v in lengths]
    err = y - ref
    e = err.norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-30)                  # [B, T]
    valid = torch.arange(y.size(1), device=y.device).unsqueeze(0) < torch.tensor(lengths, device=y.device).unsqueeze(1)
    ev = e[valid]
    ds = err[valid]                                                           # [frames, D]
    n = ds.size(0)
    rms = float(ds.pow(2).mean().sqrt())
    med = float(ev.median())
    utt_max = [float(e[b, :L].max()) for b, L in enumerate(lengths) if L > 0]
    return dict(mean=float(ev.mean()), max=float(ev.max()), median=med, frames=n, rms=rms,
                loc=max(utt_max) / med, worst_utt=int(torch.tensor(utt_max).argmax()),
                bias=float(ds.mean(0).abs().max()) / (rms / math.sqrt(n)))


def bar_ratios(got, emu):
    """Each bar's measured value over its limit (<= 1 passes)."""
    return dict(mean=got["mean"] / (MEAN_FACTOR * emu["mean"]), max=got["max"] / (MAX_FACTOR * emu["max"]),
                loc=got["loc"] / LOC_FACTOR, bias=got["bias"] / BIAS_FACTOR)


def _fmt(s):
    return f"mean {s['mean']:.3e} max {s['max']:.3e} loc {s['loc']:.2f} bias {s['bias']:.2f}"


def assert_bars(got, emu, what):
    r = bar_ratios(got, emu)
    print(f"\n{what}: HIP {_fmt(got)} | emu {_fmt(emu)} | bar use " + " ".join(f"{k} {v:.2f}" for k, v in r.items()))
    bad = {k: v for k, v in r.items() if v > 1.0}
    assert not bad, f"{what}: bars missed {bad} (HIP {_fmt(got)}; emu {_fmt(emu)}; worst utterance {got['worst_utt']})"


# ------------------------------------------------------------------ model, inputs, oracle runs
def _model():
    from oracle.configs import from_model_config
    from simulst_amd.config import mma_model_s
    from simulst_amd.weights import init_model
    cfg = mma_model_s()
    w = {k: v.to(torch.bfloat16).float() for k, v in init_model(cfg, seed=SEED).items() if k.startswith("encoder.")}
    return cfg, w, from_model_config(cfg)[0]


def _fbank(lengths, seed, T=None):
    T = T or max(lengths)
    fb = torch.randn(len(lengths), T, 80, generator=torch.Generator().manual_seed(seed))
    for b, L in enumerate(lengths):
        fb[b, L:] = 0
    return fb.to(torch.bfloat16).float()


def _w64(w):
    return {k: v.double() for k, v in w.items()}


def oracle_forward(w, ecfg, fb, lengths, emulate=None):
    """-> (encoder_out [B, T_e, D] fp64, padding mask [B, T_e]).  emulate: None (exact fp64) or ffn_out_rounded."""
    ctx = bf16_emulation(emulate) if emulate is not None else contextlib.nullcontext()
    with torch.no_grad(), ctx:
        o = oem.encoder_forward(_w64(w), "encoder", ecfg, fb.double(), torch.as_tensor(lengths))
    return o["encoder_out"][0].transpose(0, 1).contiguous(), o["encoder_padding_mask"][0]


def read_schedule(T, first=96, nxt=64):
    """The agent's READ positions: (S + R) x stride frames, then S x stride, the last call with finish (g11 schedule)."""
    pos, out, want = 0, [], first
    while pos < T:
        n = min(want, T - pos)
        pos += n
        out.append((pos, n < want or pos >= T))
        want = nxt
    return out


def oracle_stream(w, ecfg, fb_1t, emulate=None):
    """oracle.encoder_infer over one utterance [1, T, 80] on the READ schedule -> concatenated encoder_out [T_e, D] fp64."""
    ctx = bf16_emulation(emulate) if emulate is not None else contextlib.nullcontext()
    dt = torch.get_default_dtype()
    w64, fb = _w64(w), fb_1t.double()
    st, outs = oem.new_encoder_state(), []
    torch.set_default_dtype(torch.float64)            # init_layer_state's zero states
    try:
        with torch.no_grad(), ctx:
            for pos, fin in read_schedule(fb.size(1)):
                o = oem.encoder_infer(w64, "encoder", ecfg, fb[:, :pos], torch.tensor([pos]), st, fin)
                outs.append(o["encoder_out"][0][:, 0])
    finally:
        torch.set_default_dtype(dt)
    return torch.cat(outs, 0)


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module")
def case40(model):
    """The 40-utterance batch: fbank, lengths, encoder lengths, ref and both emulations (fused / two-launch fc2)."""
    cfg, w, ecfg = model
    fb = _fbank(LENGTHS_40, seed=1040)
    ref, pad = oracle_forward(w, ecfg, fb, LENGTHS_40)
    emu_fused, _ = oracle_forward(w, ecfg, fb, LENGTHS_40, emulate=True)
    emu_two, _ = oracle_forward(w, ecfg, fb, LENGTHS_40, emulate=False)
    enc_len = (~pad).sum(1)
    return dict(fb=fb, lengths=LENGTHS_40, enc_len=enc_len, pad=pad, ref=ref,
                emu={True: bar_stats(emu_fused, ref, enc_len), False: bar_stats(emu_two, ref, enc_len)})


# ------------------------------------------------------------------ CPU: the bars against the emulation and two controls
def test_bars_accept_the_emulation(case40):
    for rounded, s in case40["emu"].items():
        r = bar_ratios(s, s)
        print(f"\nemu (fc2 rounded before the residual: {rounded}): {_fmt(s)}; bar use {r}")
        assert all(v <= 1.0 for v in r.values()), r
    # the two rounding models differ by far less than the bars' margins
    assert case40["emu"][True]["mean"] < 1.25 * case40["emu"][False]["mean"]


def test_bars_reject_a_left_context_four_frames_short(model, case40):
    from dataclasses import replace
    cfg, w, ecfg = model
    y, _ = oracle_forward(w, replace(ecfg, left_context=ecfg.left_context - 4), case40["fb"], case40["lengths"], emulate=True)
    s = bar_stats(y, case40["ref"], case40["enc_len"])
    r = bar_ratios(s, case40["emu"][True])
    print(f"\nleft_context - 4: {_fmt(s)}; bar use {r}")
    assert r["mean"] > 1.0, r


def test_bars_reject_one_utterance_with_one_segment_of_keys_missing(model, case40):
    """Utterance 3 (640 frames -> 160 encoder frames, 10 whole segments) with its attention key length one segment short in
    every layer: only its last segment's 16 frames change."""
    cfg, w, ecfg = model
    b = 3
    assert int(case40["enc_len"][b]) == 160
    forward0 = oem.emformer_forward

    def short_keys(w_, p, cfg_, x, lengths):
        lk = lengths.clone()
        lk[b] -= cfg_.segment_length
        out, _, states = forward0(w_, p, cfg_, x, lk)
        return out, lengths, states

    oem.emformer_forward = short_keys
    try:
        y, _ = oracle_forward(w, ecfg, case40["fb"], case40["lengths"], emulate=True)
    finally:
        oem.emformer_forward = forward0
    s = bar_stats(y, case40["ref"], case40["enc_len"])
    r = bar_ratios(s, case40["emu"][True])
    print(f"\none segment of keys missing in utterance {b}: {_fmt(s)}; bar use {r}")
    assert s["worst_utt"] == b and (r["loc"] > 1.0 or r["mean"] > 1.0), r


# ------------------------------------------------------------------ GPU helpers
@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


SPIED = ("emformer_ffn", "emformer_ffn_prenorm", "emformer_ffn_prenorm_qkv", "emformer_qkv_mem_sum", "emformer_prenorm",
         "linear_ln")


@contextlib.contextmanager
def spy(ops):
    """Call counts of the encoder's launch choices (linear_ln: simulst_linear with a LayerNorm prologue)."""
    counts = dict.fromkeys(SPIED, 0)
    orig = {n: getattr(ops, n) for n in SPIED[:-1] + ("linear",)}

    def counted(name):
        def f(*a, **k):
            counts[name] += 1
            return orig[name](*a, **k)
        return f

    def linear(*a, **k):
        if k.get("ln") is not None:
            counts["linear_ln"] += 1
        return orig["linear"](*a, **k)

    for n in SPIED[:-1]:
        setattr(ops, n, counted(n))
    ops.linear = linear
    try:
        yield counts
    finally:
        for n in orig:
            delattr(ops, n)


def expected_counts(form, L):
    """Launch counts of one forward over L layers at >= fuse_ffn_min_rows rows (encoder.py _emformer_layers)."""
    zero = dict.fromkeys(SPIED, 0)
    if form == "F0":
        return {**zero, "emformer_prenorm": L, "linear_ln": L}
    if form == "F1":
        return {**zero, "emformer_prenorm": L, "emformer_ffn": L}
    if form == "F2":
        return {**zero, "emformer_prenorm": 1, "emformer_ffn_prenorm": L - 1, "emformer_ffn": 1}
    return {**zero, "emformer_prenorm": 1, "emformer_ffn_prenorm_qkv": L - 1, "emformer_qkv_mem_sum": L - 1, "emformer_ffn": 1}


FORMS = {"F0": dict(fuse_ffn=False, fuse_prenorm=False, fuse_qkv=False),
         "F1": dict(fuse_ffn=True, fuse_prenorm=False, fuse_qkv=False),
         "F2": dict(fuse_ffn=True, fuse_prenorm=True, fuse_qkv=False),
         "F3": dict(fuse_ffn=True, fuse_prenorm=True, fuse_qkv=True)}


def _encoder(model, ops, form):
    from simulst_amd.encoder import S2TEmformerEncoder
    cfg, w, _ = model
    enc = S2TEmformerEncoder(cfg, w, dtype=torch.bfloat16, ops=ops)
    for k, v in FORMS[form].items():
        setattr(enc, k, v)
    return enc


def assert_timed_kernels_selected(ops, enc, B, Te):
    """The C-side choices at these shapes: the options at their defaults (handle.cpp) and the row counts of their conditions."""
    from simulst_amd import _lib
    assert ops.h.get_option(_lib.OPT_WEIGHT_STATIONARY) == 1
    assert ops.h.get_option(_lib.OPT_CONV_TILE256) == 2           # 2: the LDS-DMA ring, tile256_ring_kernel
    S, R = enc.cfg.S, enc.cfg.R
    N = math.ceil(Te / S)
    rows_z, rows_c = (N - 1) + N * R + Te + N, N * R + Te + N
    # gemm_plan.cpp tile256_ok: p.M >= 8192 at the second convolution (B x Te output rows)
    assert B * Te >= 8192
    # gemm_plan.cpp wstat_ok: p.M >= 8192 for the Q|K|V product (B x rows_z) and the out-proj (B x rows_c)
    assert B * rows_z >= 8192 and B * rows_c >= 8192


def _run_offline(enc, fb, lengths):
    out = enc.forward(fb.to(torch.bfloat16).cuda(), torch.as_tensor(lengths).cuda())
    torch.cuda.synchronize()
    return out


def _check_offline(out, case, rounded, what):
    assert torch.equal(out["encoder_padding_mask"][0].cpu(), case["pad"])
    assert torch.equal(out["encoder_lengths"].cpu(), case["enc_len"])
    y = out["encoder_out_btd"]
    assert torch.isfinite(y).all()
    assert_bars(bar_stats(y, case["ref"], case["enc_len"]), case["emu"][rounded], what)


# ------------------------------------------------------------------ GPU, offline
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["F0", "F1", "F2", "F3"])
def test_offline_forms_vs_oracle(model, ops, case40, form):
    enc = _encoder(model, ops, form)
    Te = case40["pad"].size(1)
    assert_timed_kernels_selected(ops, enc, len(LENGTHS_40), Te)
    with spy(ops) as counts:
        out = _run_offline(enc, case40["fb"], case40["lengths"])
    assert counts == expected_counts(form, model[0].encoder_layers), counts
    # F0's fc2 adds its residual in fp32 and rounds once; the fused launches round fc2's output first
    _check_offline(out, case40, form != "F0", f"offline 40 utterances {form}")


@pytest.mark.gpu
def test_offline_bench_batch_vs_oracle(model, ops, case40):
    """The bench's joint-encoder size: the 40 utterances x 32 copies = 1 280, default form; every copy against the oracle and
    bit-identical to its first copy (rows at large offsets)."""
    enc = _encoder(model, ops, "F3")
    copies = 32
    fb = case40["fb"].repeat(copies, 1, 1)
    with spy(ops) as counts:
        out = _run_offline(enc, fb, case40["lengths"] * copies)
    assert counts == expected_counts("F3", model[0].encoder_layers), counts
    assert torch.equal(out["encoder_padding_mask"][0].cpu(), case40["pad"].repeat(copies, 1))
    assert torch.equal(out["encoder_lengths"].cpu(), case40["enc_len"].repeat(copies))
    y = out["encoder_out_btd"]
    B0 = len(LENGTHS_40)
    first = y[:B0]
    ref = case40["ref"].cuda()
    # per copy: the copies are not independent frames, so pooling them would shrink bar (d)'s RMS / sqrt(frames) by sqrt(32)
    for c in range(copies):
        yc = y[c * B0:(c + 1) * B0]
        assert torch.equal(yc, first), c
        assert_bars(bar_stats(yc, ref, case40["enc_len"]), case40["emu"][True], f"offline 1280 utterances F3, copy {c}")


@pytest.mark.gpu
def test_offline_prenorm_fallback_vs_oracle(model, ops):
    """Longest utterance 1 030 frames -> 258 encoder frames, 17 segments, 136 right-context rows: 136 % 32 != 0, so the
    default form falls back from the prenorm epilogue to the plain fused feed-forward (encoder.py fuse_prenorm)."""
    cfg, w, ecfg = model
    lengths = [1030] + LENGTHS_40[:31]
    fb = _fbank(lengths, seed=1030)
    ref, pad = oracle_forward(w, ecfg, fb, lengths)
    emu, _ = oracle_forward(w, ecfg, fb, lengths, emulate=True)
    enc_len = (~pad).sum(1)
    Te = pad.size(1)
    assert Te == 258 and (math.ceil(Te / cfg.S) * cfg.R) % 32 != 0
    enc = _encoder(model, ops, "F3")
    assert_timed_kernels_selected(ops, enc, len(lengths), Te)
    with spy(ops) as counts:
        out = _run_offline(enc, fb, lengths)
    assert counts == expected_counts("F1", cfg.encoder_layers), counts
    case = dict(pad=pad, enc_len=enc_len, ref=ref, emu={True: bar_stats(emu, ref, enc_len)})
    _check_offline(out, case, True, "offline 32 utterances, N*R % 32 != 0 (fallback)")


# ------------------------------------------------------------------ GPU, streaming
T_STREAM, N_DISTINCT, N_COPIES = 1003, 16, 28


@pytest.fixture(scope="module")
def stream_case(model):
    cfg, w, ecfg = model
    fb = _fbank([T_STREAM] * N_DISTINCT, seed=2003)
    ref = torch.stack([oracle_stream(w, ecfg, fb[i:i + 1]) for i in range(N_DISTINCT)])
    # the streaming encoder's fc2 is simulst_linear with the residual epilogue: one rounding
    emu = torch.stack([oracle_stream(w, ecfg, fb[i:i + 1], emulate=False) for i in range(N_DISTINCT)])
    n = ref.size(1)
    return dict(fb=fb, ref=ref, emu=emu, n=n)


def _hip_stream(enc, fb):
    inc, outs = {}, []
    B = fb.size(0)
    for pos, fin in read_schedule(fb.size(1)):
        outs.append(enc.infer(fb[:, :pos], torch.full((B,), pos), inc, finish=fin)["encoder_out_btd"])
    torch.cuda.synchronize()
    return torch.cat(outs, 1)


@pytest.mark.gpu
def test_streaming_lockstep_vs_oracle(model, ops, stream_case):
    """448 lockstep streams (16 utterances x 28 copies), T = 1003, READ 96 then 64 frames, with the flush."""
    enc = _encoder(model, ops, "F3")
    fb = stream_case["fb"].repeat(N_COPIES, 1, 1).to(torch.bfloat16).cuda()
    y = _hip_stream(enc, fb)
    assert y.shape == (N_DISTINCT * N_COPIES, stream_case["n"], model[0].embed_dim)
    first = y[:N_DISTINCT]
    for c in range(1, N_COPIES):
        assert torch.equal(y[c * N_DISTINCT:(c + 1) * N_DISTINCT], first), c
    lens = [stream_case["n"]] * N_DISTINCT
    emu = bar_stats(stream_case["emu"], stream_case["ref"], lens)
    assert_bars(bar_stats(first, stream_case["ref"], lens), emu, f"streaming {N_DISTINCT} x {N_COPIES} lockstep")


@pytest.mark.gpu
def test_streaming_single_stream_vs_oracle(model, ops, stream_case):
    """B = 1, the agent's READ path at small row counts, on two of the utterances."""
    enc = _encoder(model, ops, "F3")
    fb = stream_case["fb"][:2].to(torch.bfloat16).cuda()
    y = torch.cat([_hip_stream(enc, fb[i:i + 1]) for i in range(2)])
    lens = [stream_case["n"]] * 2
    emu = bar_stats(stream_case["emu"][:2], stream_case["ref"][:2], lens)
    assert_bars(bar_stats(y, stream_case["ref"][:2], lens), emu, "streaming B = 1")
