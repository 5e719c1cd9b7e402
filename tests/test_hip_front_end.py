"""The front of the pipeline -- simulst_fbank (csrc/fbank.hip), simulst_conv_pos_mfma (csrc/conv_pos_mfma.hip) and, in
csrc/rowops.hip, simulst_conv_pos, simulst_layernorm, simulst_emformer_prenorm, simulst_segment_mean, simulst_emformer_pack_rows,
simulst_embed_tokens and simulst_greedy_argmax -- against the float64 references of tests/front_end_ref.py, at the shapes where each
kernel's tiling changes.  tests/test_front_end_ref_cpu.py ties every reference to its oracle counterpart on every case below, shows
with a mutation table that the cases can fail, and asserts the margins the cases rely on.  This file holds the case tables (plain
data, importable without a GPU) and the GPU tests; every test prints the worst |got - ref| / bound so far for its class and dtype.

FBANK.  Compared in the energy domain, exp(got) against ee = max(e_ref, eps32):
    |exp(got) - ee| <= 4 C * 2^-23 * (||y|| * sum_j w_mj sqrt(P_j) + 2^-23 ||y||^2 * sum_j w_mj) + (2^-21 + 1.5 * 2^-23 |ln ee|) * ee
||y|| is the windowed frame's 2-norm: an FFT in fp32 leaves an error of O(u ||y||) in every bin, whatever the bin holds, so the power
of bin j moves by 2 sqrt(P_j) u ||y|| + (u ||y||)^2 and the mel sum by the bracket.  C is measured, never from the kernel: the worst
ratio, over every element of every row of the signal class in every case, of a float32 evaluation of the same chain on the CPU
(float32 tables, torch.fft.rfft in float32, a float32 mel sum) against the reference; the test asserts 4 C (the radix-2 order is not
torch's).  C is kept PER SIGNAL CLASS, which is never looser than the one C over all cases the issue asked for: that one is 176 and
comes from a single class, imp399 -- the window is 0 at sample 399, what is left after the mean is removed is a constant, and
cur - 0.97 prev of a constant cancels, so the error scales with x and not with y -- while noise sits at 5 to 6; one C for all would
hold the noise cases to 700 u.  The reference reads the pre-emphasis coefficient as the kernel does, as a float32.
The last term is the logf and the test's own exp.  EXTRA TERM, a finding about the bound and not about the kernel: the issue put
2^-21 * ee there, which is one ulp of a float32 in [2, 4) -- but the logs here run from ln eps32 = -15.9 to ln 3e14 = 33, where one
ulp of the stored float32 is up to 2^-18, and a correctly rounded float32 log already moves exp(got) by half of that
(test_front_end_ref_cpu.py::test_fbank_log_term: the CPU float32 chain followed by a float32 log stands at 1.34 of the bound with
2^-21 alone).  The term is 1.5 * 2^-23 |ln ee|: logf compiles to v_log_f32 -- log2 x to one ulp, at most 2^-23 |log2 x| -- times
ln 2 in extended precision (read in the gfx950 assembly of fbank.hip: v_log_f32, then v_mul / v_fmac by 0x3f317217; the one ulp of
v_log_f32 is the ISA's stated accuracy and is supposed here, not measured), which carries that ulp into the result as at most
2^-23 |ln x|, and the result is rounded once more (2^-24 |ln x|).  bf16 output must be the fp32 output rounded (torch.equal).
FLOOR classes (constant, silence: the frame is exactly 0 after the mean is removed, every energy is 0 and the output is ln eps32)
are declared.  So are three narrow-spectrum classes (tone, alternating +-A, imp399), whose far bins lie 1e-13 below the peak, not
1e-7: there 13 to 23 % of the elements lie below their own bound and could hide a wrong value, while the bins that hold the energy
are held to 1e-2 of their value or better.  In every other class the bound stays below 1e-3 of ee at every element (all of this
asserted on the CPU).  Strided rows hold NaN in every sample no frame covers.  Streaming: OnlineFeatureExtractor over chunks of
1 .. 1000 samples equals the one-shot fbank() of the same samples bit for bit, residual counts equal the oracle class's.

CONV-POS.  EXACT class: x, hist = m / 4, W = m / 16, bias = m / 8 with small integers m, so every product and every partial sum is a
multiple of 2^-6 below 2^8 -- exact in fp32 in any order, and in bf16 storage.  The pre-activation is then exact and the bound is
e_gelu + u |ref| with u = 2^-24 (fp32: the rounding of the add x + gelu) or 2^-8 (bf16 store); an indexing error shows at full size.
RANDOM class: |got - ref| <= (n + 2) * 2^-23 * sum |w||x| * 1.13 + e_gelu + store, n = k * cpg, 1.13 the GELU's Lipschitz bound,
store = 2^-8 |ref| for bf16 and 2^-24 |ref| for fp32.  EXTRA TERM, again about the bound: the issue put 0 for fp32, but the add
x + gelu(.) is rounded once in any fp32 kernel; where the window is almost empty (k = 31, cpg = 1, T = 3: sum |w||x| = 2e-4, y = -1.1)
that rounding is the whole error and torch's own fp32 result sits at 0.96 of the bound without the term (0.29 with it, CPU file).
e_gelu = 4 x the largest error of torch's fp32 CPU gelu against math.erf in float64 over
the case's pre-activations and 2049 points spanning their range.  In every ragged case x holds NaN at t >= len: outputs at t < len are
finite (a NaN fails the ratio), outputs at t >= len exactly 0, and a sentinel row behind y stays.  simulst_conv_pos refuses
cpg = 64 with k = 31 and 64 (k cpg^2 floats of weight do not fit its 160 KB of LDS): those two cells of the grid assert the refusal.
Where both kernels take a case each is held to the reference on its own.

LAYERNORM (and the LayerNorm rows of the pre-norm): the recipe of test_alpha_head_vs_fp64.  e32 = the largest error of the same
formula in torch fp32 on the CPU, taken over the 82 rows of the (D, class, dtype) for simulst_layernorm and over the case (at least
3 rows) for the pre-norm: the error of a row is one draw of the rounding error of its mean, amplified by 1 / sigma, and one draw is no
worst case.  |got - ref| <= 4 e32 + 2^-22 (|gamma||z| + |beta|), + 2^-8 |ref| for bf16.  Strided
calls (xs = D + 8, ys = D + 4) hold NaN in X's gaps and a sentinel in Y's.  Refusals: D % 4, D > 1024, xs % 4.
SUMMARIES: the mean of that row bound over the counted rows + cnt * 2^-23 * mean |ln| (fp32 accumulation and the division) + the
store's rounding; the reference averages the UNROUNDED LayerNorm rows, as the kernel does.  segment_mean: cnt * 2^-23 * mean |x| + store.
EXCLUDED, the one declared exclusion: the summary (and segment mean) of a segment that lies wholly at or beyond len (t0 >= len).  The
kernel's comment says nobody reads them; with NaN padding they are NaN.  Every test asserts that exactly those are left out.
PACK-ROWS: torch.equal against the reference's copy.  EMBED: 2^-23 (|scale e| + |pos|), + 2^-8 |ref| for bf16.  ARGMAX: integers.

Measured on an MI355X (worst |got - ref| / bound; C, e32 and e_gelu from the CPU of the same run).  No test takes 2 s, the file 16 s.
  fbank     C_measured: noise 5.06, tone 11.27, tiny 4.83, full 4.33, imp0 3.12, imp1 6.08, imp399 192.5, alt 9.73, floor 0 (the CPU
            these tests were written on gave 6.15, 11.94, 4.33, 6.20, 4.19, 3.85, 176.2, 3.41: C moves with the CPU's FFT path)
            worst ratio: noise 0.651, tone 0.657, tiny 0.399, full 0.624, imp0 0.741, imp1 0.581, imp399 0.157, alt 0.435, floor 0.157;
            in the classes with energies near 1e10 the stored log sits up to 2.2 ulp from ln ee, which is the 1.5 ulp of the term
            plus the spectrum's own error; bf16 == fp32 rounded and streaming == one shot in every case
  conv_pos  (VALU) exact fp32 0.466, bf16 0.996; random fp32 0.355, bf16 0.994; largest e_gelu 4.2e-6 .. 5.1e-6
  conv_pos_mfma    exact bf16 0.996; random bf16 0.982; largest e_gelu 4.8e-6 (bf16 ratios near 1 are the store's rounding alone)
  layernorm fp32: random 0.203, const 0 (exact), mean1000 0.250, huge 0.259; bf16: 0.996, 0.992, 0.994, 0.976;
            largest e32_max 3.3e-4 (fp32, mean1000, D 4) and 4.9e-5 (bf16, mean1000, D 1020)
  prenorm   rows fp32 0.261, bf16 0.996; summaries fp32 0.220, bf16 0.995; largest e32 9.2e-7 / 1.0e-6; 370 of 1800 summaries per
            (D, dtype) left out, all of them segments wholly at or beyond len
  segment_mean fp32 0.329, bf16 0.996;  embed fp32 0.500, bf16 0.985;  pack-rows and argmax exact.
(front-end row.)

Found by these cases and fixed.  (1) fbank() passed wave.stride(0) as the row stride.  For a single row that stride means nothing
-- 0 after a broadcast or after numpy's wave[None] -- and simulst_fbank then refused the call (E_SHAPE, "rows shorter than
(n_frames - 1) * 160 + 400 samples"): the one-shot call of test_fbank_streaming_equals_one_shot failed in all four chunk sequences.
fbank() now passes n when B == 1 (simulst_amd/fbank.py); results of calls that were accepted before are unchanged.  No kernel changed.
Found in the bounds, not in the kernels: the two EXTRA TERMs above; and e32 of a single row -- with e32 taken over the case alone,
the 1-row, D = 252, mean-1000 fp32 case drew 8.4e-6 where its class holds 1.6e-4, and the kernel's 8.3e-5 (0.7 u * 1000 / sigma, what
fp32 gives) stood at 2.46 of the bound; over the class it stands at 0.25.  Not caught by any case, provably (CPU file, docstring):
the mutations preemph0_zero, cnt_no_max and no_last_zero.
"""
import ctypes as C
import functools
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import front_end_ref as fr

U23, U24, BF16_STORE = 2.0 ** -23, 2.0 ** -24, 2.0 ** -8
E_SHAPE = -2
SENTINEL = 1234.0                      # exact in bf16
DTYPES = (torch.float32, torch.bfloat16)
DT_IDS = ("fp32", "bf16")
WORST = {}


def _ratio(got, ref, bound):
    """max |got - ref| / bound; inf where got is not finite or differs at a zero bound"""
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(got, dtype=np.float64) - ref)
        q = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d == 0, 0.0, np.inf))
    q = np.where(np.isfinite(d), q, np.inf)
    return float(q.max()) if q.size else 0.0


def _note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)
    return r


def _report(*keys):
    for key in keys:
        print(f"worst |got - ref| / bound so far, {' '.join(map(str, key))}: {WORST.get(key, 0.0):.4f}")
        if ("e_gelu",) + key in WORST:
            print(f"largest e_gelu so far, {' '.join(map(str, key))}: {WORST[('e_gelu',) + key]:.3e}")


def _seed(*a):
    return zlib.crc32(repr(a).encode())


def _rbf(a):
    """float32 array rounded to bf16 and back"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


# ======================================================================================================================================
# fbank
# ======================================================================================================================================
FB_N = (400, 559, 560, 561, 719, 720, 880)
FB_SIGNALS = ("noise", "tone", "const", "silence", "tiny", "full", "imp0", "imp1", "imp399", "alt")
FB_FLOOR = ("const", "silence")                  # every energy is exactly 0
FB_PARTIAL_FLOOR = ("tone", "alt", "imp399")     # narrow spectra: the far bins lie below their own bound


def _fb_signal(kind, n, rng):
    t = np.arange(n, dtype=np.float64)
    if kind == "noise":
        return np.round(rng.standard_normal(n) * 3000.0)
    if kind == "tone":
        return 8000.0 * np.sin(2.0 * np.pi * 1000.0 * t / 16000.0)
    if kind == "const":
        return np.full(n, 1000.0)
    if kind == "silence":
        return np.zeros(n)
    if kind == "tiny":
        return 1e-3 * rng.standard_normal(n)
    if kind == "full":
        return 32767.0 * np.sign(rng.standard_normal(n))
    if kind in ("imp0", "imp1", "imp399"):
        v = np.zeros(n)
        v[int(kind[3:])::160] = 20000.0                   # the same place in every frame
        return v
    if kind == "alt":
        return 8000.0 * (1.0 - 2.0 * (t % 2))
    raise KeyError(kind)


def _fb_case(kinds, n, n_mel, preemph, pad=0):
    rng = np.random.default_rng(_seed("fbank", kinds, n, n_mel, preemph))
    wave = np.stack([_fb_signal(k_, n, rng) for k_ in kinds]).astype(np.float32)
    # the coefficient as the kernel reads it: a float32
    return dict(kinds=tuple(kinds), wave=wave, n=n, n_mel=n_mel, preemph=float(np.float32(preemph)), pad=pad)


FB_CASES = {}
for _i, _n in enumerate(FB_N):                               # 3, 3, 6, 6, 6, 9 (a workgroup over two utterances), 12 frames
    FB_CASES[f"noise_n{_n}"] = functools.partial(_fb_case, ("noise",) * 3, _n, (64, 80, 128)[_i % 3], (0.97, 0.0)[_i % 2])
for _m in (64, 80, 128):
    for _p in (0.97, 0.0):
        FB_CASES[f"signals_m{_m}_p{_p}"] = functools.partial(_fb_case, FB_SIGNALS, 720, _m, _p)
for _n, _pad in ((561, 37), (719, 1), (880, 400)):
    FB_CASES[f"strided_n{_n}"] = functools.partial(_fb_case, ("noise", "tone", "imp399"), _n, 80, 0.97, _pad)
FB_NAMES = tuple(FB_CASES)


@functools.lru_cache(maxsize=None)
def fb_case(name):
    return FB_CASES[name]()


def fb_frames(n):
    return 1 + (n - 400) // 160


@functools.lru_cache(maxsize=None)
def fb_ref(name, mut=None):
    """per row: dict(e, a, ynorm, wsum) of ref_fbank"""
    c = fb_case(name)
    return tuple(fr.ref_fbank(c["wave"][b].astype(np.float64), c["n_mel"], c["preemph"], mut) for b in range(len(c["kinds"])))


@functools.lru_cache(maxsize=None)
def _fb_tables32(n_mel):
    return torch.from_numpy(fr.povey_window64()).float(), torch.from_numpy(fr.mel_weights64(n_mel)).float()


def fb_f32_chain(wave, n_mel, preemph):
    """the same chain in float32 on the CPU: wave [n] float32 -> mel energies [F, n_mel] float32"""
    win, Wm = _fb_tables32(n_mel)
    w = torch.from_numpy(np.ascontiguousarray(wave, dtype=np.float32))
    fr_ = w.unfold(0, 400, 160).clone()
    fr_ = fr_ - fr_.mean(dim=1, keepdim=True)
    prev = torch.cat([fr_[:, :1], fr_[:, :-1]], dim=1)
    y = (fr_ - torch.tensor(preemph, dtype=torch.float32) * prev) * win
    spec = torch.fft.rfft(y, n=512, dim=1)
    P = spec.real * spec.real + spec.imag * spec.imag
    return P @ Wm.t()


def fb_core(r):
    """the bracket of the bound, [F, n_mel]: ||y|| sum w sqrt(P) + 2^-23 ||y||^2 sum w"""
    return r["ynorm"][:, None] * r["a"] + U23 * (r["ynorm"] ** 2)[:, None] * r["wsum"][None, :]


@functools.lru_cache(maxsize=None)
def fb_C():
    """C_measured per signal class: worst |e32 - e_ref| / (2^-23 * bracket) of the CPU float32 chain over every element of every
    row of that class in every case (floor classes: 0)"""
    worst = {}
    for name in FB_NAMES:
        c = fb_case(name)
        for b, r in enumerate(fb_ref(name)):
            e32 = fb_f32_chain(c["wave"][b], c["n_mel"], c["preemph"]).double().numpy()
            worst[c["kinds"][b]] = max(worst.get(c["kinds"][b], 0.0), _ratio(e32, r["e"], U23 * fb_core(r)))
    return worst


def fb_bound(r, C4, log_term=True):
    ee = np.maximum(r["e"], fr.EPS32)
    last = 2.0 ** -21 + (1.5 * U23 * np.abs(np.log(ee)) if log_term else 0.0)
    return C4 * U23 * fb_core(r) + last * ee, ee


# ======================================================================================================================================
# conv-pos
# ======================================================================================================================================
MFMA_K, MFMA_D = (16, 32, 64), (32, 256)
MFMA_T = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300)
VALU_K, VALU_CPG = (1, 2, 3, 31, 64), (1, 4, 16, 64)
VALU_T = (1, 3, 4, 5, 63, 64, 65, 130)
VALU_REFUSED = ((31, 64), (64, 64))                          # (k, cpg): the weight alone is over the kernel's 160 KB of LDS
LEN_SET = (0, 1, 16, 64, 256, None)                          # None = T
CONV_CLASSES = ("exact", "random")


def conv_lens(T, i):
    """two different lengths (where T allows) from {0, 1, 16, 64, 256, T} clipped to T; i walks the pairs"""
    vals = sorted({min(T, T if v is None else v) for v in LEN_SET})
    a = vals[i % len(vals)]
    b = vals[(i // len(vals) + 1 + i) % len(vals)]
    if a == b:
        b = vals[(vals.index(a) + 1) % len(vals)]
    return [a, b]


def conv_grid(ks, Ts):
    """(k, T, hist, lens) over k x T x {no hist, hist} x {no lengths, lengths}; hist needs k > 1"""
    out, i = [], 0
    for k in ks:
        for T in Ts:
            for hist in (False, True):
                if hist and k == 1:
                    continue
                for ragged in (False, True):
                    out.append((k, T, hist, tuple(conv_lens(T, i)) if ragged else None))
                    i += 1
    return out


MFMA_GRID = conv_grid(MFMA_K, MFMA_T)
VALU_GRID = conv_grid(VALU_K, VALU_T)


@functools.lru_cache(maxsize=64)
def conv_case(cls, bf16, k, cpg, D, T, hist, lens):
    B = 2
    rng = np.random.default_rng(_seed("conv", cls, k, cpg, D, T, hist, lens))
    if cls == "exact":
        x = rng.integers(-4, 5, size=(B, T, D)) / 4.0
        h = rng.integers(-4, 5, size=(B, k - 1, D)) / 4.0
        W = rng.integers(-2, 3, size=(D, cpg, k)) / 16.0
        bias = rng.integers(-4, 5, size=D) / 8.0
    else:
        x = rng.standard_normal((B, T, D))
        h = rng.standard_normal((B, k - 1, D))
        W = rng.standard_normal((D, cpg, k)) / math.sqrt(k * cpg)
        bias = 0.1 * rng.standard_normal(D)
    x, h, W, bias = (a.astype(np.float32) for a in (x, h, W, bias))
    if bf16:
        x, h, W = _rbf(x), _rbf(h), _rbf(W)
    if lens is not None:
        for b, L in enumerate(lens):
            x[b, L:] = np.nan
    c = dict(cls=cls, bf16=bf16, k=k, cpg=cpg, D=D, T=T, x=x, hist=h if hist else None, W=W, bias=bias, lens=lens, groups=D // cpg)
    return c


def conv_ref(c, mut=None):
    f64 = lambda a: None if a is None else a.astype(np.float64)
    return fr.ref_conv_pos(f64(c["x"]), f64(c["hist"]), f64(c["W"]), f64(c["bias"]), c["lens"], c["groups"], mut)


def e_gelu(pre):
    """4 x the largest error of torch's fp32 CPU gelu against math.erf in float64, over the pre-activations and their range"""
    p = pre[np.isfinite(pre)].ravel()
    v = np.concatenate([p, np.linspace(p.min(), p.max(), 2049)]).astype(np.float32) if p.size else np.zeros(1, dtype=np.float32)
    g32 = F.gelu(torch.from_numpy(v)).double().numpy()
    return 4.0 * float(np.abs(g32 - fr.gelu64(v.astype(np.float64))).max())


def conv_bound(c, ref):
    y, pre, mag = ref
    eg = e_gelu(pre)
    if c["cls"] == "exact":
        return eg * (y != 0) + (BF16_STORE if c["bf16"] else U24) * np.abs(y), eg
    n = c["k"] * c["cpg"]
    return ((n + 2) * U23 * mag * 1.13 + eg) * (y != 0) + (BF16_STORE if c["bf16"] else U24) * np.abs(y), eg


def conv_exact_margins(c):
    """EXACT inputs are multiples of 1/4, 1/16, 1/8 and the largest possible sum stays below 2^8: 14 bits, exact in any order"""
    for a, q in ((c["x"], 4), (c["W"], 16), (c["bias"], 8)) + (((c["hist"], 4),) if c["hist"] is not None else ()):
        a = np.nan_to_num(a.astype(np.float64))
        assert np.array_equal(a * q, np.round(a * q))
    assert c["k"] * c["cpg"] * 1.0 * 0.125 + 0.5 <= 256.0


# ======================================================================================================================================
# LayerNorm, pre-norm, segment mean
# ======================================================================================================================================
LN_D = (4, 8, 252, 256, 260, 512, 1020, 1024)
LN_ROWS = (1, 15, 16, 17, 33)
LN_CLASSES = ("random", "const", "mean1000", "huge")
PN_TS = ((1, 4), (5, 16), (16, 16), (17, 16), (33, 16), (40, 17), (41, 40), (7, 1))
PN_RC, PN_MEM, PN_D = (0, 1, 16, 17, 35), (0, 3), (64, 256, 260, 512)
SM_D = PN_D + (1, 80, 300)
PN_B = 3


def ln_formula32(x, g, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * g + b


def _ln_params(D, rng):
    return (0.8 + 0.4 * rng.random(D)).astype(np.float32), (0.1 * rng.standard_normal(D)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ln_case(D, rows, cls, bf16):
    rng = np.random.default_rng(_seed("ln", D, rows, cls))
    g, b = _ln_params(D, rng)
    if cls == "random":
        x = rng.standard_normal((rows, D)) * 1.5 + 0.3
    elif cls == "const":
        x = np.full((rows, D), 0.5)
    elif cls == "mean1000":
        x = 1000.0 + rng.standard_normal((rows, D))
    else:
        x = rng.standard_normal((rows, D))
        x[np.arange(rows), rng.integers(0, D, size=rows)] = 1e4
    x = x.astype(np.float32)
    if bf16:
        x = _rbf(x)
    y, z = fr.ref_layernorm(x.astype(np.float64), g.astype(np.float64), b.astype(np.float64))
    e32 = float(np.abs(ln_formula32(torch.from_numpy(x), torch.from_numpy(g), torch.from_numpy(b)).double().numpy() - y).max())
    return dict(x=x, g=g, b=b, y=y, z=z, e32=e32)


def ln_e32_max(D, cls, bf16):
    """the largest e32 over every row count of the class: 82 rows.  One row's e32 is ONE draw of the mean's rounding error (which
    1 / sigma amplifies: u * 1000 for the mean-1000 class), far too few for a worst case"""
    return max(ln_case(D, rows, cls, bf16)["e32"] for rows in LN_ROWS)


def ln_bound(y, z, g, b, e32, bf16):
    with np.errstate(all="ignore"):
        return 4.0 * e32 + 2.0 ** -22 * (np.abs(g) * np.abs(z) + np.abs(b)) + (BF16_STORE * np.abs(y) if bf16 else 0.0)


def pn_lens(T, S):
    """None and two length vectors that together hold T, 1, the middle of a segment, exactly a segment start t0 and t0 + 1"""
    N = -(-T // S)
    t0 = S * (N // 2) if N > 1 else 0                                      # a segment start inside the utterance (0 only when N = 1)
    mid = min(T, t0 + max(1, (min(t0 + S, T) - t0 + 1) // 2))
    cl = lambda v: max(1, min(T, v))
    return (None, (T, 1, cl(mid)), (cl(t0), cl(t0 + 1), cl(mid)))


def pn_grid():
    """(T, S, n_rc, n_mem, with_sum, lens)"""
    return [(T, S, rc, mem, ws, lens) for (T, S) in PN_TS for rc in PN_RC for mem in PN_MEM for ws in (False, True)
            for lens in pn_lens(T, S)]


PN_GRID = pn_grid()


@functools.lru_cache(maxsize=16)
def pn_case(D, bf16, T, S, n_rc, lens):
    """X [B, n_rc + T, D] with NaN rows at t >= len, its reference and e32 (n_mem and n_sum only place the rows in Z)"""
    rng = np.random.default_rng(_seed("pn", D, T, S, n_rc, lens))
    g, b = _ln_params(D, rng)
    X = (rng.standard_normal((PN_B, n_rc + T, D)) * 1.5 + 0.3).astype(np.float32)
    if bf16:
        X = _rbf(X)
    if lens is not None:
        for i, L in enumerate(lens):
            X[i, n_rc + L:] = np.nan
    ln, z, summ, cnt, mabs = fr.ref_prenorm(X.astype(np.float64), g.astype(np.float64), b.astype(np.float64), lens, T, n_rc, S)
    with np.errstate(all="ignore"):
        l32 = ln_formula32(torch.from_numpy(X), torch.from_numpy(g), torch.from_numpy(b)).double().numpy()
        e32 = float(np.nanmax(np.abs(l32 - ln)))
    return dict(X=X, g=g, b=b, ln=ln, z=z, summ=summ, cnt=cnt, mabs=mabs, e32=e32)


def pn_live(T, S, lens):
    """[B, N] bool: the segment starts inside the row (t0 < len) -- the summaries that are compared"""
    N = -(-T // S)
    L = np.array([T] * PN_B if lens is None else lens)
    return (np.arange(N)[None, :] * S) < L[:, None]


def pn_summary_bound(c, T, S, n_rc, bf16):
    """mean over the counted rows of the row bound + cnt 2^-23 mean |ln| + store"""
    N = -(-T // S)
    rowb = ln_bound(c["ln"], c["z"], c["g"], c["b"], c["e32"], False)
    out = np.zeros((PN_B, N, c["X"].shape[2]))
    for bb in range(PN_B):
        for i in range(N):
            n = int(c["cnt"][bb, i])
            with np.errstate(all="ignore"):
                out[bb, i] = rowb[bb, n_rc + i * S:n_rc + i * S + n].mean(axis=0) + n * U23 * c["mabs"][bb, i]
    with np.errstate(all="ignore"):
        return out + (BF16_STORE * np.abs(c["summ"]) if bf16 else 0.0)


@functools.lru_cache(maxsize=8)
def sm_case(D, bf16, T, S, lens):
    rng = np.random.default_rng(_seed("sm", D, T, S, lens))
    X = (rng.standard_normal((PN_B, T, D)) * 1.5 + 0.3).astype(np.float32)
    if bf16:
        X = _rbf(X)
    if lens is not None:
        for i, L in enumerate(lens):
            X[i, L:] = np.nan
    N = -(-T // S)
    out, cnt, mabs = fr.ref_segment_mean(X.astype(np.float64), lens, S, N)
    return dict(X=X, out=out, cnt=cnt, mabs=mabs)


# ======================================================================================================================================
# pack-rows, embed, argmax
# ======================================================================================================================================
PK_TSR = ((3, 4, 2), (16, 4, 0), (16, 4, 1), (17, 4, 4), (17, 4, 6), (9, 4, 3), (300, 16, 4))
PK_D, PK_B = (8, 80, 256, 264), (1, 3)
EMB_D = (1, 80, 256, 300)
AM_V = (1, 2, 255, 256, 257, 1000, 10001)
AM_TOP = 100.0


@functools.lru_cache(maxsize=None)
def pk_case(T, S, R, D, B, bf16):
    rng = np.random.default_rng(_seed("pk", T, S, R, D, B))
    x = rng.standard_normal((B, T, D)).astype(np.float32)
    return _rbf(x) if bf16 else x


def am_case(V):
    """rows of integer-valued logits below AM_TOP with AM_TOP planted; returns logits [B, V], eos_bias [B], pad_idx, eos_idx, names"""
    rng = np.random.default_rng(_seed("argmax", V))
    pad, eos = (1, 2) if V > 2 else ((1, -1) if V == 2 else (-1, -1))
    rows, bias, names = [], [], []

    def add(name, cols, eb=0.0, fill=None, extra=()):
        if any(c >= V or c < 0 for c in cols) or len(set(cols)) != len(cols):
            return
        v = rng.integers(-50, 50, size=V).astype(np.float32) if fill is None else np.full(V, fill, dtype=np.float32)
        for c in cols:
            v[c] = AM_TOP
        for c, val in extra:
            if c >= V:
                return
            v[c] = val
        rows.append(v), bias.append(eb), names.append(name)

    add("last", [V - 1])
    add("first", [0])
    add("two_lanes", [5, 37])
    add("two_waves", [138, 10])
    add("same_thread", [263, 7])
    add("same_thread_0_256", [256, 0])
    add("all_at_once", [532, 276, 84, 52, 20])
    add("all_at_once_wrapped", [9000, 4116, 276, 148, 20])
    add("pad_max", [pad], extra=((V - 1, 60.0),)) if pad >= 0 and V > 2 else None
    add("pad_max_v2", [pad]) if V == 2 else None
    add("eos_max", [eos], extra=((V - 1, 70.0),)) if eos >= 0 else None
    add("eos_bias_wins", [], eb=20.0, extra=((eos, 90.0), (0, 99.0))) if eos >= 0 else None
    add("eos_bias_ties_lower", [0], eb=8.0, extra=((eos, AM_TOP - 8.0),)) if eos >= 0 else None
    add("eos_bias_ties_higher", [V - 1], eb=8.0, extra=((eos, AM_TOP - 8.0),)) if eos >= 0 and V - 1 > eos else None
    add("all_neg_inf", [], fill=-np.inf)
    add("all_equal", [], fill=3.0)
    return np.stack(rows), np.array(bias, dtype=np.float32), pad, eos, names


# ======================================================================================================================================
# what the case tables launch (from the tables, not from a profiler)
# ======================================================================================================================================
FB_OUT_DTYPES = DTYPES                                       # test_fbank_vs_fp64 launches every case once per entry


def launched_instantiations():
    """the template instantiations the GPU tests launch, from the iterables they are parametrised on and loop over:
    test_conv_pos_mfma_vs_fp64 takes k from MFMA_K and the rows of MFMA_GRID with that k; test_layernorm_vs_fp64 takes D from LN_D,
    dtype from DTYPES and every rows of LN_ROWS; test_fbank_vs_fp64 takes name from FB_NAMES and out dtype from FB_OUT_DTYPES"""
    mfma = {k // 2 for k in MFMA_K if any(k_ == k and T > 0 for (k_, T, _, _) in MFMA_GRID)}
    ln = {(1 if D <= 256 else 4, dt) for D in LN_D for dt in DTYPES if len(LN_ROWS) > 0}
    fb = {dt for dt in FB_OUT_DTYPES for name in FB_NAMES if fb_frames(fb_case(name)["n"]) > 0}
    return mfma, ln, fb


def test_every_instantiation_has_a_case():
    """conv_pos_mfma_kernel<8 | 16 | 32> (k = 16, 32, 64), layernorm_kernel<T, 1> (D <= 256) and <T, 4> (D > 256) in both dtypes,
    fbank_kernel<float | bf16>"""
    mfma, ln, fb = launched_instantiations()
    assert mfma == {8, 16, 32}
    assert ln == {(nv, dt) for nv in (1, 4) for dt in (torch.float32, torch.bfloat16)}
    assert fb == {torch.float32, torch.bfloat16}


# ======================================================================================================================================
# GPU
# ======================================================================================================================================
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


def vp(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _tdt(dtype):
    from simulst_amd import _lib
    return _lib.F32 if dtype == torch.float32 else _lib.BF16


# ---- fbank ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fb_tables(n_mel):
    from simulst_amd.fbank import FbankTables
    return FbankTables(torch.device("cuda"), n_mel)


def _fb_run(ops, c, dtype):
    """the kernel on the case's rows; strided cases sit in a wider NaN buffer with NaN behind each row's last frame"""
    from simulst_amd.fbank import fbank
    B, n = c["wave"].shape
    F_ = fb_frames(n)
    if c["pad"] == 0:
        return fbank(ops, _fb_tables(c["n_mel"]), _dev(c["wave"]), out_dtype=dtype, preemphasis=c["preemph"])
    buf = torch.full((B, n + c["pad"]), float("nan"))
    covered = (F_ - 1) * 160 + 400
    buf[:, :covered] = torch.from_numpy(c["wave"][:, :covered])
    buf = buf.cuda()
    tb = _fb_tables(c["n_mel"])
    out = torch.empty(B, F_, c["n_mel"], device="cuda", dtype=dtype)
    ops.h.check(ops.lib.simulst_fbank(ops.h.ptr, vp(buf), n + c["pad"], vp(tb.window), vp(tb.tw_cos), vp(tb.tw_sin), vp(tb.mel_lo),
                                      vp(tb.mel_w), vp(out), B, F_, c["n_mel"], c["preemph"], _tdt(dtype)), "simulst_fbank")
    return out


@pytest.mark.parametrize("name", FB_NAMES)
def test_fbank_vs_fp64(ops, name):
    c = fb_case(name)
    outs = {dt: _fb_run(ops, c, dt) for dt in FB_OUT_DTYPES}
    got, got16 = outs[torch.float32], outs[torch.bfloat16]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()), (name, "non-finite output")
    assert torch.equal(got16, got.to(torch.bfloat16)), (name, "bf16 is not the fp32 result rounded")
    g = np.exp(got.cpu().double().numpy())
    for b, r in enumerate(fb_ref(name)):
        bound, ee = fb_bound(r, 4.0 * fb_C()[c["kinds"][b]])
        key = ("fbank", "floor" if c["kinds"][b] in FB_FLOOR else c["kinds"][b])
        q = _note(key, _ratio(g[b], ee, bound))
        assert q <= 1.0, (name, b, c["kinds"][b], "|exp(got) - max(e, eps)| / bound", q)
    print("C_measured", {k_: round(v, 2) for k_, v in fb_C().items()})
    _report(*sorted({("fbank", "floor" if k_ in FB_FLOOR else k_) for k_ in c["kinds"]}))


STREAM_CHUNKS = ((1, 159, 160, 161, 399, 400, 401, 1000), (1000, 401, 400, 399, 161, 160, 159, 1),
                 (400, 160, 160, 1, 1, 159, 1000, 161, 399, 401), (399, 1, 159, 1, 160, 161))


@pytest.mark.parametrize("chunks", STREAM_CHUNKS, ids=lambda c: "-".join(map(str, c)))
def test_fbank_streaming_equals_one_shot(ops, chunks):
    """a frame is a pure function of its 400 samples: the frames of the chunked run are those of fbank() over all samples, bit for
    bit, and the residual carried between calls has the length the oracle class carries"""
    from oracle.fbank import OnlineFeatureExtractor as OracleExtractor
    from simulst_amd.fbank import OnlineFeatureExtractor, fbank
    rng = np.random.default_rng(_seed("stream", chunks))
    total = sum(chunks)
    wave = np.round(rng.standard_normal(total) * 3000.0).astype(np.float32)
    ex, orc = OnlineFeatureExtractor(ops), OracleExtractor()
    one = fbank(ops, ex.tables, _dev(wave[None]))[0]
    frames, lo = [], 0
    for n_new in chunks:
        got = ex(wave[lo:lo + n_new])
        ref = orc(wave[lo:lo + n_new].tolist())
        lo += n_new
        assert (got is None) == (ref is None)
        assert int(ex.previous_residual_samples.numel()) == len(orc.previous_residual_samples), (lo, "residual count")
        if got is not None:
            assert got.shape[0] == ref.shape[0]
            frames.append(got)
    torch.cuda.synchronize()
    n_got = sum(f.shape[0] for f in frames)
    assert n_got == (fb_frames(total) if total >= 400 else 0) and n_got > 0
    assert torch.equal(torch.cat(frames), one[:n_got])


# ---- conv-pos -------------------------------------------------------------------------------------------------------------------------
def _conv_run(ops, c, mfma):
    dtype = torch.bfloat16 if c["bf16"] else torch.float32
    B, T, D = c["x"].shape
    ybuf = torch.full((B * T + 1, D), SENTINEL, device="cuda", dtype=dtype)
    y = ybuf[:B * T].view(B, T, D)
    x, W, bias = _dev(c["x"], dtype), _dev(c["W"], dtype), _dev(c["bias"])
    hist = _dev(c["hist"], dtype) if c["hist"] is not None else None
    lens = torch.tensor(c["lens"], dtype=torch.int32).cuda() if c["lens"] is not None else None
    if mfma:
        ops.conv_pos_mfma(x, hist, ops.pack_conv_pos_weight(W), bias, lens, c["groups"], out=y)
    else:
        ops.conv_pos(x, hist, W, bias, lens, c["groups"], out=y)
    return ybuf, y


def _conv_check(c, ybuf, y, key, what):
    ref = conv_ref(c)
    bound, eg = conv_bound(c, ref)
    WORST[("e_gelu",) + key] = max(WORST.get(("e_gelu",) + key, 0.0), eg)
    assert bool((ybuf[-1] == SENTINEL).all()), (what, "the row behind y was written")
    got = y.cpu().double().numpy()
    if c["lens"] is not None:
        for b, L in enumerate(c["lens"]):
            assert not got[b, L:].any() and np.isfinite(got[b, L:]).all(), (what, b, "output at t >= len is not exactly 0")
    q = _note(key, _ratio(got, ref[0], bound))
    assert q <= 1.0, (what, "|got - ref| / bound", q)


@pytest.mark.parametrize("cls", CONV_CLASSES)
@pytest.mark.parametrize("D", MFMA_D)
@pytest.mark.parametrize("k", MFMA_K)
def test_conv_pos_mfma_vs_fp64(ops, k, D, cls):
    key = ("conv_pos_mfma", cls, "bf16")
    runs = []
    for (k_, T, hist, lens) in MFMA_GRID:
        if k_ == k:
            c = conv_case(cls, True, k, 16, D, T, hist, lens)
            runs.append((c, (T, hist, lens)) + _conv_run(ops, c, True))
    torch.cuda.synchronize()
    for c, what, ybuf, y in runs:
        _conv_check(c, ybuf, y, key, what)
    _report(key)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("cpg", VALU_CPG)
@pytest.mark.parametrize("k", VALU_K)
def test_conv_pos_valu_vs_fp64(ops, k, cpg, dtype):
    bf16 = dtype == torch.bfloat16
    D = 4 * cpg
    if (k, cpg) in VALU_REFUSED:
        t = torch.zeros(64, device="cuda", dtype=dtype)
        b = torch.zeros(D, device="cuda")
        rc = ops.lib.simulst_conv_pos(ops.h.ptr, vp(t), None, vp(t), vp(b), None, vp(t), 1, 1, D, 4, k, _tdt(dtype))
        torch.cuda.synchronize()
        assert rc == E_SHAPE and bool((t == 0).all())
        return
    for cls in CONV_CLASSES:
        key = ("conv_pos", cls, "bf16" if bf16 else "fp32")
        runs = []
        for (k_, T, hist, lens) in VALU_GRID:
            if k_ == k:
                c = conv_case(cls, bf16, k, cpg, D, T, hist, lens)
                runs.append((c, (cls, T, hist, lens)) + _conv_run(ops, c, False))
        torch.cuda.synchronize()
        for c, what, ybuf, y in runs:
            _conv_check(c, ybuf, y, key, what)
        _report(key)


@pytest.mark.parametrize("cls", CONV_CLASSES)
@pytest.mark.parametrize("k", MFMA_K)
def test_conv_pos_valu_on_the_mfma_cases(ops, k, cls):
    """bf16, cpg 16, k 16 / 32 / 64 is taken by both kernels: the VALU kernel against the reference on the D = 32 cases of the MFMA
    table (each kernel on its own, never against the other)"""
    key = ("conv_pos", cls, "bf16")
    runs = []
    for (k_, T, hist, lens) in MFMA_GRID:
        if k_ == k:
            c = conv_case(cls, True, k, 16, 32, T, hist, lens)
            runs.append((c, (T, hist, lens)) + _conv_run(ops, c, False))
    torch.cuda.synchronize()
    for c, what, ybuf, y in runs:
        _conv_check(c, ybuf, y, key, what)
    _report(key)


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D", LN_D)
def test_layernorm_vs_fp64(ops, D, dtype):
    bf16 = dtype == torch.bfloat16
    runs = []
    for rows in LN_ROWS:
        for cls in LN_CLASSES:
            c = ln_case(D, rows, cls, bf16)
            g, b = _dev(c["g"]), _dev(c["b"])
            dense = ops.layernorm(_dev(c["x"], dtype), g, b)
            xs, ys = D + 8, D + 4
            X = torch.full((rows, xs), float("nan"), dtype=dtype)
            X[:, :D] = torch.from_numpy(c["x"]).to(dtype)
            X = X.cuda()
            Y = torch.full((rows, ys), SENTINEL, device="cuda", dtype=dtype)
            ops.h.check(ops.lib.simulst_layernorm(ops.h.ptr, vp(X), vp(g), vp(b), vp(Y), rows, D, xs, ys, _tdt(dtype)), "simulst_layernorm")
            runs.append((rows, cls, c, dense, Y))
    torch.cuda.synchronize()
    for rows, cls, c, dense, Y in runs:
        key = ("layernorm", cls, DT_IDS[bf16])
        e32 = ln_e32_max(D, cls, bf16)
        bound = ln_bound(c["y"], c["z"], c["g"], c["b"], e32, bf16)
        assert bool((Y[:, D:] == SENTINEL).all()), (rows, cls, "Y's gap was written")
        assert torch.equal(Y[:, :D], dense), (rows, cls, "strided and dense calls differ")
        q = _note(key, _ratio(dense.cpu().double().numpy(), c["y"], bound))
        WORST[("layernorm e32_max", DT_IDS[bf16])] = max(WORST.get(("layernorm e32_max", DT_IDS[bf16]), 0.0), e32)
        assert q <= 1.0, (rows, cls, "|got - ref| / bound", q, "e32_max", e32, "this case's e32", c["e32"])
        if cls == "const":
            assert torch.equal(dense.cpu().float(), torch.from_numpy(c["b"]).to(dtype).float().expand(rows, D)), "variance 0: y = beta"
    _report(*[("layernorm", cls, DT_IDS[bf16]) for cls in LN_CLASSES])
    print(f"largest e32_max so far, {DT_IDS[bf16]}: {WORST[('layernorm e32_max', DT_IDS[bf16])]:.3e}")


def test_layernorm_refusals(ops):
    """D % 4 != 0, D > 1024, xs % 4 != 0 (and ys): E_SHAPE, nothing launched"""
    from simulst_amd import _lib
    t = torch.zeros(4 * 1100, device="cuda")
    rc = lambda D, xs, ys: ops.lib.simulst_layernorm(ops.h.ptr, vp(t), vp(t), vp(t), vp(t), 2, D, xs, ys, _lib.F32)
    assert rc(6, 8, 8) == E_SHAPE
    assert rc(1028, 1028, 1028) == E_SHAPE
    assert rc(8, 10, 8) == E_SHAPE and rc(8, 8, 10) == E_SHAPE
    assert rc(0, 8, 8) == E_SHAPE
    torch.cuda.synchronize()
    assert bool((t == 0).all())


# ---- pre-norm and segment mean ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D", PN_D)
def test_emformer_prenorm_vs_fp64(ops, D, dtype):
    bf16 = dtype == torch.bfloat16
    kl, ks = ("prenorm rows", DT_IDS[bf16]), ("prenorm summaries", DT_IDS[bf16])
    runs, gb = [], {}
    for (T, S, n_rc, n_mem, with_sum, lens) in PN_GRID:
        c = pn_case(D, bf16, T, S, n_rc, lens)
        N = -(-T // S)
        n_sum = N if with_sum else 0
        rows_z = n_mem + n_rc + T + n_sum
        Zbuf = torch.full((PN_B * rows_z + N + 1, D), SENTINEL, device="cuda", dtype=dtype)     # N + 1 guard rows behind the batch
        Z = Zbuf[:PN_B * rows_z].view(PN_B, rows_z, D)
        lt = torch.tensor(lens, dtype=torch.int32).cuda() if lens is not None else None
        ops.emformer_prenorm(_dev(c["X"], dtype), _dev(c["g"]), _dev(c["b"]), lt, Z, T=T, n_mem=n_mem, n_rc=n_rc, n_sum=n_sum, seg_len=S)
        runs.append(((T, S, n_rc, n_mem, with_sum, lens), c, Zbuf, Z))
    torch.cuda.synchronize()
    n_excl = n_all = 0
    for what, c, Zbuf, Z in runs:
        T, S, n_rc, n_mem, with_sum, lens = what
        N = -(-T // S)
        rows_z = Z.shape[1]
        assert bool((Zbuf[PN_B * rows_z:] == SENTINEL).all()), (what, "rows behind Z were written")
        assert bool((Z[:, :n_mem] == SENTINEL).all()), (what, "memory rows were written")
        got = Z.cpu().double().numpy()
        L = [T] * PN_B if lens is None else lens
        bound = ln_bound(c["ln"], c["z"], c["g"], c["b"], c["e32"], bf16)
        WORST[("prenorm e32", DT_IDS[bf16])] = max(WORST.get(("prenorm e32", DT_IDS[bf16]), 0.0), c["e32"])
        for bb in range(PN_B):
            sl = slice(0, n_rc + L[bb])                           # right-context rows and the row's own frames
            q = _note(kl, _ratio(got[bb, n_mem:n_mem + n_rc + L[bb]], c["ln"][bb, sl], bound[bb, sl]))
            assert q <= 1.0, (what, bb, "LayerNorm rows: |got - ref| / bound", q)
        if with_sum:
            live = pn_live(T, S, lens)
            n_all += live.size
            n_excl += int((~live).sum())
            assert np.array_equal(~live, (np.arange(N)[None, :] * S) >= np.array(L)[:, None])     # only segments wholly beyond len
            sb = pn_summary_bound(c, T, S, n_rc, bf16)
            gs = got[:, n_mem + n_rc + T:]
            q = _note(ks, _ratio(gs[live], c["summ"][live], sb[live]))
            assert q <= 1.0, (what, "summaries: |got - ref| / bound", q)
    print(f"summaries left out (segments wholly at or beyond len): {n_excl} of {n_all}")
    _report(kl, ks)
    print(f"largest e32 so far, prenorm {DT_IDS[bf16]}: {WORST[('prenorm e32', DT_IDS[bf16])]:.3e}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D", SM_D)
def test_segment_mean_vs_fp64(ops, D, dtype):
    bf16 = dtype == torch.bfloat16
    key = ("segment_mean", DT_IDS[bf16])
    runs = []
    for (T, S) in PN_TS:
        N = -(-T // S)
        for lens in pn_lens(T, S):
            c = sm_case(D, bf16, T, S, lens)
            for n_out in sorted({1, max(1, N - 1), N}):
                Xb = torch.full((PN_B, T + 2, D), float("nan"), dtype=dtype)
                Xb[:, :T] = torch.from_numpy(c["X"]).to(dtype)
                Xb = Xb.cuda()
                out = torch.full((PN_B, n_out + 1, D), SENTINEL, device="cuda", dtype=dtype)
                lt = torch.tensor(lens, dtype=torch.int32).cuda() if lens is not None else None
                ops.segment_mean(Xb, lt, out, T=T, x_bs=(T + 2) * D, o_bs=(n_out + 1) * D, seg_len=S, n_out=n_out)
                runs.append(((T, S, lens, n_out), c, out))
    torch.cuda.synchronize()
    for what, c, out in runs:
        T, S, lens, n_out = what
        assert bool((out[:, n_out:] == SENTINEL).all()), (what, "rows behind the output were written")
        live = pn_live(T, S, lens)[:, :n_out]
        assert np.array_equal(~live, (np.arange(n_out)[None, :] * S) >= np.array([T] * PN_B if lens is None else lens)[:, None])
        with np.errstate(all="ignore"):
            bound = c["cnt"][:, :n_out, None] * U23 * c["mabs"][:, :n_out] + (BF16_STORE * np.abs(c["out"][:, :n_out]) if bf16 else 0.0)
        q = _note(key, _ratio(out[:, :n_out].cpu().double().numpy()[live], c["out"][:, :n_out][live], bound[live]))
        assert q <= 1.0, (what, "|got - ref| / bound", q)
    _report(key)


def test_segment_mean_refusal(ops):
    """n_out * S >= T + S (a segment that starts at or beyond T): E_SHAPE, nothing launched"""
    from simulst_amd import _lib
    t = torch.zeros(64, device="cuda")
    o = torch.full((64,), SENTINEL, device="cuda")
    rc = lambda T, S, n_out: ops.lib.simulst_segment_mean(ops.h.ptr, vp(t), None, vp(o), 1, T, 4, T * 4, n_out * 4, S, n_out, _lib.F32)
    assert rc(8, 4, 3) == E_SHAPE and rc(9, 4, 4) == E_SHAPE and rc(1, 4, 2) == E_SHAPE
    assert rc(9, 4, 3) == 0
    torch.cuda.synchronize()
    assert bool((o[12:] == SENTINEL).all()) and bool((o[:12] == 0).all())


# ---- pack-rows --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_pack_rows_equals_reference(ops, dtype):
    bf16 = dtype == torch.bfloat16
    runs = []
    for (T, S, R) in PK_TSR:
        N = -(-T // S)
        for D in PK_D:
            for B in PK_B:
                x = pk_case(T, S, R, D, B, bf16)
                rows = N * R + T
                Xbuf = torch.full((B * rows + 1, D), SENTINEL, device="cuda", dtype=dtype)
                ops.h.check(ops.lib.simulst_emformer_pack_rows(ops.h.ptr, vp(_dev(x, dtype)), vp(Xbuf), B, T, D, S, R, N, _tdt(dtype)),
                            "simulst_emformer_pack_rows")
                runs.append(((T, S, R, D, B), x, Xbuf))
    torch.cuda.synchronize()
    assert any(((-(-T // S)) * R + T) * (D // 4) > 64 * 256 for (T, S, R) in PK_TSR for D in PK_D), "no case loops over the grid twice"
    for what, x, Xbuf in runs:
        T, S, R, D, B = what
        N = -(-T // S)
        ref = torch.from_numpy(fr.ref_pack_rows(x, S, R, N)).to(dtype)
        assert bool((Xbuf[-1] == SENTINEL).all()), (what, "the row behind X was written")
        assert torch.equal(Xbuf[:-1].cpu().view(B, N * R + T, D), ref), what


def test_pack_rows_refusals(ops):
    """D % 8 != 0 and n_seg != ceil(T / S): E_SHAPE, nothing launched"""
    from simulst_amd import _lib
    t = torch.zeros(512, device="cuda")
    o = torch.full((512,), SENTINEL, device="cuda")
    rc = lambda T, D, S, R, N: ops.lib.simulst_emformer_pack_rows(ops.h.ptr, vp(t), vp(o), 1, T, D, S, R, N, _lib.F32)
    assert rc(9, 12, 4, 1, 3) == E_SHAPE and rc(9, 4, 4, 1, 3) == E_SHAPE
    assert rc(9, 8, 4, 1, 2) == E_SHAPE and rc(9, 8, 4, 1, 4) == E_SHAPE and rc(8, 8, 4, 1, 3) == E_SHAPE
    torch.cuda.synchronize()
    assert bool((o == SENTINEL).all())


# ---- embed ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D", EMB_D)
def test_embed_tokens_vs_fp64(ops, D, dtype):
    bf16 = dtype == torch.bfloat16
    key = ("embed", DT_IDS[bf16])
    V, P = 50, 12
    rng = np.random.default_rng(_seed("embed", D))
    E = rng.standard_normal((V, D)).astype(np.float32)
    if bf16:
        E = _rbf(E)
    pos = rng.standard_normal((P, D)).astype(np.float32)
    tokens = np.array([0, V - 1, 7, 7, V - 1, 0, 23, 1], dtype=np.int64)
    pos_row = np.array([3, 0, 3, 11, 1, 0, 11, 5], dtype=np.int32)
    for scale in (1.0, math.sqrt(D)):
        s32 = float(np.float32(scale))
        ref, mag = fr.ref_embed(tokens, E.astype(np.float64), pos.astype(np.float64), pos_row, s32)
        buf = torch.full((len(tokens) + 1, D), SENTINEL, device="cuda", dtype=dtype)
        ops.embed_tokens(_dev(tokens), _dev(E, dtype), _dev(pos), _dev(pos_row), scale, out=buf[:-1])
        torch.cuda.synchronize()
        assert bool((buf[-1] == SENTINEL).all())
        bound = U23 * mag + (BF16_STORE * np.abs(ref) if bf16 else 0.0)
        q = _note(key, _ratio(buf[:-1].cpu().double().numpy(), ref, bound))
        assert q <= 1.0, (D, scale, "|got - ref| / bound", q)
    _report(key)


# ---- argmax -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", AM_V)
def test_greedy_argmax_equals_reference(ops, V):
    logits, bias, pad, eos, names = am_case(V)
    dl, db = _dev(logits), _dev(bias)
    for mask_eos in (False, True):
        for use_bias in (False, True):
            buf = torch.full((len(names) + 1,), -7, device="cuda", dtype=torch.int64)
            ops.greedy_argmax(dl, pad_idx=pad, eos_idx=eos, mask_eos=mask_eos, eos_bias=db if use_bias else None, out=buf[:-1])
            torch.cuda.synchronize()
            ref = fr.ref_argmax(logits.astype(np.float64), pad, eos, mask_eos, bias.astype(np.float64) if use_bias else None)
            got = buf.cpu().numpy()
            assert got[-1] == -7
            bad = [(n_, int(g_), int(r_)) for n_, g_, r_ in zip(names, got[:-1], ref) if g_ != r_]
            assert not bad, (V, mask_eos, use_bias, bad)
