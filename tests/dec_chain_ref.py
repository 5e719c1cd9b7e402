"""The four decoder layer-chain launches in float64, written from the comment block of include/simulst_hip.h ("Row-local chains of the
decoder layer ...", "The closing launch of a decode step ...") and from nothing in csrc/.

One function per VISIBLE stage, so that a stage can be fed the kernel's own output of the stage before it; every stage returns its
unrounded float64 value and, per output element, the bound a correct bf16 / fp32 implementation is held to:

  stage_residual(ctx, x, W, b)                         x + W ctx + b, S = sum |ctx||W| + |b| + |x|     (first stage of the proj / ffn chain)
  stage_ln_proj(x, gamma, beta, W, b, kk=None)         W bf16(LN(x)) + b, or gelu_erf(. + kk)             (q, q2, qkv, the logits)
  stage_slab(x_mid, gamma, beta, W1, b1, W2, sp)       fp32 slab `sp`: W2[:, 256 sp ..] bf16(gelu_erf(W1[256 sp ..] bf16(LN(x_mid)) + b1))
  stage_slab_sum(x_mid, b2, slabs)                     x_mid + b2 + slab 0 + slab 1 + ..., T = sum |terms|
  pick(logits, lo, hi, skip_a, skip_b, row_bias, row_bias_col)     (largest value, its lowest column) of columns [lo, hi)
  fold(vals, cols)                                     the same rule over the `split` pairs of a row

Bounds (u24 = 2^-24, u23 = 2^-23; every operand is a bf16 or fp32 number, products of two bf16 numbers are exact in fp32)
  contraction   an fp32 accumulation of K exact products plus bias (plus residual, plus kk) in any order: (K + 3) u23 S with S the sum
                of the magnitudes, the bound simulst_linear is held to (tests/linear_cases.py, `core`).
  slab sum      n slabs added one after the other to x_mid + b2 in fp32: n + 1 roundings, (n + 3) u23 T in the same form.
  store         a bf16 output adds half a bf16 spacing at |ref| + (the other terms); the fp32 slabs and the logits add none.
  GELU          the kernels' fitted erf GELU is within E_GELU_FIT = 7.1e-7 of gelu_erf in fp32 (csrc/common.h); an error e of its
                argument passes through with sup |gelu'| = 1.13.
  LayerNorm     the kernels take one-pass moments in fp32: mean^ = sum x / 256, var^ = max(sum x^2 / 256 - mean^2, 0).  With sums of 256
                terms over a tree of at most 8 levels behind at most 4 roundings inside a lane (at most C_MEAN = 10 roundings for sum x,
                12 for sum x^2), mean^2 carries 2 * 10 + 1 roundings of a number <= E[x^2], the subtraction one more:
                    |var^ - var| <= C_VAR u24 E[x^2],  C_VAR = 12 + 21 + 1 = 34         (the clamp only moves var^ towards var >= 0)
                    |mean^ - mean| <= C_MEAN u24 E|x|
                so with r = C_VAR u24 E[x^2] / (var + eps) -- the CANCELLATION term, 1 + (offset / deviation)^2 times larger for a row
                with a common offset -- rstd^ = rstd (1 + rho), |rho| <= 1 / sqrt(1 - r) - 1 + 4 u24 (sqrt, add, divide), r < 1/2 asserted.
                y^ = ((x - mean^) rstd^) gamma + beta in fp32 (4 roundings, or fewer with fused multiply-adds) is then within
                    e(y) = |gamma| rstd (C_MEAN u24 E|x| + u24 |x - mean|) + |gamma z| (rho + 3 u24) + 2 u24 (|gamma z| + |beta|)
                of y.  A CONSTANT row of bf16 numbers is exact: k c and k c^2 (k <= 256, c of 8 significant bits) fit in 24 bits, so
                every partial sum in any order is exact, mean^ = c, var^ = 0, x - mean^ = 0 and y^ = beta: e(y) = 0 there.

Hidden roundings.  The LayerNorm output and the GELU output are rounded to bf16 inside the launch and never leave it.  The reference
rounds them to nearest (round_once).  A hidden value v whose fp32 twin v^ is known to lie within e(v) of it rounds to the SAME bf16
number unless v lies within e(v) of a rounding midpoint (fragile); a fragile value may come out one bf16 spacing away, u(|v| + e(v))
-- or, where e(v) exceeds half that spacing (values next to zero), e(v) + u(|v| + e(v)) away.  The stage's FLIP TERM of output j is the
sum over the fragile k of |w_jk| times that amount, in place of the all-elements-may-flip 2^-8 sum |w||v|.  A LayerNorm flip enters fc1
through |W1| u(y) before the GELU output's own e is formed: e(h) = 1.13 (flip(y) + (K + 3) u23 S1) + 7.1e-7.

`mut` names one deliberate error (MUTANTS); tests/test_dec_chain_ref_cpu.py shows that the case table sees each of them.
"""
import math

import numpy as np

D = 256
LN_EPS = 1e-5
U23, U24 = 2.0 ** -23, 2.0 ** -24
GELU_LIP = 1.13                       # sup |gelu'|
E_GELU_FIT = 7.1e-7                   # csrc/common.h: the bf16 kernels' fitted GELU, error of the result in fp32
C_MEAN, C_VAR = 10.0, 34.0            # roundings behind mean^ and var^ (module docstring)

MUTANTS = ("last_k_step_dropped", "slab_last_k_step_dropped", "slab_9_skipped", "slab_masked_tail_added_twice", "b2_dropped",
           "last_tile_row_from_row_0", "x_mid_from_x", "ln_eps_1e-6", "ln_unbiased_variance", "ln_without_clamp_sign",
           "ln_output_not_rounded", "gelu_output_not_rounded", "gelu_tanh_form", "kk_dropped", "kk_added_after_gelu", "q2_from_wq",
           "qkv_block_1_and_2_swapped", "bias_of_block_0_on_every_block", "pick_highest_column_on_tie",
           "pick_ge_instead_of_gt_across_lanes", "skip_before_row_bias", "row_bias_on_every_range", "skip_b_ignored",
           "fold_takes_first_pair")

_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu64(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


# ======================================================================================================================================
# bf16 helpers
# ======================================================================================================================================
def bf16_spacing(v):
    """distance between neighbouring bf16 numbers (8 significant bits) in the binade of |v|; at a power of two the spacing ABOVE it;
    below the smallest normal number the subnormal spacing 2^-133"""
    a = np.abs(np.asarray(v, dtype=np.float64))
    _, e = np.frexp(a)                                       # a = m 2^e, m in [1/2, 1)
    e = np.where(a == 0, -10000, e)
    return np.ldexp(1.0, np.maximum(e, -125) - 8)


def round_once(v):
    """float64 -> the nearest bf16 number, ties to the even significand, as float64"""
    v = np.asarray(v, dtype=np.float64)
    sp = bf16_spacing(v)
    return np.round(v / sp) * sp                             # np.round: halves to the even integer = the even significand


def midpoint_distance(v):
    """distance of |v| to the nearest point where bf16 rounding changes its result: the midpoints of v's own binade, the last one of
    the binade below (half the spacing there) and the first one of the binade above"""
    a = np.abs(np.asarray(v, dtype=np.float64))
    sp = bf16_spacing(a)
    lo = 128.0 * sp                                          # the binade is [lo, 2 lo)
    t = a / sp
    own = np.abs(t - np.floor(t) - 0.5) * sp
    below = a - (lo - 0.25 * sp)
    above = (2.0 * lo + sp) - a
    return np.minimum(own, np.minimum(below, above))


def fragile(v, e):
    """True where a number within e of v may round to another bf16 number than v does"""
    return midpoint_distance(v) <= e


def flip_amount(v, e):
    """how far the bf16 rounding of a number within e of v can lie from round_once(v), given that it differs"""
    u = bf16_spacing(np.abs(v) + e)
    return np.where(e <= 0.5 * u, u, e + u)


def hidden_round(v, e, rounded=True):
    """-> (the value the next contraction reads, per-element flip amount: 0 where v is not fragile)"""
    return (round_once(v) if rounded else v), np.where(fragile(v, e), flip_amount(v, e), 0.0)


def to_bf16_bits(v):
    """bf16-representable float64 -> int16 bit patterns"""
    f = np.ascontiguousarray(v, dtype=np.float64).astype(np.float32)
    assert np.array_equal(f.astype(np.float64), np.asarray(v, dtype=np.float64))
    bits = f.view(np.uint32)
    assert not (bits & 0xFFFF).any(), "not a bf16 number"
    return (bits >> 16).astype(np.uint16).view(np.int16)


# ======================================================================================================================================
# stages
# ======================================================================================================================================
def layer_norm(x, gamma, beta, mut=None):
    """-> (y unrounded, e: bound on |the kernels' fp32 y - y|, module docstring)"""
    n = x.shape[1]
    mean = x.mean(1, keepdims=True)
    d = x - mean
    var = (d * d).mean(1, keepdims=True)
    if mut == "ln_unbiased_variance":
        var = var * n / (n - 1)
    if mut == "ln_without_clamp_sign":                       # the clamp with the wrong sign: min(var, 0) for max(var, 0)
        var = np.minimum(var, 0.0)
    rstd = 1.0 / np.sqrt(var + (1e-6 if mut == "ln_eps_1e-6" else LN_EPS))
    z = d * rstd
    y = z * gamma[None] + beta[None]
    const = (x.max(1, keepdims=True) == x.min(1, keepdims=True))
    r = C_VAR * U24 * (x * x).mean(1, keepdims=True) / (var + LN_EPS)
    assert mut is not None or (r[~const] < 0.5).all(), "a row whose one-pass variance has no correct digit"
    rho = 1.0 / np.sqrt(1.0 - np.minimum(r, 0.5)) - 1.0 + 4 * U24
    zg = np.abs(gamma)[None] * np.abs(z)
    e = np.abs(gamma)[None] * rstd * (C_MEAN * U24 * np.abs(x).mean(1, keepdims=True) + U24 * np.abs(d)) + zg * (rho + 3 * U24) + \
        2 * U24 * (zg + np.abs(beta)[None])
    return y, np.where(const, 0.0, e)


def stage_residual(ctx, x, W, b, mut=None):
    """-> (x + W ctx + b unrounded, S = sum |ctx||W| + |b| + |x|)"""
    c, r = ctx, x
    if mut == "last_k_step_dropped":
        c = ctx.copy()
        c[:, -32:] = 0.0
    if mut == "last_tile_row_from_row_0" and x.shape[0] % 16 != 0 and x.shape[0] > 1:
        r = x.copy()
        r[-1] = x[0]
    val = r + c @ W.T + b[None]
    if mut == "x_mid_from_x":
        val = x.copy()
    return val, np.abs(ctx) @ np.abs(W).T + np.abs(b)[None] + np.abs(x)


def residual_bound(val, S, K=D):
    core = (K + 3) * U23 * S
    return core + 0.5 * bf16_spacing(np.abs(val) + core)


def stage_ln_proj(x, gamma, beta, W, b, kk=None, mut=None, out_bf16=True):
    """x: the bf16 rows the LayerNorm reads.  -> (value unrounded, per-element bound, info)"""
    N, K = W.shape
    y, e = layer_norm(x, gamma, beta, mut)
    yb, amt = hidden_round(y, e, rounded=mut != "ln_output_not_rounded")
    absW = np.abs(W)
    flip = amt @ absW.T
    yk = yb
    if mut == "last_k_step_dropped":
        yk = yb.copy()
        yk[:, -32:] = 0.0
    bv = np.zeros(N) if b is None else np.asarray(b, dtype=np.float64)
    if mut == "bias_of_block_0_on_every_block" and N > 256:
        bv = np.tile(bv[:256], N // 256)
    pre = yk @ W.T + bv[None]
    if mut == "qkv_block_1_and_2_swapped" and N == 768:
        pre = np.concatenate([pre[:, :256], pre[:, 512:], pre[:, 256:512]], axis=1)
    S = np.abs(yb) @ absW.T + np.abs(bv)[None]
    info = dict(frag_ln=amt > 0, allflip=2.0 ** -8 * (np.abs(y) @ absW.T))
    if kk is None:
        val, bound = pre, flip + (K + 3) * U23 * S
    else:
        S = S + np.abs(kk)
        g = gelu_tanh64 if mut == "gelu_tanh_form" else gelu64
        if mut == "kk_dropped":
            val = g(pre)
        elif mut == "kk_added_after_gelu":
            val = g(pre) + kk
        else:
            val = g(pre + kk)
        bound = GELU_LIP * (flip + (K + 3) * U23 * S) + E_GELU_FIT
    if out_bf16:
        bound = bound + 0.5 * bf16_spacing(np.abs(val) + bound)
    return val, bound, info


def stage_slab(x_mid, gamma, beta, W1, b1, W2, sp, mut=None):
    """-> (fp32 slab `sp` unrounded, per-element bound, info: pre-activations and the shares the CPU test prints)"""
    K = x_mid.shape[1]
    y, e = layer_norm(x_mid, gamma, beta, mut)
    yb, amt = hidden_round(y, e, rounded=mut != "ln_output_not_rounded")
    W1s, b1s, W2s = W1[256 * sp:256 * sp + 256], b1[256 * sp:256 * sp + 256], W2[:, 256 * sp:256 * sp + 256]
    pre = yb @ W1s.T + b1s[None]
    e_pre = amt @ np.abs(W1s).T + (K + 3) * U23 * (np.abs(yb) @ np.abs(W1s).T + np.abs(b1s)[None])
    h = (gelu_tanh64 if mut == "gelu_tanh_form" else gelu64)(pre)
    e_h = GELU_LIP * e_pre + E_GELU_FIT
    hb, amt_h = hidden_round(h, e_h, rounded=mut != "gelu_output_not_rounded")
    hk = hb
    if mut == "slab_last_k_step_dropped":
        hk = hb.copy()
        hk[:, -32:] = 0.0
    val = hk @ W2s.T
    bound = amt_h @ np.abs(W2s).T + (256 + 3) * U23 * (np.abs(hb) @ np.abs(W2s).T)
    info = dict(pre=pre, frag_ln=amt > 0, frag_h=amt_h > 0,
                allflip=2.0 ** -8 * (np.abs(h) @ np.abs(W2s).T), hb=hb, W2s=W2s)
    return val, bound, info


def stage_slab_sum(x_mid, b2, slabs, mut=None):
    """slabs [n][B][256] -> (x_mid + b2 + slab 0 + slab 1 + ... unrounded, T = sum |terms|)"""
    n = slabs.shape[0]
    val = x_mid + (0.0 if mut == "b2_dropped" else b2[None])
    for k in range(n):
        if not (mut == "slab_9_skipped" and k == 8):
            val = val + slabs[k]
    if mut == "slab_masked_tail_added_twice" and n % 8:       # the slots of the last batch of eight beyond n re-read slab n - 1
        val = val + (8 - n % 8) * slabs[n - 1]
    return val, np.abs(x_mid) + np.abs(b2)[None] + np.abs(slabs).sum(0)


def slab_sum_bound(val, T, n):
    core = (n + 3) * U23 * T
    return core + 0.5 * bf16_spacing(np.abs(val) + core)


# ======================================================================================================================================
# the vocabulary pick
# ======================================================================================================================================
def biased_logits(L, bound, row_bias, row_bias_col):
    """the logits the pick sees: row_bias[row] added to column row_bias_col (one more fp32 rounding there)"""
    if row_bias is None:
        return L, bound
    L, bound = L.copy(), bound.copy()
    L[:, row_bias_col] += row_bias
    bound[:, row_bias_col] += U24 * (np.abs(L[:, row_bias_col]) + np.abs(row_bias)) + bound[:, row_bias_col] * U24
    return L, bound


def _lane(c):
    """which lane of a workgroup holds column c of a 256-column weight block: (wave, group of four columns of a 16-column tile)"""
    return (c % 256) // 64 * 4 + (c % 16) // 4


def pick(logits, lo, hi, skip_a, skip_b, row_bias, row_bias_col, mut=None):
    """logits [B][V] WITHOUT the addend.  -> (val [B], col [B]): the largest value over columns [lo, hi) and its lowest column, the
    addend row_bias[row] on column row_bias_col first, then columns skip_a / skip_b (-1: none) excluded"""
    Lr = logits[:, lo:hi].copy()
    n = hi - lo
    rb_at = None
    if row_bias is not None:
        if mut == "row_bias_on_every_range":
            rb_at = row_bias_col % n
        elif lo <= row_bias_col < hi:
            rb_at = row_bias_col - lo
    if rb_at is not None:
        Lr[:, rb_at] += row_bias
    resurrect = Lr[:, rb_at].copy() if rb_at is not None else None
    for s in (skip_a,) + (() if mut == "skip_b_ignored" else (skip_b,)):
        if lo <= s < hi:
            Lr[:, s - lo] = -np.inf
    if mut == "skip_before_row_bias" and rb_at is not None:   # the addend's column is written after the exclusions
        Lr[:, rb_at] = resurrect
    best = Lr.max(1)
    tied = Lr == best[:, None]
    cols = np.arange(n)
    if mut == "pick_highest_column_on_tie":
        col = np.where(tied, cols[None], -1).max(1)
    elif mut == "pick_ge_instead_of_gt_across_lanes":         # lowest inside a lane, but the later lane wins a tie
        lanes = _lane(cols + lo)
        col = np.empty(Lr.shape[0], dtype=np.int64)
        for i in range(Lr.shape[0]):
            t = cols[tied[i]]
            firsts = [t[lanes[t] == ln].min() for ln in np.unique(lanes[t])]
            col[i] = max(firsts)
    else:
        col = np.where(tied, cols[None], n).min(1)
    return best, col + lo


def fold(vals, cols, mut=None):
    """vals / cols [B][split] -> (val [B], col [B]) by the (largest value, lowest column) rule"""
    if mut == "fold_takes_first_pair":
        return vals[:, 0].copy(), cols[:, 0].copy()
    best = vals.max(1)
    tied = vals == best[:, None]
    if mut in ("pick_highest_column_on_tie", "pick_ge_instead_of_gt_across_lanes"):
        return best, np.where(tied, cols, -1).max(1)
    return best, np.where(tied, cols, np.iinfo(np.int64).max).min(1)


def check_pick(val, col, L, bound, lo, hi, skip_a, skip_b, tie_group=()):
    """the conditions a pair (val, col) of columns [lo, hi) is held to against the biased logits L and their bounds:
         col lies in the range and is not skipped;  |val - L[col]| <= bound[col];  no admissible column c of the range has
         L[c] - bound[c] > L[col] + bound[col];  a column of tie_group (duplicated weight rows: exactly equal logits) is picked only
         if it is the lowest admissible member of the group in the range.
    -> (list of violations, worst |val - L[col]| / bound[col])"""
    bad = []
    rows = np.arange(L.shape[0])
    col = np.asarray(col, dtype=np.int64)
    inside = (col >= lo) & (col < hi) & (col != skip_a) & (col != skip_b)
    if not inside.all():
        return [f"rows {rows[~inside][:5].tolist()}: column {col[~inside][:5].tolist()} outside [{lo}, {hi}) or skipped"], np.inf
    at, bat = L[rows, col], bound[rows, col]
    ratio = np.abs(val - at) / bat
    if (ratio > 1.0).any():
        i = int(ratio.argmax())
        bad.append(f"row {i}: value {val[i]!r} at column {col[i]}, reference {at[i]!r}, bound {bat[i]:.3e}")
    adm = np.ones(L.shape[1], dtype=bool)
    adm[:lo] = False
    adm[hi:] = False
    for s in (skip_a, skip_b):
        if 0 <= s < L.shape[1]:
            adm[s] = False
    lower = np.where(adm[None], L - bound, -np.inf).max(1)
    beaten = lower > at + bat
    if beaten.any():
        i = int(rows[beaten][0])
        bad.append(f"row {i}: column {col[i]} ({at[i]!r} + {bat[i]:.3e}) is beaten by column "
                   f"{int(np.where(adm[None], L - bound, -np.inf)[i].argmax())} ({lower[i]!r} after its bound)")
    g = [c for c in tie_group if adm[c]]
    if g:
        wrong = np.isin(col, g) & (col != min(g))
        if wrong.any():
            bad.append(f"rows {rows[wrong][:5].tolist()}: column {col[wrong][:5].tolist()} picked, the tie's lowest column is {min(g)}")
    return bad, float(ratio.max())
