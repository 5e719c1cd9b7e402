"""The one case table of tests/test_dec_chain_ref_cpu.py and tests/test_hip_dec_chain_fp64.py: which launches of the decoder layer chains
are made and with what operands.  The stages and their bounds are tests/dec_chain_ref.py's.

Rows B: 1 (one live row in the tile), 15 (one short), 16 (full tile), 17 (one live row in the second tile), 33 (two full tiles plus one
row), 129 (the first row count at which the decode plan uses the chains).  The kernels tile 16 rows per workgroup whatever B is.

Row classes.  Row i of a case is of class CLASSES[(i + rot) % 9], so that every case of 15 rows or more carries all of them in one launch
(a one-row case carries the class its `rot` gives it; the one-row cases of a chain differ in rot).  The class is a property of the row
the LayerNorm of the launch READS, which is an output of the launch's first stage, x + W ctx + b or x_mid + b2 + slabs; b is shared by
the rows, so a special row is built through that stage:
  normal   N(0, 1) operands
  exact    small integers and dyadic fractions: ctx in {-1, 0, 1} on the columns k % 8 == 3 where W holds multiples of 1/4 up to 1/2,
           x multiples of 1/4 up to 2, b multiples of 1/8 up to 1 (slab sum: x_mid multiples of 1/4, slabs multiples of 1/4 up to 1/2):
           every partial sum is a multiple of 1/8 below 32, exact in fp32 AND in bf16 -- x must equal the reference bit for bit
  tiny     variance about 1.5e-5, so eps is seen: ctx = 2^-9 N(0, 1), x = -b (slab sum: x_mid = -b2, slab 0 = 2^-8 N(0, 1), others 0)
  const    every element 4: ctx = 0, x = 4 - b (exact); variance 0, LN(x) = beta
  off8, off32   N(0, 1) around a common offset of 8 and 32 standard deviations (ctx = 0, x = bf16(offset + N(0, 1) - b))
  big      N(0, 1) scaled by 2^6 (ctx = 0)
  ctx0     ctx = 0, x N(0, 1)          (slab sum and vocabulary chain: `cancel` -- slab 0 = 2^10 N(0, 1), slab 1 = -slab 0)

Feed-forward weights: the hidden units 32 .. 63 of every slab have their fc1 rows scaled by 1/4 and b1 = -9, the units 64 .. 95 likewise
with b1 = +9: pre-activations below -6 (the GELU's exp2 flushes) and above +6 (the GELU is the identity); the CPU test asserts both.

Vocabulary weights: row 5 of Wout is scaled by 6 (so that it is a row's largest logit in about a third of the rows) and copied to row
`tie`: the two logits tie exactly whatever LayerNorm gives.  skip modes: 0 none; 1 (1, a random column); 2 both in the last range;
3 skip_b == row_bias_col (the addend must not resurrect the column); 4 skip_a == 5 (the tie's other column must win).
row_bias: None, or 50 on every third row and N(0, 0.1) elsewhere.

No NaN or Inf is placed in an input, and no index outside its buffer is given to a launch.
"""
import zlib

import numpy as np

import dec_chain_ref as R

D = 256
ROWS = (1, 15, 16, 17, 33, 129)
CLASSES = ("normal", "exact", "tiny", "const", "off8", "off32", "big", "ctx0", "normal")
SUM_CLASSES = ("normal", "exact", "tiny", "const", "off8", "off32", "big", "cancel", "normal")
EXACT_CLASSES = ("exact",)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def row_classes(B, rot, classes=CLASSES):
    return [classes[(i + rot) % len(classes)] for i in range(B)]


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _weight(rng, N, K, dyadic=False):
    w = rng.standard_normal((N, K)) / np.sqrt(K)
    if dyadic:
        w[:, 3::8] = rng.integers(-2, 3, (N, K // 8)) / 4.0
    return R.round_once(w)


def _dyadic_bias(rng, n):
    return rng.integers(-8, 9, n) / 8.0


def _ln_params(rng):
    return f32(0.8 + 0.4 * rng.random(D)), f32(0.1 * rng.standard_normal(D))


def _target(rng, cls):
    z = rng.standard_normal(D)
    return {"const": np.full(D, 4.0), "off8": 8.0 + z, "off32": 32.0 + z, "big": 64.0 * z}[cls]


def _residual_rows(rng, classes, b):
    """ctx, x [B][256] (bf16 numbers) such that row i of x + W ctx + b is of class classes[i]"""
    B = len(classes)
    ctx, x = np.zeros((B, D)), np.zeros((B, D))
    for i, c in enumerate(classes):
        if c == "normal":
            ctx[i], x[i] = rng.standard_normal(D), rng.standard_normal(D)
        elif c == "exact":
            ctx[i, 3::8] = rng.integers(-1, 2, D // 8)
            x[i] = rng.integers(-8, 9, D) / 4.0
        elif c == "tiny":
            ctx[i], x[i] = 2.0 ** -9 * rng.standard_normal(D), -b
        elif c == "ctx0":
            x[i] = rng.standard_normal(D)
        else:
            x[i] = _target(rng, c) - b
    return R.round_once(ctx), R.round_once(x)


def _sum_rows(rng, classes, b2, n):
    """x_mid [B][256] (bf16 numbers), slabs [n][B][256] (fp32 numbers) such that row i of x_mid + b2 + slabs is of class classes[i]"""
    B = len(classes)
    x_mid, slabs = np.zeros((B, D)), np.zeros((n, B, D))
    for i, c in enumerate(classes):
        if c in ("normal", "cancel"):
            x_mid[i] = rng.standard_normal(D)
            slabs[:, i] = 0.3 * rng.standard_normal((n, D))
            if c == "cancel" and n >= 2:
                slabs[0, i] = f32(1024.0 * rng.standard_normal(D))
                slabs[1, i] = -slabs[0, i]
        elif c == "exact":
            x_mid[i] = rng.integers(-8, 9, D) / 4.0
            slabs[:, i] = rng.integers(-2, 3, (n, D)) / 4.0
        elif c == "tiny":
            x_mid[i] = -b2
            slabs[0, i] = 2.0 ** -8 * rng.standard_normal(D)
        else:
            x_mid[i] = _target(rng, c) - b2
    return R.round_once(x_mid), f32(slabs)


# ======================================================================================================================================
# the table
# ======================================================================================================================================
PROJ_CASES, FFN_CASES, SUM_CASES, VOCAB_CASES = [], [], [], []

for _i, _B in enumerate(ROWS):
    for _j, _v in enumerate(("q", "q2", "kk", "kkb")):       # wq2_fm NULL / given; the kk form with bq NULL / given
        PROJ_CASES.append(dict(name=f"proj-{_v}-B{_B}", B=_B, variant=_v, rot=(1, 3, 6, 7)[_j] if _B == 1 else 0))
for _F, _rows in ((256, ROWS), (2048, ROWS), (2304, ROWS), (8192, (1, 17, 33))):      # 1, 8, 9 and 32 slabs
    for _i, _B in enumerate(_rows):
        FFN_CASES.append(dict(name=f"ffn-F{_F}-B{_B}", B=_B, F=_F, rot={256: 0, 2048: 2, 2304: 4, 8192: 6}[_F] if _B == 1 else 0))
for _n, _rows in ((1, ROWS), (8, ROWS), (9, ROWS), (32, (1, 17, 33))):
    for _i, _B in enumerate(_rows):
        SUM_CASES.append(dict(name=f"sum-n{_n}-B{_B}" + ("-qkv" if (_i + _n) % 2 == 0 else ""), B=_B, n=_n, qkv=(_i + _n) % 2 == 0,
                              rot={1: 1, 8: 3, 9: 5, 32: 7}[_n] if _B == 1 else 0))
#                    V, split,   B,  n, skip mode, row_bias, its column, the column tied with column 5
for _row in ((256, 1, 1, 1, 0, False, 7, 9),
             (256, 1, 15, 2, 1, True, 7, 6),                  # the same lane
             (256, 1, 16, 8, 3, True, 7, 21),                 # the next column tile of the wave
             (256, 1, 17, 9, 4, False, 7, 69),                # the next wave
             (512, 2, 1, 2, 0, True, 7, 6),
             (512, 2, 17, 2, 0, True, 7, 256 + 5),            # the next range: decided by the fold
             (512, 2, 33, 1, 2, True, 256 + 7, 69),           # the addend in a range other than range 0
             (1024, 1, 16, 2, 1, False, 7, 261),              # the next weight block of the workgroup
             (1024, 1, 129, 8, 0, True, 7, 261),
             (4096, 16, 15, 2, 1, True, 7, 256 + 5),
             (4096, 16, 33, 9, 3, True, 3 * 256 + 7, 21),
             (4096, 16, 129, 2, 0, False, 7, 9),              # a neighbouring lane group
             (16384, 64, 17, 32, 1, True, 7, 256 + 5)):       # the limit
    _V, _s, _B, _n, _m, _rb, _rc, _t = _row
    VOCAB_CASES.append(dict(name=f"vocab-V{_V}-s{_s}-B{_B}-n{_n}-m{_m}" + ("-rb" if _rb else "") + f"-tie{_t}", V=_V, split=_s, B=_B, n=_n,
                            mode=_m, row_bias=_rb, row_bias_col=_rc, tie=_t, rot=len(VOCAB_CASES) if _B == 1 else 0))

ALL_CASES = PROJ_CASES + FFN_CASES + SUM_CASES + VOCAB_CASES
BY_NAME = {c["name"]: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


# ======================================================================================================================================
# operands: float64 numpy arrays holding bf16 numbers (activations, weights) or fp32 numbers (biases, LayerNorm vectors, slabs)
# ======================================================================================================================================
def proj_operands(c):
    rng = _rng(c["name"])
    classes = row_classes(c["B"], c["rot"])
    bo = _dyadic_bias(rng, D)
    ctx, x = _residual_rows(rng, classes, bo)
    gamma, beta = _ln_params(rng)
    v = c["variant"]
    o = dict(classes=classes, ctx=ctx, x=x, Wo=_weight(rng, D, D, dyadic=True), bo=bo, gamma=gamma, beta=beta, Wq=_weight(rng, D, D),
             bq=None if v == "kk" else f32(0.5 * rng.standard_normal(D)), Wq2=None, bq2=None, kk=None)
    if v == "q2":
        o["Wq2"], o["bq2"] = _weight(rng, D, D), f32(0.5 * rng.standard_normal(D))
    if v in ("kk", "kkb"):
        o["kk"] = R.round_once(rng.standard_normal((c["B"], D)))
    return o


def ffn_operands(c):
    rng = _rng(c["name"])
    F = c["F"]
    classes = row_classes(c["B"], c["rot"])
    bco = _dyadic_bias(rng, D)
    ctx, x = _residual_rows(rng, classes, bco)
    gamma, beta = _ln_params(rng)
    W1, b1 = rng.standard_normal((F, D)) / 16.0, 0.1 * rng.standard_normal(F)
    unit = np.arange(F) % 256
    lo, hi = (unit >= 32) & (unit < 64), (unit >= 64) & (unit < 96)
    W1[lo | hi] *= 0.25
    b1[lo], b1[hi] = -9.0, 9.0
    return dict(classes=classes, ctx=ctx, x=x, Wco=_weight(rng, D, D, dyadic=True), bco=bco, gamma=gamma, beta=beta, W1=R.round_once(W1),
                b1=f32(b1), W2=_weight(rng, D, F), b2=_dyadic_bias(rng, D), flush=lo[:256], ident=hi[:256])


def sum_operands(c):
    rng = _rng(c["name"])
    classes = row_classes(c["B"], c["rot"], SUM_CLASSES)
    b2 = _dyadic_bias(rng, D)
    x_mid, slabs = _sum_rows(rng, classes, b2, c["n"])
    gamma, beta = _ln_params(rng)
    o = dict(classes=classes, x_mid=x_mid, slabs=slabs, b2=b2, gamma=gamma, beta=beta, Wqkv=None, bqkv=None)
    if c.get("qkv"):
        o["Wqkv"], o["bqkv"] = _weight(rng, 3 * D, D), f32(0.5 * rng.standard_normal(3 * D))
    return o


def vocab_operands(c):
    o = sum_operands(c)
    rng = _rng(c["name"] + "/vocab")
    V, split, B = c["V"], c["split"], c["B"]
    VC = V // split
    W = rng.standard_normal((V, D)) / 16.0
    W[5] *= 6.0
    W[c["tie"]] = W[5]
    o["Wout"] = R.round_once(W)
    rc = c["row_bias_col"]
    o["row_bias"] = f32(np.where(np.arange(B) % 3 == 0, 50.0, 0.1 * rng.standard_normal(B))) if c["row_bias"] else None
    m = c["mode"]
    if m == 0:
        sa, sb = -1, -1
    elif m == 1:
        sa, sb = 1, int(rng.integers(0, V))
        if sb in (rc, 5, c["tie"]):
            sb += 1
    elif m == 2:
        sa, sb = (split - 1) * VC + 2, (split - 1) * VC + 11
    elif m == 3:
        sa, sb = 1, rc
    else:
        sa, sb = 5, -1
    o.update(skip_a=sa, skip_b=sb, VC=VC, tie_group=(5, c["tie"]), row_bias_col=rc)
    return o


def class_rows(classes):
    """{class: row indices}"""
    out = {}
    for i, c in enumerate(classes):
        out.setdefault(c, []).append(i)
    return {k: np.array(v) for k, v in out.items()}


# ======================================================================================================================================
# the stages of a launch, each on the VISIBLE input of that stage: `seen` holds the bf16 / fp32 arrays the stage before left (the
# kernel's own in the GPU test, the rounded reference in the CPU test); mut mutates the stages, never their inputs
# ======================================================================================================================================
def proj_stages(o, seen=None, mut=None):
    """-> {"x": (val, bound), "q": ..., "q2": ...}"""
    val, S = R.stage_residual(o["ctx"], o["x"], o["Wo"], o["bo"], mut)
    out = {"x": (val, R.residual_bound(val, S))}
    xw = seen["x"] if seen else R.round_once(val)
    out["q"] = R.stage_ln_proj(xw, o["gamma"], o["beta"], o["Wq"], o["bq"], kk=o["kk"], mut=mut)[:2]
    if o["Wq2"] is not None:
        W, b = (o["Wq"], o["bq"]) if mut == "q2_from_wq" else (o["Wq2"], o["bq2"])
        out["q2"] = R.stage_ln_proj(xw, o["gamma"], o["beta"], W, b, mut=mut)[:2]
    return out


def ffn_stages(o, seen=None, mut=None, info=None):
    """-> {"x_mid": (val, bound), "slabs": ([n][B][256] val, bound), "x": (val, bound)}"""
    n = o["W1"].shape[0] // 256
    val, S = R.stage_residual(o["ctx"], o["x"], o["Wco"], o["bco"], mut)
    out = {"x_mid": (val, R.residual_bound(val, S))}
    xm = seen["x_mid"] if seen else R.round_once(val)
    sl = [R.stage_slab(xm, o["gamma"], o["beta"], o["W1"], o["b1"], o["W2"], sp, mut) for sp in range(n)]
    out["slabs"] = (np.stack([s[0] for s in sl]), np.stack([s[1] for s in sl]))
    if info is not None:
        info.extend(s[2] for s in sl)
    slabs = seen["slabs"] if seen else f32(out["slabs"][0])
    val, T = R.stage_slab_sum(xm, o["b2"], slabs, mut)
    out["x"] = (val, R.slab_sum_bound(val, T, n))
    return out


def sum_stages(o, seen=None, mut=None):
    """-> {"x": (val, bound), "qkv": (val, bound)}"""
    n = o["slabs"].shape[0]
    val, T = R.stage_slab_sum(o["x_mid"], o["b2"], o["slabs"], mut)
    out = {"x": (val, R.slab_sum_bound(val, T, n))}
    if o["Wqkv"] is not None:
        xw = seen["x"] if seen else R.round_once(val)
        out["qkv"] = R.stage_ln_proj(xw, o["gamma"], o["beta"], o["Wqkv"], o["bqkv"], mut=mut)[:2]
    return out


def vocab_stages(o, seen=None, mut=None):
    """-> {"x": (val, bound), "logits": (L, bound) with the row addend in, "plain": L without it}"""
    n = o["slabs"].shape[0]
    val, T = R.stage_slab_sum(o["x_mid"], o["b2"], o["slabs"], mut)
    out = {"x": (val, R.slab_sum_bound(val, T, n))}
    xw = seen["x"] if seen else R.round_once(val)
    L, bound, _ = R.stage_ln_proj(xw, o["gamma"], o["beta"], o["Wout"], None, mut=mut, out_bf16=False)
    out["plain"] = L
    out["logits"] = R.biased_logits(L, bound, o["row_bias"], o["row_bias_col"]) if o["row_bias"] is not None else (L, bound)
    return out


def ref_pairs(c, o, L, mut=None):
    """the `split` pairs of every row from the logits WITHOUT the addend -> (vals [B][split], cols [B][split])"""
    VC = o["VC"]
    pr = [R.pick(L, s * VC, (s + 1) * VC, o["skip_a"], o["skip_b"], o["row_bias"], c["row_bias_col"], mut) for s in range(c["split"])]
    return np.stack([p[0] for p in pr], 1), np.stack([p[1] for p in pr], 1)


def check_pairs(c, o, vals, cols, Lb, bound, folded=None):
    """every range's pair and the fold against check_pick -> (violations, worst value ratio)"""
    VC, bad, worst = o["VC"], [], 0.0
    for s in range(c["split"]):
        b, r = R.check_pick(vals[:, s], cols[:, s], Lb, bound, s * VC, (s + 1) * VC, o["skip_a"], o["skip_b"], o["tie_group"])
        bad += [f"range {s}: {m}" for m in b]
        worst = max(worst, r)
    fv, fc = folded if folded is not None else R.fold(vals, cols)
    b, r = R.check_pick(fv, fc, Lb, bound, 0, c["V"], o["skip_a"], o["skip_b"], o["tie_group"])
    return bad + [f"fold: {m}" for m in b], max(worst, r)
