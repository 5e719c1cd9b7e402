"""The three CIF kernels -- simulst_cif_integrate (csrc/scans.hip: cif_kernel), simulst_cif_alpha_head (cif_alpha_head_kernel) and
simulst_cif_stream_append (csrc/cif_decode.hip: cif_append_kernel) -- against plain fp64 references, at the edges where a slot fires.

The reference (`seq_cif`) is integrate-and-fire from its definition, one frame after the other in float64: an accumulated weight w,
a vector acc and a delay sum; while w + a >= beta it takes beta - w of the frame, emits a slot and goes on with the rest of the
frame; at the end the tail is emitted, rescaled by beta / w, iff w >= tail_thres.  Delays are sum weight * (s + 1) / beta and the
tail's delay is NOT rescaled (neither oracle.cif.cif_function nor the kernel rescales it).  A row reads its first src_len frames
and nothing else.  It shares no index arithmetic with the kernel's prefix-scan form or the oracle's scatter form;
test_reference_equals_oracle (CPU) ties it to the oracle on every case, test_reference_mutations_change_a_case (CPU) shows that
the cases can fail.

Every decision is exact by construction.  DYADIC cases: alpha = k / 64, beta in {1, 1/2, 1/4}, so every prefix sum up to S = 3000
is exact in fp32 in any summation order; cif_len, tail_w and alpha_sum are compared with ==, and the kernel's left / right weights
are exact.  NON-DYADIC cases (beta 0.8, 0.926, 0.3; S <= 110): a deterministic fp64 walk keeps every prefix 1e-3 away from a
multiple of beta and the tail 1e-3 away from tail_thres (asserted on the inputs, test_nondyadic_margins); the fp32 prefix-sum error
(S - 1) * 2^-24 * sum(alpha) <= 5e-4 (asserted too) stays inside, so the integers are compared exactly and no row is left out.
In every ragged case x and alpha hold NaN at frames >= src_len[b]: the outputs must be finite and those of the row alone.

Bounds, per element.  Dyadic fp32: the weights are exact and the kernel is one fma chain, so |got - ref| <= (n + 3) * 2^-23 *
sum |w||x| over the slot's n terms (the tail's beta / tail_w factor applies to the bound as to the value); delays the same over
w (s + 1) / beta with 2 n + 2.  bf16 adds 2^-8 |ref| for the one rounding at the store; the reference reads the bf16-rounded x.
Non-dyadic: the tolerances of test_cif_integrate_vs_oracle (out 1e-4 / 1e-3, delays 1e-3 / 1e-4, tail_w 1e-4 / 1e-3, alpha_sum
1e-4 / 1e-5), bf16 again + 2^-8 |ref| on out.  Each test prints the worst |got - ref| / bound so far for its class and dtype.

EXCLUDED: a total that is an exact multiple of beta at the last frame with tail_thres = 0 (an all-zero row included).  The tail
weight is 0 >= 0, reference, oracle and kernel all scale a zero vector by beta / 0 and return NaN; no caller reaches it with a
meaning (streaming withholds the tail slot, and a zero carry is asserted away in the streaming cases below).

Streaming (test_streaming_equals_one_shot): ops.cif_integrate + ops.cif_stream_append driven as CIFLayer.infer_batched drives them
must give, over chunks of 1, 2, 5, 64, 3 and 130 frames, the one-shot reference of the whole row: counts exact, fp32 within
1e-4 / 1e-3, bf16 within (2 c + 1) * 2^-8 * sum |w||x| for a slot that spans c chunk boundaries (the carried tail is rounded when
it is stored and again when it is divided by beta).  No prefix at a chunk end is a multiple of beta (asserted); mid-chunk hits stay.

Alpha head (test_alpha_head_vs_fp64): sigmoid(w . gelu_erf(LN(h)) + b) in fp64 from the inputs as the kernel reads them.  The bound
is measured, not fixed: e32 = the error of the same formula in torch fp32 on the CPU; |got - ref| <= 4 * e32_max + 2^-22 (4 for the
other summation order of the wave reductions).  The constant row holds 0.5, whose partial sums are exact in any order: variance 0
exactly, LN output = its bias.  (A non-dyadic constant's mean is off by an ulp in ANY fp32 sum and 1 / sqrt(eps) = 316 amplifies
that; this is a property of LayerNorm in fp32, not of a kernel.)  Rows aligned with +-sign(w) saturate the sigmoid on either side.
Measured on an MI355X: largest e32_max 5.1e-7 (rows 257, D 1024, bf16 inputs), worst |got - ref| / bound 0.47 (fp32, rows 1, D 80)
and 0.46 (bf16, rows 5, D 1024).  Integrate, worst |got - ref| / bound: dyadic fp32 out 0.200, delays exact; dyadic bf16 out 0.996
(the store's rounding alone); non-dyadic fp32 out 0.096, delays 0.152; non-dyadic bf16 out 0.763; streaming fp32 0.0004, bf16 0.996.
No derived bound had to be touched.  (`cif_function` row.)

Found by these cases and fixed: for the tail slot cif_kernel walked the frames up to S - 1, with weight 0 beyond src_len -- and
fmaf(0, NaN, acc) is NaN, so a ragged batch with non-finite padded encoder rows got a NaN tail slot (8 of the 13 `*_ragged` cases
below, those with a row shorter than S that emits a tail, failed in both dtypes on a non-finite out, the counts right).  The walk
now ends at min(src_len, S) - 1; frames at or beyond src_len are never read.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

U23 = 2.0 ** -23
BF16_STORE = 2.0 ** -8
MARGIN = 1e-3
E_SHAPE = -2
GUARD = 64
SENTINEL = 1234.0                      # exact in bf16
DTYPES = (torch.float32, torch.bfloat16)
MUTATIONS = ("fire_gt", "tail_gt", "drop_whole", "swap_lr", "len_plus1", "tail_noscale", "tail_delay_scaled")
WORST = {}


# ---- the reference --------------------------------------------------------------------------------------------------------------------
class _Slot:
    def __init__(self, Cc):
        self.acc, self.mag = np.zeros(Cc), np.zeros(Cc)
        self.d = self.dm = 0.0
        self.nt, self.f0 = 0, -1

    def add(self, wt, s, xs, axs, beta):
        if wt == 0.0:
            return
        self.acc += wt * xs
        self.mag += abs(wt) * axs
        self.d += wt * (s + 1) / beta
        self.dm += abs(wt) * (s + 1) / beta
        self.nt += 1
        if self.f0 < 0:
            self.f0 = s


def seq_cif(x, alpha, L, beta, tail_thres, mut=None):
    """x [S, C] float64, alpha [S] float64, the row's length L.  Returns n, out [n, C], mag [n, C] = sum |w||x|, nt [n] terms,
    delays [n], dmag [n], span [n, 2] (first and last frame of each slot), tail_w, alpha_sum and counts of the edges walked."""
    S, Cc = x.shape
    if mut == "len_plus1":
        L = min(L + 1, S)
    ax = np.abs(x)
    slots, sl = [], _Slot(Cc)
    stats = dict(hits=0, multi_clean=0, multi_carry=0, max_fires=0, zero_frames=0, first_fires=0)
    w = asum = 0.0
    for s in range(L):
        a = float(alpha[s])
        asum += a
        rem, fires, w_in, swapped = a, 0, w, 0.0
        while (w + rem > beta) if mut == "fire_gt" else (w + rem >= beta):
            take = beta - w
            wt = take
            if mut == "swap_lr" and fires == 0:        # the frame's right weight into the slot it closes
                rest = rem - take
                wt, swapped = rest - math.floor(rest / beta) * beta, take
            sl.add(wt, s, x[s], ax[s], beta)
            slots.append((sl, s))
            sl = _Slot(Cc)
            rem -= take
            w = 0.0
            fires += 1
            if mut == "drop_whole":
                while rem >= beta:
                    rem -= beta
        sl.add(swapped if (mut == "swap_lr" and fires) else rem, s, x[s], ax[s], beta)
        w += rem
        stats["zero_frames"] += a == 0.0
        stats["hits"] += fires > 0 and rem == 0.0 and s < L - 1
        stats["multi_clean"] += fires > 1 and w_in == 0.0
        stats["multi_carry"] += fires > 1 and w_in > 0.0
        stats["first_fires"] += s == 0 and fires > 0
        stats["max_fires"] = max(stats["max_fires"], fires)
    n_full = len(slots)
    if (w > tail_thres) if mut == "tail_gt" else (w >= tail_thres):
        sc = 1.0 if mut == "tail_noscale" else (beta / w if w != 0.0 else float("nan"))
        sl.acc, sl.mag, sl.nt = sl.acc * sc, sl.mag * sc, sl.nt + 1
        if mut == "tail_delay_scaled":
            sl.d *= beta / w if w != 0.0 else float("nan")
        slots.append((sl, L - 1))
    n = len(slots)
    return dict(n=n, n_full=n_full, tail_w=w, alpha_sum=asum, stats=stats,
                out=np.array([q.acc for q, _ in slots]).reshape(n, Cc), mag=np.array([q.mag for q, _ in slots]).reshape(n, Cc),
                nt=np.array([q.nt for q, _ in slots], dtype=np.float64), delays=np.array([q.d for q, _ in slots], dtype=np.float64),
                dmag=np.array([q.dm for q, _ in slots], dtype=np.float64),
                span=np.array([(q.f0 if q.f0 >= 0 else last, last) for q, last in slots], dtype=np.int64).reshape(n, 2))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _poison(x, alpha, lens):
    for b, L in enumerate(lens):
        x[b, L:] = np.nan
        alpha[b, L:] = np.nan


def _dyadic(B, S, Cc, beta, thres, lens=None, T_cap=None, seed=0, edits=(), tail=None):
    """alpha = k / 64.  edits, in frame order, applied to every row that is long enough: ("set", j, k), ("one", j) alpha = 1,
    ("zero", j, n) a run of n zeros, ("hit", j) frame j makes the prefix an exact multiple of beta with a nonzero weight.
    tail (one per row or one for all): the last frame is set so that the total leaves tail / 64 above a multiple of beta."""
    rng = np.random.default_rng(1000 + seed)
    q = int(round(64 * beta))
    k = rng.integers(0, 65, size=(B, S))
    L = list(lens) if lens is not None else [S] * B
    for b in range(B):
        for e in sorted(edits, key=lambda e: e[1]):
            j = e[1]
            if j >= L[b] - 1 and L[b] > 1:
                continue                                 # the last frame belongs to the tail rule
            if j >= L[b]:
                continue
            if e[0] == "set":
                k[b, j] = e[2]
            elif e[0] == "one":
                k[b, j] = 64
            elif e[0] == "zero":
                k[b, j:min(j + e[2], L[b] - 1)] = 0
            elif e[0] == "hit":
                v = int(-k[b, :j].sum()) % q
                k[b, j] = v if v > 0 else q
        if tail is not None:
            tw = tail[b] if isinstance(tail, (list, tuple)) else tail
            v = int(tw - k[b, :L[b] - 1].sum()) % q
            k[b, L[b] - 1] = v if v > 0 else q
    alpha = k.astype(np.float64) / 64.0
    x = rng.standard_normal((B, S, Cc)).astype(np.float32)
    if lens is not None:
        _poison(x, alpha, L)
    return dict(kind="dyadic", B=B, S=S, C=Cc, beta=beta, thres=thres, lens=lens, T_cap=T_cap, alpha=alpha, x=x)


def _nondyadic(B, S, Cc, beta, thres, lens, seed):
    """random alphas walked in fp64: while a prefix lies within MARGIN of a multiple of beta, 4e-3 is added to that frame; the same
    for the last frame while |tail - thres| < MARGIN; clamped to 1; then rounded to fp32, which is what kernel and reference read"""
    rng = np.random.default_rng(2000 + seed)
    alpha = rng.random((B, S))
    for b in range(B):
        p = 0.0
        for s in range(lens[b]):
            a = alpha[b, s]
            for _ in range(64):
                t = p + a
                near = abs(t - round(t / beta) * beta) < MARGIN
                if s == lens[b] - 1:
                    near = near or abs(t - math.floor(t / beta) * beta - thres) < MARGIN
                if not near:
                    break
                a += 4e-3
            alpha[b, s] = min(a, 1.0)
            p += alpha[b, s]
    alpha = alpha.astype(np.float32).astype(np.float64)
    x = rng.standard_normal((B, S, Cc)).astype(np.float32)
    _poison(x, alpha, lens)
    return dict(kind="nondyadic", B=B, S=S, C=Cc, beta=beta, thres=thres, lens=list(lens), T_cap=None, alpha=alpha, x=x)


def _mixed_lens(B, S, seed):
    r = np.random.default_rng(seed).integers(1, S + 1, size=B)
    return [S if b % 2 == 0 else int(r[b]) for b in range(B)]


# simulst_cif_integrate picks the slots per wave (spw; a workgroup covers 4 * spw slots) from T_cap and B:
#     spw = 16 if T_cap <= 512 else (32 if T_cap <= 1024 else 64)
#     while spw > 16 and B * ceil(T_cap / (4 * spw)) < 512: spw /= 2
# B = 104: T_cap 66 -> 16; T_cap 600 -> 32 (104 * 5 = 520 workgroups keeps it); T_cap 1100 -> 64 (104 * 5 = 520)
CASES = {
    # S = 1, 2: one frame that stays below beta, hits it, or whose tail sits on / one step below the threshold
    "s1_c4_b1": lambda: _dyadic(3, 1, 4, 1.0, 0.5, tail=[32, 31, 0], seed=1),
    "s2_c36_b05_first_fires": lambda: _dyadic(2, 2, 36, 0.5, 0.25, edits=[("set", 0, 48)], tail=[16, 15], seed=2),
    "s2_c4_below_beta_thres0": lambda: _dyadic(1, 2, 4, 1.0, 0.0, edits=[("set", 0, 10)], tail=30, seed=3),
    "s2_c4_below_beta_no_slot": lambda: _dyadic(1, 2, 4, 1.0, 0.5, edits=[("set", 0, 10)], tail=30, seed=4),
    # alpha = 1 at beta = 1/4: four fires, clean (after a hit) and with a remainder carried in
    "s63_c256_b025_ragged": lambda: _dyadic(2, 63, 256, 0.25, 0.125, lens=[63, 62],
                                            edits=[("hit", 10), ("one", 11), ("hit", 20), ("set", 21, 5), ("one", 22), ("zero", 40, 6)],
                                            tail=[8, 7], seed=5),
    "s64_c260_b1_ragged": lambda: _dyadic(3, 64, 260, 1.0, 0.5, lens=[64, 63, 32],
                                          edits=[("hit", 5), ("zero", 6, 4), ("hit", 40), ("zero", 55, 5)], tail=[32, 31, 0], seed=6),
    "s65_c512_b05_ragged": lambda: _dyadic(2, 65, 512, 0.5, 0.25, lens=[65, 1], edits=[("set", 0, 64), ("hit", 62), ("hit", 63)],
                                           tail=[0, 16], seed=7),
    "s128_c36_b025_thres0": lambda: _dyadic(3, 128, 36, 0.25, 0.0,
                                            edits=[("one", 0), ("hit", 50), ("one", 51), ("set", 70, 3), ("one", 71), ("zero", 100, 20)],
                                            tail=[5, 1, 15], seed=8),
    "s129_c4_b1_ragged": lambda: _dyadic(2, 129, 4, 1.0, 0.5, lens=[129, 128], edits=[("zero", 0, 3), ("hit", 63), ("hit", 64), ("hit", 126)],
                                         tail=[0, 32], seed=9),
    "s257_c512_b05_ragged": lambda: _dyadic(3, 257, 512, 0.5, 0.25, lens=[257, 256, 128],
                                            edits=[("hit", 64), ("zero", 65, 64), ("hit", 192), ("one", 193)], tail=[16, 15, 0], seed=10),
    "s3000_c36_b1_ragged": lambda: _dyadic(2, 3000, 36, 1.0, 0.5, lens=[3000, 1500],
                                           edits=[("hit", 1000), ("zero", 1001, 200), ("hit", 2047), ("hit", 2048)], tail=[0, 32], seed=11),
    "s130_c260_b1_full_len": lambda: _dyadic(2, 130, 260, 1.0, 0.5, lens=[130, 130], edits=[("hit", 64)], tail=[33, 0], seed=12),
    # the host's three spw classes
    "spw16_b104_ragged": lambda: _dyadic(104, 64, 8, 1.0, 0.5, lens=_mixed_lens(104, 64, 31), edits=[("hit", 7)], seed=13),
    "spw32_b104_tcap600_ragged": lambda: _dyadic(104, 64, 8, 0.25, 0.125, lens=_mixed_lens(104, 64, 32), T_cap=600,
                                                 edits=[("hit", 7), ("one", 8)], seed=14),
    "spw64_b104_tcap1100_ragged": lambda: _dyadic(104, 64, 8, 0.25, 0.0, lens=_mixed_lens(104, 64, 33), T_cap=1100,
                                                  edits=[("hit", 7), ("one", 8)], tail=5, seed=15),
    # non-dyadic
    "nd_s110_c64_b08_ragged": lambda: _nondyadic(3, 110, 64, 0.8, 0.4, [110, 105, 65], 1),
    "nd_s70_c40_b03_ragged": lambda: _nondyadic(2, 70, 40, 0.3, 0.15, [70, 35], 2),
    "nd_s37_c36_b0926_ragged": lambda: _nondyadic(3, 37, 36, 0.926, 0.463, [37, 36, 1], 3),
    "nd_s100_c260_b03_thres0_ragged": lambda: _nondyadic(2, 100, 260, 0.3, 0.0, [100, 64], 4),
}
NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def _x64(c, bf16):
    x = torch.from_numpy(c["x"])
    return (x.to(torch.bfloat16) if bf16 else x).double().numpy()


def _lens(c):
    return c["lens"] if c["lens"] is not None else [c["S"]] * c["B"]


@functools.lru_cache(maxsize=None)
def refs(name, bf16=False, mut=None):
    """the reference of every row, computed once per (case, dtype) and shared by the tests"""
    c = case(name)
    x = _x64(c, bf16)
    with np.errstate(all="ignore"):
        return tuple(seq_cif(x[b], c["alpha"][b], L, c["beta"], c["thres"], mut) for b, L in enumerate(_lens(c)))


def _bounds(c, r, bf16):
    if c["kind"] == "dyadic":
        bo = (r["nt"][:, None] + 3) * U23 * r["mag"]
        bd = (2 * r["nt"] + 2) * U23 * r["dmag"]
    else:
        bo = 1e-4 + 1e-3 * np.abs(r["out"])
        bd = 1e-3 + 1e-4 * np.abs(r["delays"])
    if bf16:
        bo = bo + BF16_STORE * np.abs(r["out"])
    return bo, bd


def _ratio(got, ref, bound):
    """max |got - ref| / bound; inf where got is not finite or differs at a zero bound"""
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(got, dtype=np.float64) - ref)
        q = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d == 0, 0.0, np.inf))
    q = np.where(np.isfinite(d), q, np.inf)
    return float(q.max()) if q.size else 0.0


def _compare(c, r, n, out, delays, tw, asum, bf16, key, what, rows=None):
    """one row against its reference r; out [>= rows, C], delays [>= rows]"""
    assert n == r["n"], (what, "cif_len", n, r["n"])
    if c["kind"] == "dyadic":
        assert tw == r["tail_w"] and asum == r["alpha_sum"], (what, tw, r["tail_w"], asum, r["alpha_sum"])
    else:
        assert abs(tw - r["tail_w"]) <= 1e-4 + 1e-3 * abs(r["tail_w"]), (what, tw, r["tail_w"])
        assert abs(asum - r["alpha_sum"]) <= 1e-4 + 1e-5 * abs(r["alpha_sum"]), (what, asum, r["alpha_sum"])
    rows = n if rows is None else rows
    bo, bd = _bounds(c, r, bf16)
    ro = _ratio(out[:rows], r["out"][:rows], bo[:rows])
    rd = _ratio(delays[:rows], r["delays"][:rows], bd[:rows])
    w = WORST.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], ro), max(w[1], rd)
    assert ro <= 1.0, (what, "out: |got - ref| / bound", ro)
    assert rd <= 1.0, (what, "delays: |got - ref| / bound", rd)


def _report(key):
    w = WORST.get(key, [0.0, 0.0])
    print(f"worst |got - ref| / bound so far, {' '.join(key)}: out {w[0]:.4f} delays {w[1]:.4f}")


# ---- CPU: the cases and the reference ---------------------------------------------------------------------------------------------------
def test_nondyadic_margins():
    """every prefix of a non-dyadic row is MARGIN away from a multiple of beta and its tail MARGIN away from tail_thres, so an fp32
    prefix sum in any order takes the same decisions as fp64"""
    for name in NAMES:
        c = case(name)
        if c["kind"] != "nondyadic":
            continue
        worst = np.inf
        for b, L in enumerate(_lens(c)):
            p = np.cumsum(c["alpha"][b, :L])
            m = np.abs(p - np.round(p / c["beta"]) * c["beta"]).min()
            t = abs(p[-1] - math.floor(p[-1] / c["beta"]) * c["beta"] - c["thres"])
            worst = min(worst, m, t)
            assert (L - 1) * 2.0 ** -24 * p[-1] <= MARGIN / 2
            assert c["alpha"][b, :L].max() <= 1.0
        print(f"{name}: margin {worst:.2e}")
        assert worst >= MARGIN, (name, worst)


def test_dyadic_cases_cover_the_edges():
    """the edges the cases were written for are walked by the reference (counts over all dyadic rows)"""
    tot = dict(hits=0, multi_clean=0, multi_carry=0, zero_frames=0, first_fires=0, max_fires=0, below_beta=0, tail_on_thres=0,
               tail_under_thres=0, exact_end_no_tail=0, no_slot=0)
    for name in NAMES:
        c = case(name)
        if c["kind"] != "dyadic":
            continue
        assert np.array_equal(np.nan_to_num(c["alpha"]) * 64, np.round(np.nan_to_num(c["alpha"]) * 64))
        for r in refs(name):
            for k_ in ("hits", "multi_clean", "multi_carry", "zero_frames", "first_fires"):
                tot[k_] += r["stats"][k_]
            tot["max_fires"] = max(tot["max_fires"], r["stats"]["max_fires"])
            tot["below_beta"] += r["n_full"] == 0
            tot["no_slot"] += r["n"] == 0
            tot["tail_on_thres"] += c["thres"] > 0 and r["tail_w"] == c["thres"] and r["n"] == r["n_full"] + 1
            tot["tail_under_thres"] += r["tail_w"] == c["thres"] - 1 / 64 and r["n"] == r["n_full"]
            tot["exact_end_no_tail"] += r["tail_w"] == 0 and r["n_full"] > 0 and r["n"] == r["n_full"]
            assert not (c["thres"] == 0 and r["tail_w"] == 0), (name, "the excluded case")
    print(tot)
    assert tot["max_fires"] == 4 and all(v > 0 for v in tot.values()), tot


def test_reference_equals_oracle():
    """the sequential reference and oracle.cif.cif_function (fp32, scatter form) on every row of every case: integers exact,
    values within the fp32 bounds of the class -- the two restatements hold each other"""
    from oracle import cif as ocif
    for name in NAMES:
        c = case(name)
        for b, L in enumerate(_lens(c)):
            r = refs(name)[b]
            o = ocif.cif_function(torch.from_numpy(c["x"][b:b + 1, :L]), torch.from_numpy(c["alpha"][b:b + 1, :L]).float(),
                                  beta=c["beta"], tail_thres=c["thres"])
            _compare(c, r, int(o["cif_lengths"][0][0]), o["cif_out"][0][0].double().numpy(), o["delays"][0][0].double().numpy(),
                     float(o["tail_weights"][0][0]), float(o["alpha_sum"][0][0]), False, ("oracle", c["kind"]), (name, b))
    _report(("oracle", "dyadic"))
    _report(("oracle", "nondyadic"))


def _differs(c, r, m):
    """does the mutated reference m of a row differ from r in an integer, or in a value by more than 10 x its bound?"""
    same = lambda a, b: a == b or (a != a and b != b)
    if not (same(m["n"], r["n"]) and same(m["tail_w"], r["tail_w"]) and same(m["alpha_sum"], r["alpha_sum"])):
        return True
    bo, bd = _bounds(c, r, False)
    return _ratio(m["out"], r["out"], bo) > 10 or _ratio(m["delays"], r["delays"], bd) > 10


def test_reference_mutations_change_a_case():
    """each one-off mistake, applied to the reference, changes cif_len / tail_w / alpha_sum or moves an output by more than 10 x its
    bound in at least one case.  Cases out of 19 that notice (fp32 inputs): fire on > 9, tail on > 10, whole slots dropped 10,
    left and right weights swapped 17, src_len + 1 13 (every ragged case: the poisoned frame), tail not rescaled 16, tail delay
    rescaled 16."""
    counts = {}
    for mut in MUTATIONS:
        counts[mut] = sum(any(_differs(case(name), r, m) for r, m in zip(refs(name), refs(name, False, mut))) for name in NAMES)
    print(counts, "of", len(NAMES))
    assert all(v > 0 for v in counts.values()), counts


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


def _device_inputs(c, dtype):
    x = torch.from_numpy(c["x"]).to(dtype).cuda()
    al = torch.from_numpy(c["alpha"]).float().cuda()
    lens = torch.tensor(c["lens"], dtype=torch.int32).cuda() if c["lens"] is not None else None
    return x, al, lens


def _check_integrate(c, name, dtype, res, T_cap=None):
    out, n, delays, tw, asum = (t.cpu() for t in res)
    bf16 = dtype == torch.bfloat16
    key = ("integrate", c["kind"], "bf16" if bf16 else "fp32")
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(delays).all()), (name, "non-finite output")
    T = out.shape[1]
    for b, r in enumerate(refs(name, bf16)):
        rows = min(r["n"], T)
        _compare(c, r, int(n[b]), out[b].double().numpy(), delays[b].double().numpy(), float(tw[b]), float(asum[b]), bf16, key,
                 (name, b), rows)
        if rows < T:                                              # zero beyond cif_len, in every workgroup's slot range
            assert float(out[b, rows:].float().abs().max()) == 0.0, (name, b, "slots beyond cif_len")
            assert float(delays[b, rows:].abs().max()) == 0.0, (name, b, "delays beyond cif_len")
    _report(key)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("name", NAMES)
def test_integrate_vs_sequential_fp64(ops, name, dtype):
    c = case(name)
    x, al, lens = _device_inputs(c, dtype)
    res = ops.cif_integrate(x, al, beta=c["beta"], tail_thres=c["thres"], src_len=lens, T_cap=c["T_cap"])
    torch.cuda.synchronize()
    _check_integrate(c, name, dtype, res)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_integrate_same_bits_every_run(ops, dtype):
    c = case("s257_c512_b05_ragged")
    x, al, lens = _device_inputs(c, dtype)
    runs = [ops.cif_integrate(x, al, beta=c["beta"], tail_thres=c["thres"], src_len=lens) for _ in range(3)]
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.uint8)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(bits(a), bits(b))


def _guarded(shape, dtype):
    """a SENTINEL-filled buffer with GUARD elements on either side of the returned view"""
    n = int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, device="cuda", dtype=dtype)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("short", [0, 1])
@pytest.mark.parametrize("name", ["s64_c260_b1_ragged", "s128_c36_b025_thres0"])
def test_integrate_capacity(ops, name, short, dtype):
    """T_cap == the largest cif_len of the batch: everything right; one less (the slot that does not fit is a fired one in the
    first case, the tail in the second): the slots below T_cap right, nothing written outside out and delays, and cif_len still the
    true count, which is how a caller detects the overflow"""
    from simulst_amd.ops import dt
    c = case(name)
    x, al, lens = _device_inputs(c, dtype)
    B, Cc = c["B"], c["C"]
    T_cap = max(r["n"] for r in refs(name)) - short
    obuf, out = _guarded((B, T_cap, Cc), dtype)
    dbuf, delays = _guarded((B, T_cap), torch.float32)
    n = torch.full((B,), -1, device="cuda", dtype=torch.int32)
    tw, asum = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    ops.h.check(ops.lib.simulst_cif_integrate(ops.h.ptr, vp(x), vp(al), vp(lens), vp(out), vp(n), vp(delays), vp(tw), vp(asum), B, c["S"],
                                              Cc, T_cap, c["beta"], c["thres"], dt(x)), "simulst_cif_integrate")
    torch.cuda.synchronize()
    assert _guards_intact(obuf) and _guards_intact(dbuf)
    if short:
        assert int(n.max()) == T_cap + 1
    _check_integrate(c, name, dtype, (out, n, delays, tw, asum))


@pytest.mark.gpu
def test_integrate_refusals(ops):
    """C % 4 != 0, beta <= 0 and more than 64 KB of LDS (4 S + T_cap + 1 floats): E_SHAPE, nothing launched"""
    from simulst_amd import _lib
    t = torch.zeros(64, device="cuda")
    i = torch.full((4,), 7, device="cuda", dtype=torch.int32)
    vp = lambda z: C.c_void_p(z.data_ptr())

    def rc(S, Cc, T_cap, beta):
        return ops.lib.simulst_cif_integrate(ops.h.ptr, vp(t), vp(t), None, vp(t), vp(i), vp(t), vp(t), vp(t), 1, S, Cc, T_cap, beta, 0.5,
                                             _lib.F32)
    assert rc(4, 6, 4, 1.0) == E_SHAPE
    assert rc(4, 4, 4, 0.0) == E_SHAPE and rc(4, 4, 4, -1.0) == E_SHAPE
    assert rc(3000, 4, 4384, 1.0) == E_SHAPE                      # 12000 + 4384 + 1 = 16385 floats
    torch.cuda.synchronize()
    assert bool((i == 7).all()) and bool((t == 0).all())


# ---- streaming == one shot ----------------------------------------------------------------------------------------------------------------
CHUNKS = (5, 1, 64, 2, 130, 3, 1, 64, 2, 5)


@functools.lru_cache(maxsize=None)
def stream_case(beta, bf16):
    B, Cc, S = 3, 36, sum(CHUNKS)
    rng = np.random.default_rng(3000 + int(beta * 4))
    q = int(round(64 * beta))
    k = rng.integers(0, 65, size=(B, S))
    ends = np.cumsum(CHUNKS)
    for b in range(B):
        k[b, 0] = 7 + b
        for j in (30, 100, 101, 250):                             # mid-chunk exact hits stay
            v = int(-k[b, :j].sum()) % q
            k[b, j] = v if v > 0 else q
        for e in ends:                                            # no chunk ends on a multiple of beta: the carry is never empty
            if k[b, :e].sum() % q == 0:
                k[b, e - 1] += 1 if k[b, e - 1] < 64 else -1
    alpha = k / 64.0
    x = rng.standard_normal((B, S, Cc)).astype(np.float32)
    c = dict(kind="dyadic", B=B, S=S, C=Cc, beta=beta, thres=beta / 2, lens=None, T_cap=None, alpha=alpha, x=x)
    x64 = _x64(c, bf16)
    return c, ends, tuple(seq_cif(x64[b], alpha[b], S, beta, beta / 2) for b in range(B))


def _stream(ops, c, dtype, acc):
    """CIFLayer.infer_batched without the weight head: the first chunk plain, later chunks with the carried pseudo-frame in front,
    tail_thres 0 until the last chunk and beta / 2 there"""
    B, Cc, beta = c["B"], c["C"], c["beta"]
    x, al, _ = _device_inputs(c, dtype)
    prev_feat = torch.zeros(B, 1, Cc, device="cuda", dtype=dtype)
    prev_w = torch.zeros(B, 1, device="cuda")
    acc_len = torch.zeros(B, device="cuda", dtype=torch.int32)
    lo = 0
    for i, n_fr in enumerate(CHUNKS):
        xc, ac = x[:, lo:lo + n_fr], al[:, lo:lo + n_fr]
        if i > 0:
            xc, ac = torch.cat([prev_feat, xc], dim=1), torch.cat([prev_w, ac], dim=1)
        finish = i == len(CHUNKS) - 1
        out, n, _, tw, _ = ops.cif_integrate(xc.contiguous(), ac.contiguous(), beta=beta, tail_thres=beta / 2 if finish else 0.0)
        ops.cif_stream_append(out, n, tw, acc, acc_len, prev_feat, prev_w, beta=beta, finish=finish)
        lo += n_fr
    torch.cuda.synchronize()
    return acc_len.cpu()


def _stream_bound(c, ends, r, bf16):
    if not bf16:
        return 1e-4 + 1e-3 * np.abs(r["out"])
    crossed = np.array([sum(1 for e in ends[:-1] if f0 < e <= f1) for f0, f1 in r["span"]], dtype=np.float64)
    return (2 * crossed[:, None] + 1) * BF16_STORE * r["mag"]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("beta", [1.0, 0.5])
def test_streaming_equals_one_shot(ops, beta, dtype):
    bf16 = dtype == torch.bfloat16
    c, ends, ref = stream_case(beta, bf16)
    q = int(round(64 * beta))
    k = np.round(c["alpha"] * 64).astype(np.int64)
    assert all(k[b, :e].sum() % q != 0 for b in range(c["B"]) for e in ends), "a chunk ends on a multiple of beta"
    assert sum(r["stats"]["hits"] for r in ref) >= 3 * c["B"]
    n_cap = max(r["n"] for r in ref) + 2
    abuf, acc = _guarded((c["B"], n_cap, c["C"]), dtype)
    acc.zero_()
    acc_len = _stream(ops, c, dtype, acc)
    assert _guards_intact(abuf)
    key = ("stream", "dyadic", "bf16" if bf16 else "fp32")
    w = WORST.setdefault(key, [0.0, 0.0])
    for b, r in enumerate(ref):
        assert int(acc_len[b]) == r["n"], (b, int(acc_len[b]), r["n"])
        ro = _ratio(acc[b, :r["n"]].double().cpu().numpy(), r["out"], _stream_bound(c, ends, r, bf16))
        w[0] = max(w[0], ro)
        assert ro <= 1.0, (b, "acc: |got - ref| / bound", ro)
        assert float(acc[b, r["n"]:].float().abs().max()) == 0.0
    _report(key)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_streaming_stops_at_n_cap(ops, dtype):
    """n_cap below the rows' counts: every row stops at n_cap with acc_len == n_cap, holds its own first n_cap vectors (so no row
    wrote into the next one) and the buffer's guards are intact"""
    bf16 = dtype == torch.bfloat16
    c, ends, ref = stream_case(1.0, bf16)
    n_cap = min(r["n"] for r in ref) // 2
    assert n_cap >= 8
    abuf, acc = _guarded((c["B"], n_cap, c["C"]), dtype)
    acc.zero_()
    acc_len = _stream(ops, c, dtype, acc)
    assert _guards_intact(abuf)
    for b, r in enumerate(ref):
        assert int(acc_len[b]) == n_cap
        assert _ratio(acc[b].double().cpu().numpy(), r["out"][:n_cap], _stream_bound(c, ends, r, bf16)[:n_cap]) <= 1.0, b


# ---- the weight head ----------------------------------------------------------------------------------------------------------------------
def _head_formula(h, g, bt, w, bias):
    mu = h.mean(-1, keepdim=True)
    var = ((h - mu) ** 2).mean(-1, keepdim=True)
    v = (h - mu) / torch.sqrt(var + 1e-5) * g + bt
    gelu = 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    return torch.sigmoid((gelu * w).sum(-1) + bias)


@functools.lru_cache(maxsize=None)
def head_case(rows, D, bf16):
    g_ = torch.Generator().manual_seed(4000 + 7 * rows + D)
    w = torch.randn(D, generator=g_) * (8.0 / math.sqrt(D))
    gam = 0.8 + 0.4 * torch.rand(D, generator=g_)
    bt = 0.1 * torch.randn(D, generator=g_)
    # random rows are drawn four to one and those with the smallest |logit| kept: w is large enough for the aligned rows below to
    # saturate, which spreads random logits over +-4, and an error in the logit shows only where the sigmoid has a slope
    cand = torch.randn(4 * rows, D, generator=g_) * 1.5 + 0.3
    z = _head_formula(cand.double(), gam.double(), bt.double(), w.double(), 0.1)
    h = cand[torch.sort((z - 0.5).abs()).indices[:rows]].clone()
    if rows >= 3:
        h[0] = 0.5                                                # variance 0, every partial sum exact
        h[1] = torch.sign(w)                                      # logit far above 0
        h[2] = -torch.sign(w)                                     # logit far below 0
    if bf16:
        h, w = h.to(torch.bfloat16).float(), w.to(torch.bfloat16).float()
    bias = 0.1
    ref = _head_formula(h.double(), gam.double(), bt.double(), w.double(), bias)
    e32 = float((_head_formula(h, gam, bt, w, bias).double() - ref).abs().max())
    return h, w, gam, bt, bias, ref, e32


def test_alpha_head_cases_saturate():
    """rows 1 and 2 of every case with >= 3 rows sit where fp32 rounds the sigmoid to 1 and below 2^-25; the constant row and,
    where there is one, some random row sit where the sigmoid has a slope"""
    for bf16 in (False, True):
        for rows in (1, 3, 4, 5, 257):
            for D in (64, 80, 256, 1024):
                ref = head_case(rows, D, bf16)[5]
                if rows >= 3:
                    assert float(ref[1]) > 1 - 2.0 ** -25 and float(ref[2]) < 2.0 ** -25, (rows, D, float(ref[1]), float(ref[2]))
                    assert 0.02 < float(ref[0]) < 0.98
                if rows != 3:
                    assert bool(((ref[3 if rows >= 3 else 0:] > 0.02) & (ref[3 if rows >= 3 else 0:] < 0.98)).any()), (rows, D)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("D", [64, 80, 256, 1024])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 257])
def test_alpha_head_vs_fp64(ops, rows, D, dtype):
    bf16 = dtype == torch.bfloat16
    h, w, gam, bt, bias, ref, e32 = head_case(rows, D, bf16)
    got = ops.cif_alpha_head(h.to(dtype).cuda(), gam.cuda(), bt.cuda(), w.to(dtype).cuda(), bias)
    torch.cuda.synchronize()
    err = float((got.cpu().double() - ref).abs().max())
    bound = 4 * e32 + 2.0 ** -22
    key = ("alpha_head", "bf16" if bf16 else "fp32")
    w_ = WORST.setdefault(key, [0.0, 0.0])
    w_[0], w_[1] = max(w_[0], err / bound), max(w_[1], e32)
    print(f"rows {rows} D {D} {key[1]}: |got - ref| {err:.3e}, e32_max {e32:.3e}, ratio {err / bound:.4f}; worst ratio so far "
          f"{w_[0]:.4f}, largest e32_max so far {w_[1]:.3e}")
    assert bool(torch.isfinite(got).all()) and err <= bound, (err, bound)
