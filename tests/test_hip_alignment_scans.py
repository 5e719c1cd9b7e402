"""The training-mode alignment chain of csrc/scans.hip -- simulst_expected_alignment (five kernel classes by source length),
simulst_expected_alignment_backward, simulst_mass_preservation, simulst_expected_soft_attention (infinite lookback and chunkwise) --
against the fp64 reference tests/alignment_ref.py, at the edges of the kernels: chunk and lane-group boundaries, the prefetch and
double-buffer tails, row pairs, ragged key lengths, the LDS limits and the refusals one past them.

CPU part (unmarked): the fp64 reference agrees with oracle/monotonic.py and the g9_alignment fixture; every GPU case can SEE the bugs
it is there for (each applicable mutant of the reference is more than 10 x the tolerance away on an element the GPU test compares);
the alignment front of each case's full-length row crosses every 64-wide chunk of the source.
GPU part (pytest.mark.gpu): the kernels against the same cached references, at the project's tolerances."""
import functools
import os

import pytest
import torch

import alignment_ref as ar
from conftest import load_golden

ATOL_A, RTOL_A = 1e-5, 1e-3           # alpha: the project's tolerance for the expected alignment
ATOL_B, RTOL_B = 1e-5, 1e-4           # beta and the mass-preserved position
GRAD_BOUND = 2e-4                     # gradient error over the bh row's largest reference gradient
MUTANT_FACTOR = 10.0                  # a mutant must be this many tolerances away
COVER = 100 * ATOL_A                  # an alpha this large in every 64-wide chunk of the full-length row
EPS = 1e-6
COARSE_EPS = 0.05                     # `coarse` family: an eps large enough that the prepended (1 + eps) shows at rtol 1e-3
EDGES = (0, 31, 32, 63, 64, 255, 256, 511, 512)


def _seed(*ints):
    s = 1234567
    for v in ints:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _key_len(BH, S, g):
    kl = torch.randint(1, S + 1, (BH,), generator=g, dtype=torch.int32)
    kl[0] = S
    if BH > 1:
        kl[1] = 1
    return kl


def _tol_ratio(got, ref, atol, rtol):
    """elementwise |got - ref| / (atol + rtol |ref|); NaN / inf count as infinitely far"""
    ref = ref.double()
    r = (got.double() - ref).abs() / (atol + rtol * ref.abs())
    return torch.nan_to_num(r, nan=float("inf"), posinf=float("inf"))


def _valid(kl, BH, U, S):
    if kl is None:
        return torch.ones(BH, U, S, dtype=torch.bool)
    BH = kl.numel()
    return (torch.arange(S).view(1, 1, S) < kl.long().view(BH, 1, 1)).expand(BH, U, S)


# ===================================================================================================== expected alignment: the cases
# (kernel class, S, U, BH): a subset of the product that meets every S, U and BH of the class at least once.  U walks the prefetch
# groups of EA_PF = 4 (1..4 inside the first group, 5 / 7 a guarded tail, 8 two groups, 9 / 11 the full-group loop plus a tail) and the
# double buffer of the wide kernels; BH walks row pairs and the 4-waves-per-block edge.
EA_CASES = {
    "small_half": [(1, 1, 1), (1, 5, 9), (1, 11, 37), (31, 2, 7), (31, 7, 8), (31, 9, 37),
                   (32, 3, 8), (32, 4, 9), (32, 8, 37), (32, 11, 7)],
    "small_full": [(33, 1, 1), (33, 5, 9), (33, 9, 37), (63, 2, 7), (63, 7, 8), (63, 11, 37),
                   (64, 3, 8), (64, 4, 9), (64, 8, 37)],
    "wide4": [(65, 1, 3), (65, 3, 5), (255, 2, 4), (255, 4, 5), (256, 3, 3), (256, 4, 4)],
    "wide8": [(257, 1, 3), (257, 4, 5), (511, 2, 4), (511, 3, 5), (512, 4, 5), (512, 1, 3)],
    # the general kernel at the sizes it is dispatched for; U is raised with S so that each target's alpha stays above COVER
    "general": [(513, 5, 5), (577, 6, 5), (1024, 8, 5), (4096, 16, 5)],
}
EA_FAMILIES = ("spread", "spread_nolen", "sigmoid", "saturating", "staircase", "coarse")


def ea_families(S):
    """the families that fit a source length: with the coarse eps the padded tail of a row multiplies c by (1 + eps) per position,
    which leaves fp32 (in the oracle and in the kernels alike) beyond about 1800 positions"""
    return [f for f in EA_FAMILIES if f != "coarse" or S <= 1024]


def _spread_p(BH, U, S, kl, g, pmax=1.0, spike=1.0):
    """the alignment front crosses the whole source in U targets.  From p = U(0, 1) * 2 U / key_len, adjusted until the coverage and
    mutant conditions hold:
      * target i keeps 2 % of that rate below position i * key_len / U, where its front starts.  A uniform rate cannot carry mass
        along a long source: c = cumprod(1 - p) falls under eps after sum(p) = 14, and the recurrence loses what lies beyond;
        below that rate the fronts are wider than 1 / COVER positions.
      * from four front widths past its start on, where a target has placed all but e^-4 of its mass, p is 0.98: c steps across eps by
        factors of 50 and does not creep through the 1 % band around it in which the backward test has to drop a row.
      * the last valid position stops at least half of what reaches it, so the one-position tail chunk of S = 64 k + 1 holds mass.
      * spike > 1 (soft-attention inputs): every 16th position has `spike` times the rate.  A single target over 2048 positions has
        a mean alpha of 1 / 2048, under COVER; its chunks reach COVER at the spikes."""
    klf = (kl.double() if kl is not None else torch.full((BH,), float(S), dtype=torch.float64)).view(BH, 1, 1)
    s, i = torch.arange(S, dtype=torch.float64).view(1, 1, S), torch.arange(U, dtype=torch.float64).view(1, U, 1)
    p = torch.rand(BH, U, S, generator=g, dtype=torch.float64) * 2 * U / klf
    p = torch.where(s % 16 == 5, spike * p, p)
    p = torch.where(s < i * klf / U, 0.02 * p, p)
    p = torch.where(s >= (i + 4) * klf / U, torch.full((), 0.98, dtype=torch.float64), p)
    p = torch.where(s == klf - 1, p.clamp(min=0.5), p)
    return p.clamp(0.0, pmax).float()


def _edges(S):
    return sorted({e for e in EDGES + (S - 1,) if e < S})


def _staircase_steps(BH, U, S):
    """-> per row U non-decreasing steps out of the chunk and lane-group edges below S.  The BH rows of the case (ragged lengths: a
    step at or beyond key_len is masked away) rotate through the list, row 0 (full length) from S - 1 down in strides, so that its
    steps lie in different chunks whenever S has more than one.  Full-length rows are appended that take the edges in order, U at a
    time (the last one repeated to fill a row): every edge below S is a VALID step of some row, whatever the lengths drawn."""
    edges = _edges(S)
    n, stride = len(edges), -(-len(edges) // U)
    rows = [sorted(edges[(n - 1 - b - i * stride) % n] for i in range(U)) for b in range(BH)]
    rows += [(edges[j:j + U] + [edges[-1]] * U)[:U] for j in range(0, n, U)]
    return rows


def _staircase_key_len(BH, U, S, kl):
    extra = len(_staircase_steps(BH, U, S)) - BH
    return torch.cat([kl, torch.full((extra,), S, dtype=torch.int32)])


def _staircase_valid_steps(BH, U, S, kl):
    """the steps that land on valid positions, per row (kl: the lengths of all rows, appended ones included)"""
    return [[k for k in steps if k < int(kl[b])] for b, steps in enumerate(_staircase_steps(BH, U, S))]


def _staircase_changes_chunk(BH, U, S, kl):
    """some row makes a valid step into a later 64-wide chunk than the one its mass is in: the additive carry is live"""
    for steps in _staircase_valid_steps(BH, U, S, kl):
        at = 0
        for k in steps:
            if k // 64 > at // 64:
                return True
            at = k
    return False


@functools.lru_cache(maxsize=None)
def ea_inputs(S, U, BH, family):
    """-> (p fp32 [BH, U, S], key_len int32 [BH] or None, eps); the staircase family has a few more rows than BH (_staircase_steps)"""
    g = _seed(S, U, BH, EA_FAMILIES.index(family))
    kl = _key_len(BH, S, g)
    eps = EPS
    if family == "spread":
        p = _spread_p(BH, U, S, kl, g)
    elif family == "spread_nolen":
        p, kl = _spread_p(BH, U, S, None, g), None
    elif family == "sigmoid":
        p = torch.sigmoid(torch.randn(BH, U, S, generator=g) * 2)
    elif family == "coarse":
        # 0.05 <= p <= 0.9: p (1 + eps) stays under the upper clamp and well above atol, so the prepended (1 + eps) shows at position 0
        # of the first target even where that is the only element (S = U = BH = 1)
        p, eps = torch.sigmoid(torch.randn(BH, U, S, generator=g) * 2).clamp(0.05, 0.9), COARSE_EPS
    elif family == "saturating":
        # exact 0.0 at every 7th and exact 1.0 at every 11th position; the residue moves with the target, so that a target's exact
        # 1.0 (cumprod under eps from there on) lies BELOW mass the previous target left: the lower clamp acts on real mass
        p = torch.sigmoid(torch.randn(BH, U, S, generator=g) * 2)
        s, i = torch.arange(S).view(1, 1, S), torch.arange(U).view(1, U, 1)
        p = torch.where((s + 2 * i) % 7 == 3, torch.zeros(()), p)
        p = torch.where((s + 10 * i) % 11 == 10, torch.ones(()), p)
        if BH > 2:
            p[2] = 0.0
        if BH > 3:
            p[3] = 0.999
    elif family == "staircase":
        rows = _staircase_steps(BH, U, S)
        p, kl = torch.zeros(len(rows), U, S), _staircase_key_len(BH, U, S, kl)
        for b, steps in enumerate(rows):
            for i, k in enumerate(steps):
                p[b, i, k] = 1.0
    else:
        raise KeyError(family)
    return p, kl, eps


@functools.lru_cache(maxsize=None)
def ea_ref(S, U, BH, family, mutation=None):
    p, kl, eps = ea_inputs(S, U, BH, family)
    return ar.expected_alignment(p, kl, eps, mutation=mutation)


def ea_mutations(S, U, BH, family):
    """the mutations a case can show.
    carries: more than one 64-wide chunk, and mass beyond the first one -- the spread families by construction, the staircase for
      the additive carry only (its cumprod stays above 1, where the clamp hides the product carry); sigmoid-shaped p keeps the front
      inside the first chunk and shows neither.
    no_lead: changes c by 1 + eps, which cancels wherever eps < c < 1; it shows where the clamps act, at a tolerance of 1e-3 only with
      the coarse eps.
    no_lower_clamp: the cumprod has to fall under eps below mass of the previous target: the saturating and coarse families, from
      the second target on (the first target's predecessor is the one-hot at 0, where c = 1 + eps)."""
    m = []
    if S > 64 and family in ("spread", "spread_nolen"):
        m += ["drop_sum_carry", "drop_prod_carry"]
    if family == "staircase" and _staircase_changes_chunk(BH, U, S, ea_inputs(S, U, BH, family)[1]):
        m += ["drop_sum_carry"]
    if family == "coarse":
        m += ["no_lead"]
    if family in ("saturating", "coarse") and U > 1 and S > 2:
        m += ["no_lower_clamp"]
    return m


# ===================================================================================================== CPU part
def _oracle_alpha(p, kl, eps):
    from oracle import monotonic as omo
    BH, U, S = p.shape
    pad = None if kl is None else torch.arange(S).view(1, S) >= kl.long().view(BH, 1)
    return omo.expected_alignment_from_p_choose(p, pad, eps)


@pytest.mark.parametrize("cls", list(EA_CASES))
def test_reference_alignment_agrees_with_oracle(cls):
    """fp64 reference against the fp32 oracle (oracle/monotonic.py) on every case and family of the GPU tables, at the project's alpha
    tolerance; the staircase family also against the literal one-hot."""
    worst = 0.0
    for S, U, BH in EA_CASES[cls]:
        for fam in ea_families(S):
            p, kl, eps = ea_inputs(S, U, BH, fam)
            ref = ea_ref(S, U, BH, fam)
            v = _valid(kl, BH, U, S)
            r = float(_tol_ratio(_oracle_alpha(p, kl, eps), ref, ATOL_A, RTOL_A)[v].max())
            worst = max(worst, r)
            assert r <= 1.0, (cls, S, U, BH, fam, r)
            if fam == "staircase":
                onehot = torch.where(v, p, torch.zeros(())).double()
                # at the step c >= 1 and the running sum is 1: u >= 1 clamps to exactly 1; p = 0 gives exactly 0 elsewhere
                assert float((ref - onehot).abs().max()) <= 4 * EPS, (S, U, BH)
                hit = {k for steps in _staircase_valid_steps(BH, U, S, kl) for k in steps}
                assert hit == set(_edges(S)), (S, U, BH, sorted(set(_edges(S)) - hit))
    print(f"\n[alignment_ref vs oracle] {cls}: largest err/tol {worst:.4f}")


@pytest.mark.parametrize("cls", list(EA_CASES))
def test_alignment_cases_see_the_mutants(cls):
    """a condition on the inputs: every mutation a case can show moves some compared alpha by more than 10 x its tolerance"""
    for S, U, BH in EA_CASES[cls]:
        for fam in ea_families(S):
            p, kl, eps = ea_inputs(S, U, BH, fam)
            ref, v = ea_ref(S, U, BH, fam), _valid(kl, BH, U, S)
            for mut in ea_mutations(S, U, BH, fam):
                r = float(_tol_ratio(ea_ref(S, U, BH, fam, mut), ref, ATOL_A, RTOL_A)[v].max())
                assert r > MUTANT_FACTOR, (cls, S, U, BH, fam, mut, r)


def _chunk_cover(alpha_row):
    """alpha_row [U, S]: the smallest over the 64-wide chunks of the largest alpha in the chunk over all targets"""
    top = alpha_row.max(dim=0).values
    return min(float(c.max()) for c in top.split(64))


@pytest.mark.parametrize("cls", list(EA_CASES))
def test_alignment_front_crosses_every_chunk(cls):
    """in the full-length row (row 0) of the spread inputs, every 64-wide chunk of the source holds an alpha above 100 x atol for
    some target: mass, and so every carry, is live along the whole source"""
    for S, U, BH in EA_CASES[cls]:
        for fam in ("spread", "spread_nolen"):
            c = _chunk_cover(ea_ref(S, U, BH, fam)[0])
            assert c > COVER, (cls, S, U, BH, fam, c)


def test_reference_agrees_with_g9_fixture():
    """g9_alignment is recorded from the reference project: alignment, mass preservation, both soft attentions, with and without
    padding, and the extreme-p row"""
    a, _ = load_golden("g9_alignment")
    p, pm, e = a["p"], a["padmask"], a["energy"]
    klen = (~pm).sum(1).to(torch.int32)
    for tag, kl in (("nopad", None), ("pad", klen)):
        al = ar.expected_alignment(p, kl, 1e-6)
        assert float(_tol_ratio(a[f"alpha.{tag}"], al, ATOL_A, RTOL_A).max()) <= 1.0
        amp = ar.mass_preservation(a[f"alpha.{tag}"], kl)
        assert float(_tol_ratio(a[f"alpha_mp.{tag}"], amp, ATOL_B, RTOL_B).max()) <= 1.0
        for name, chunk in (("beta_il", None), ("beta_chunk3", 3)):
            b = ar.expected_soft_attention(a[f"alpha_mp.{tag}"], e, kl, chunk, 1e-6)
            assert float(_tol_ratio(a[f"{name}.{tag}"], b, ATOL_B, RTOL_B).max()) <= 1.0, (tag, name)
    ext = ar.expected_alignment(a["p_extreme"], None, 1e-6)
    assert float(_tol_ratio(a["alpha_extreme"], ext, ATOL_A, RTOL_A).max()) <= 1.0


# ----------------------------------------------------------------------------------------------------- mass preservation: the cases
# (S, U, BH, with key_len): BH * U is never a multiple of 4 (a partly filled last block).  Odd bh rows are scaled up (sum > 1, the
# residual clamps to 0), even ones keep the alignment's sum < 1.
MP_CASES = [(1, 1, 3, True), (1, 3, 3, False), (2, 3, 3, True), (2, 1, 5, False), (63, 3, 3, True), (63, 1, 5, False),
            (64, 1, 7, True), (64, 3, 3, False), (65, 3, 3, True), (65, 1, 5, False), (300, 3, 5, True), (300, 3, 3, False)]


@functools.lru_cache(maxsize=None)
def mp_inputs(S, U, BH, with_len):
    g = _seed(S, U, BH, int(with_len), 77)
    kl = _key_len(BH, S, g)
    # a front that stops short of the end of the source, so that the even rows keep a residual
    p = (_spread_p(BH, U, S, kl, g) * 0.5).float()
    alpha = ar.expected_alignment(p, kl, EPS)
    alpha[1::2] = (alpha[1::2] * 3.0 + 0.01).clamp(max=1.0)
    return alpha.float().contiguous(), (kl if with_len else None)


def mp_mutations(S, U, with_len):
    return ["keylen_of_row"] if (with_len and U > 1 and S > 1) else []


def test_mass_preservation_reference_and_mutants():
    from oracle import monotonic as omo
    saw_under = saw_over = False
    for S, U, BH, with_len in MP_CASES:
        alpha, kl = mp_inputs(S, U, BH, with_len)
        assert (BH * U) % 4 != 0 and _chunk_cover(alpha[0].double()) > COVER
        ref = ar.mass_preservation(alpha, kl)
        pad = None if kl is None else torch.arange(S).view(1, S) >= kl.long().view(BH, 1)
        orc = omo.mass_preservation(alpha, pad)
        assert float(_tol_ratio(orc, ref, ATOL_B, RTOL_B).max()) <= 1.0, (S, U, BH, with_len)
        sums = torch.where(_valid(kl, BH, U, S), alpha, torch.zeros(())).double().sum(-1)
        if kl is None:
            sums = alpha[..., :-1].double().sum(-1)
        saw_under |= bool((sums < 0.9).any())
        saw_over |= bool((sums > 1.1).any())
        for mut in mp_mutations(S, U, with_len):
            r = float(_tol_ratio(ar.mass_preservation(alpha, kl, mutation=mut), ref, ATOL_B, RTOL_B).max())
            assert r > MUTANT_FACTOR, (S, U, BH, mut, r)
    assert saw_under and saw_over


# ----------------------------------------------------------------------------------------------------- soft attention: the cases
# (S, U, BH, chunk, eps, energy scale, with key_len, atol, rtol).  alpha is the fp64 reference's mass-preserved spread alignment in
# fp32.  rows = BH * U is never a multiple of 4.  The bound is the project's atol 1e-5 / rtol 1e-4 unless the fp32 oracle's own error
# against fp64 exceeds a quarter of it; then it is 4 x the oracle's measured error, written at the case (one case needs it; the largest oracle error measured
# is 0.021 of the tolerance elsewhere).
SA_CASES = [
    (1, 1, 3, None, 1e-10, 3, True, ATOL_B, RTOL_B), (1, 3, 3, 1, 1e-6, 30, True, ATOL_B, RTOL_B),
    (1, 1, 5, 8, 1e-6, 3, False, ATOL_B, RTOL_B),
    (63, 3, 3, None, 1e-6, 3, True, ATOL_B, RTOL_B), (63, 1, 5, 3, 1e-10, 30, True, ATOL_B, RTOL_B),
    (63, 3, 3, 63, 1e-6, 3, True, ATOL_B, RTOL_B),
    (64, 3, 3, None, 1e-10, 30, True, ATOL_B, RTOL_B), (64, 1, 5, 64, 1e-6, 3, False, ATOL_B, RTOL_B),
    (64, 3, 3, 65, 1e-10, 3, True, ATOL_B, RTOL_B),
    (65, 3, 3, None, 1e-6, 30, True, ATOL_B, RTOL_B), (65, 3, 3, 64, 1e-10, 3, True, ATOL_B, RTOL_B),
    (65, 1, 5, 65, 1e-6, 3, True, ATOL_B, RTOL_B), (65, 3, 3, 72, 1e-6, 30, False, ATOL_B, RTOL_B),
    (128, 3, 3, None, 1e-10, 3, True, ATOL_B, RTOL_B), (128, 1, 5, 1, 1e-6, 30, True, ATOL_B, RTOL_B),
    (128, 3, 3, 128, 1e-6, 3, True, ATOL_B, RTOL_B),
    (129, 3, 3, None, 1e-6, 3, False, ATOL_B, RTOL_B), (129, 3, 3, 65, 1e-10, 30, True, ATOL_B, RTOL_B),
    (129, 1, 5, 136, 1e-6, 3, True, ATOL_B, RTOL_B),
    (300, 3, 3, None, 1e-10, 30, True, ATOL_B, RTOL_B), (300, 3, 3, None, 1e-6, 3, True, ATOL_B, RTOL_B),
    (300, 3, 3, 3, 1e-6, 30, True, ATOL_B, RTOL_B), (300, 1, 5, 64, 1e-10, 3, True, ATOL_B, RTOL_B),
    (300, 3, 3, 300, 1e-6, 3, False, ATOL_B, RTOL_B), (300, 3, 3, 307, 1e-6, 30, True, ATOL_B, RTOL_B),
    (2048, 3, 3, None, 1e-6, 3, True, ATOL_B, RTOL_B), (2048, 1, 5, None, 1e-10, 30, True, ATOL_B, RTOL_B),
    (2048, 3, 3, 64, 1e-6, 3, True, ATOL_B, RTOL_B),
    # fp32 oracle at 0.369 of the project's tolerance (2048-term windows of eps around one large term): bound 4 x 0.369 = 1.48 x it
    (2048, 1, 3, 2048, 1e-6, 30, True, 1.48e-5, 1.48e-4),
    (2048, 1, 2, 2055, 1e-10, 3, False, ATOL_B, RTOL_B),
]


@functools.lru_cache(maxsize=None)
def sa_inputs(S, U, BH, chunk, eps, scale, with_len):
    g = _seed(S, U, BH, chunk or 0, scale, int(with_len), int(eps * 1e12), 1)
    kl = _key_len(BH, S, g)
    if not with_len:
        kl = None
    alpha = ar.mass_preservation(ar.expected_alignment(_spread_p(BH, U, S, kl, g, spike=8.0), kl, EPS), kl).float().contiguous()
    energy = (torch.randn(BH, U, S, generator=g) * scale).contiguous()
    return alpha, energy, kl


@functools.lru_cache(maxsize=None)
def sa_ref(S, U, BH, chunk, eps, scale, with_len, mutation=None):
    alpha, energy, kl = sa_inputs(S, U, BH, chunk, eps, scale, with_len)
    return ar.expected_soft_attention(alpha, energy, kl, chunk, eps, mutation=mutation)


def sa_mutations(S, U, chunk, with_len):
    m = []
    if with_len and U > 1 and S > 1:             # S = 1 has no ragged lengths
        m.append("keylen_of_row")
    if chunk is None and S > 64:
        m += ["soft_drop_fwd_carry", "soft_drop_rev_carry"]
    if chunk is not None and chunk < S:
        m.append("chunk_window_off_by_one")
    return m


def _oracle_beta(alpha, energy, kl, chunk, eps):
    from oracle import monotonic as omo
    BH, U, S = alpha.shape
    pad = None if kl is None else torch.arange(S).view(1, S) >= kl.long().view(BH, 1)
    return omo.expected_soft_attention(alpha, energy, pad, chunk, eps)


def test_soft_attention_reference_bounds_and_mutants():
    """per case: the fp32 oracle against fp64 within the case's bound, and in fact within a quarter of it (else the 4 x rule of the
    table applies and the table must say so); every applicable mutant more than 10 x the bound away"""
    worst = 0.0
    for case in SA_CASES:
        S, U, BH, chunk, eps, scale, with_len, atol, rtol = case
        assert (BH * U) % 4 != 0
        alpha, energy, kl = sa_inputs(*case[:7])
        assert _chunk_cover(alpha[0].double()) > COVER, case
        ref = sa_ref(*case[:7])
        r = float(_tol_ratio(_oracle_beta(alpha, energy, kl, chunk, eps), ref, ATOL_B, RTOL_B).max())
        worst = max(worst, r)
        assert r <= 1.0, (case, r)                   # the reference and the oracle agree at the project's tolerance, whatever the bound
        assert r <= 0.25 or (atol >= 4 * r * ATOL_B and rtol >= 4 * r * RTOL_B), (case, r)
        assert atol <= 1.01 * max(ATOL_B, 4 * r * ATOL_B) and rtol <= 1.01 * max(RTOL_B, 4 * r * RTOL_B), case    # two digits written
        for mut in sa_mutations(S, U, chunk, with_len):
            m = float(_tol_ratio(sa_ref(*case[:7], mut), ref, atol, rtol).max())
            assert m > MUTANT_FACTOR, (case, mut, m)
    print(f"\n[soft attention] fp32 oracle vs fp64: largest err/tol {worst:.4f}")


# ----------------------------------------------------------------------------------------------------- backward: the cases
# (S, U, BH, with key_len, family, seed).  p <= 0.98 keeps u off 1.  The seed is picked so that no bh row has to be dropped.
BW_SEED = {(63, False, "sigmoid"): 1, (129, True, "sigmoid"): 1, (257, False, "sigmoid"): 1, (4096, True, "sigmoid"): 2}
BW_CASES = [(S, U, BH, wl, fam, BW_SEED.get((S, wl, fam), 0)) for (S, U, BH) in [(1, 1, 3), (2, 2, 4), (63, 5, 5), (64, 1, 6), (65, 2, 7), (129, 5, 8), (257, 2, 9),
                                                        (1024, 5, 3), (4096, 16, 4)]
            for wl in (True, False) for fam in ("spread", "sigmoid")]


@functools.lru_cache(maxsize=None)
def bw_inputs(S, U, BH, with_len, family, seed):
    g = _seed(S, U, BH, int(with_len), int(family == "spread"), seed, 99)
    kl = _key_len(BH, S, g)
    if not with_len:
        kl = None
    if family == "spread":
        p = _spread_p(BH, U, S, kl, g, pmax=0.98)
    else:
        p = torch.sigmoid(torch.randn(BH, U, S, generator=g) * 2).clamp(max=0.98)
    up = torch.randn(BH, U, S, generator=g)
    return p.contiguous(), kl, up


@functools.lru_cache(maxsize=None)
def bw_ref(S, U, BH, with_len, family, seed, mutation=None):
    """-> (grad fp64 with exact zeros at padded positions, keep [BH] bool: rows off the gradient's jumps)"""
    p, kl, up = bw_inputs(S, U, BH, with_len, family, seed)
    grad, _, c, u = ar.alignment_grad(p, kl, EPS, up, mutation=mutation)
    near = ((c - EPS).abs() < 0.01 * EPS) | ((u - 1.0).abs() < 1e-3)
    return grad, ~near.flatten(1).any(dim=1)


def bw_mutations(S, family):
    return ["drop_sum_carry", "drop_prod_carry"] if (S > 64 and family == "spread") else []


def _grad_ratio(got, ref, keep):
    """largest over the kept bh rows of max |got - ref| / (GRAD_BOUND * max |ref|)"""
    err = (got.double() - ref).abs().flatten(1).max(dim=1).values
    scale = ref.abs().flatten(1).max(dim=1).values
    r = torch.where((scale == 0) & (err == 0), torch.zeros_like(err), err / (GRAD_BOUND * scale))    # an all-zero row reproduced
    r = torch.nan_to_num(r, nan=float("inf"), posinf=float("inf"))                                    # NaN / inf: infinitely far
    return float(r[keep].max()) if bool(keep.any()) else 0.0


def test_backward_cases_rows_kept_oracle_error_and_mutants():
    """from the reference alone: at most 10 % of a case's rows sit on a jump of the gradient; the fp32 oracle's own autograd is
    within a quarter of the bound (so the bound stays the project's 2e-4); the carry mutants are more than 10 x the bound away"""
    from oracle import monotonic as omo
    worst = 0.0
    for case in BW_CASES:
        S, U, BH, with_len, fam, seed = case
        p, kl, up = bw_inputs(*case)
        ref, keep = bw_ref(*case)
        assert float(p.max()) <= 0.98 + 1e-7
        assert int((~keep).sum()) <= 0.1 * BH, (case, keep)
        pad = None if kl is None else torch.arange(S).view(1, S) >= kl.long().view(BH, 1)
        pr = p.clone().requires_grad_(True)
        (omo.expected_alignment_from_p_choose(pr, pad, EPS) * up).sum().backward()
        r = _grad_ratio(pr.grad, ref, keep)
        worst = max(worst, r)
        assert r <= 0.25, (case, r)
        if kl is not None:
            assert float(ref[~_valid(kl, BH, U, S)].abs().max() if bool((~_valid(kl, BH, U, S)).any()) else 0.0) == 0.0
        for mut in bw_mutations(S, fam):
            m = _grad_ratio(bw_ref(*case, mut)[0], ref, keep)
            assert m > MUTANT_FACTOR, (case, mut, m)
    print(f"\n[backward] fp32 oracle autograd vs fp64: largest err/bound {worst:.4f}")


def test_backward_spread_cases_cross_every_chunk():
    for case in BW_CASES:
        S, U, BH, with_len, fam, seed = case
        if fam == "spread":
            p, kl, _ = bw_inputs(*case)
            c = _chunk_cover(ar.expected_alignment(p, kl, EPS)[0])
            assert c > COVER, (case, c)


# ===================================================================================================== GPU part
@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


@pytest.fixture(scope="module")
def general_ops():
    """a handle created under SIMULST_EA_GENERAL=1: every source length goes to the chunked general kernel"""
    from simulst_amd import _lib
    from simulst_amd.ops import Ops
    os.environ["SIMULST_EA_GENERAL"] = "1"
    try:
        return Ops(_lib.Handle())
    finally:
        del os.environ["SIMULST_EA_GENERAL"]


def _dev(t):
    return None if t is None else t.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("cls", list(EA_CASES))
def test_expected_alignment_vs_fp64(ops, general_ops, cls):
    """every case and family of the class against fp64 on the valid positions, naturally dispatched and (S <= 512) through the
    general kernel; the staircase family against the literal one-hot too"""
    worst = {"natural": 0.0, "general": 0.0}
    for S, U, BH in EA_CASES[cls]:
        for fam in ea_families(S):
            p, kl, eps = ea_inputs(S, U, BH, fam)
            ref, v = ea_ref(S, U, BH, fam), _valid(kl, BH, U, S)
            runs = [("natural", ops)] + ([("general", general_ops)] if S <= 512 else [])
            for name, o in runs:
                got = o.expected_alignment(_dev(p), _dev(kl), eps).cpu()
                r = float(_tol_ratio(got, ref, ATOL_A, RTOL_A)[v].max())
                worst[name] = max(worst[name], r)
                assert r <= 1.0, (cls, name, S, U, BH, fam, r)
                if fam == "staircase":
                    onehot = torch.where(v, p, torch.zeros(()))
                    assert float((got - onehot)[v].abs().max()) <= ATOL_A, (cls, name, S, U, BH)
    print(f"\n[expected_alignment] {cls}: largest err/tol natural {worst['natural']:.4f}"
          + (f", SIMULST_EA_GENERAL=1 {worst['general']:.4f}" if cls != "general" else ""))


@pytest.mark.gpu
def test_expected_alignment_refuses_longer_sources(ops):
    p = torch.full((1, 1, 4097), 0.5, device="cuda")
    with pytest.raises(RuntimeError, match=r"S <= 4096"):
        ops.expected_alignment(p, None, EPS)


@pytest.mark.gpu
def test_mass_preservation_vs_fp64(ops):
    """in place: zeros at and beyond key_len, every position before the last valid one untouched to the bit, the last valid one
    against fp64"""
    worst = 0.0
    for S, U, BH, with_len in MP_CASES:
        alpha, kl = mp_inputs(S, U, BH, with_len)
        ref = ar.mass_preservation(alpha, kl)
        buf = alpha.cuda()
        out = ops.mass_preservation(buf, _dev(kl))
        assert out.data_ptr() == buf.data_ptr()
        got = out.cpu()
        v = _valid(kl, BH, U, S)
        last = v.sum(-1, keepdim=True) - 1
        is_last = torch.arange(S).view(1, 1, S) == last
        assert bool((got[~v] == 0).all()), (S, U, BH)
        before = v & ~is_last
        assert torch.equal(got[before].view(torch.int32), alpha[before].view(torch.int32)), (S, U, BH)
        r = float(_tol_ratio(got[is_last], ref[is_last], ATOL_B, RTOL_B).max())
        worst = max(worst, r)
        assert r <= 1.0, (S, U, BH, with_len, r)
    print(f"\n[mass_preservation] largest err/tol {worst:.4f}")


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["infinite_lookback", "chunkwise"])
def test_expected_soft_attention_vs_fp64(ops, group):
    worst = 0.0
    for case in SA_CASES:
        S, U, BH, chunk, eps, scale, with_len, atol, rtol = case
        if (chunk is None) != (group == "infinite_lookback"):
            continue
        alpha, energy, kl = sa_inputs(*case[:7])
        got = ops.expected_soft_attention(_dev(alpha), _dev(energy), _dev(kl), chunk, eps).cpu()
        r = float(_tol_ratio(got, sa_ref(*case[:7]), atol, rtol).max())
        worst = max(worst, r)
        assert r <= 1.0, (case, r)
    print(f"\n[expected_soft_attention] {group}: largest err/tol {worst:.4f}")


@pytest.mark.gpu
def test_expected_soft_attention_refuses_longer_sources(ops):
    a = torch.zeros(1, 1, 2049, device="cuda")
    with pytest.raises(RuntimeError, match=r"S <= 2048"):
        ops.expected_soft_attention(a, a.clone(), None, None, EPS)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["spread", "sigmoid"])
def test_expected_alignment_backward_vs_fp64_autograd(family):
    """through simulst_amd.losses.expected_alignment: exact zeros at padded positions; elsewhere the error over the bh row's largest
    reference gradient below 2e-4, on the rows the reference keeps off the gradient's jumps"""
    from simulst_amd import losses as sl
    worst = 0.0
    for case in BW_CASES:
        S, U, BH, with_len, fam, seed = case
        if fam != family:
            continue
        p, kl, up = bw_inputs(*case)
        ref, keep = bw_ref(*case)
        pd = p.cuda().requires_grad_(True)
        alpha = sl.expected_alignment(pd, _dev(kl), EPS)
        (alpha * up.cuda()).sum().backward()
        got = pd.grad.cpu()
        v = _valid(kl, BH, U, S)
        assert bool(torch.isfinite(got).all()), case
        assert bool((got[~v] == 0).all()), case
        r = _grad_ratio(got, ref, keep)
        worst = max(worst, r)
        assert r <= 1.0, (case, r)
    print(f"\n[expected_alignment_backward] {family}: largest err/bound {worst:.4f}")


@pytest.mark.gpu
def test_expected_alignment_backward_refuses_longer_sources():
    """the library call itself: through simulst_amd.losses the forward would refuse first"""
    from simulst_amd.ops import Ops, _p
    o = Ops()
    t = torch.zeros(1, 1, 4097, device="cuda")
    grad_p = torch.zeros_like(t)
    with pytest.raises(RuntimeError, match=r"simulst_expected_alignment_backward.*S <= 4096"):
        o.h.check(o.lib.simulst_expected_alignment_backward(o.h.ptr, _p(t), _p(t), _p(t), _p(grad_p), None, 1, 1, 4097, EPS),
                  "simulst_expected_alignment_backward")
