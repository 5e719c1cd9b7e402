"""The one case table of tests/test_linear_ref_cpu.py and tests/test_hip_linear.py: which simulst_linear calls are made, with what
operands, and the bound every output element is held to.

A case is a descriptor (a dict under the header's field names), the dtype, the handle's options and environment overrides (as
test_linear_plan.py's _handle takes them), the operand class, the operands that start off their alignment and the kernel family and
variant flags the call is meant to reach -- test_linear_ref_cpu.py asserts against csrc/gemm_plan.cpp that it does.  Tile constants come
from csrc/gemm_plan.h and thresholds from the handle's defaults in csrc/common.h, both read from the sources.

Operand classes
  EXACT   A and W integers in [-3, 3], bias and residual multiples of 1/4 up to 8: every partial sum in any order is an integer below
          2^24, exact in fp32.  BIAS / RES / F32OUT outputs must equal the reference rounded once to the output dtype; the activations
          are held to e_act + u |ref|.  LayerNorm cases cannot be exact and are RANDOM.
  RANDOM  A is N(0, 1), W is N(0, 1) / sqrt(K), the bias N(0, 1), the residual N(0, 1); one A row in eight is scaled by 1000 and one W
          row in eight by 1e-3, so that no absolute tolerance could hide a column.  Two choices the 2 % rule (at most 2 % of the compared
          elements may lie below their own bound, asserted on the CPU) forces: W carries 1 / sqrt(K), so that the bias stays visible
          against (K + 3) 2^-23 S at K = 8192; and under GELU, GLU and RES_GELU the tall rows are scaled by 2, not 1000 -- gelu(-1000)
          and sigmoid(-1000) are 0, and with the activation's GLOBAL Lipschitz constant in the bound every such output would lie below
          its bound.  LayerNorm cases also scale one row in eight by 2^-8: its variance, 1.5e-5, is the size of eps, so eps is seen.

Guards: every element of the A buffer that the descriptor does not address is NaN (stride gaps, the rows between rows_per_batch and the
batch stride, 256 elements in front and behind), 16 NaN rows follow a row-major W, 8 NaN follow the bias, every residual element the
call does not address is NaN, and C and aux are filled with a NaN bit pattern that every element the reference does not list must keep.
"""
import os
import re
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import linear_ref as lr
from linear_ref import BF16, BIAS, EMF_OUT, F32, F32OUT, GELU, GLU, RES, RES_GELU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simulst_amd", "csrc")
U23, U24, U8 = 2.0 ** -23, 2.0 ** -24, 2.0 ** -8
GELU_LIP = 1.13                       # sup |gelu'|
E_GELU_FIT = 7.1e-7                   # csrc/common.h: the bf16 kernels' fitted GELU, error of the result in fp32
SENT16, SENT32 = 0x7FB7, 0x7FB7C3A5   # NaN bit patterns nobody computes
N_CUS = 256


def _constants():
    plan = open(os.path.join(CSRC, "gemm_plan.h")).read()
    c = {}
    for stmt in re.findall(r"constexpr int ([^;]*);", plan):
        for name, val in re.findall(r"(\w+) = (\d+)\b(?! \*)", stmt):
            c[name] = int(val)
    common = open(os.path.join(CSRC, "common.h")).read()
    for name in ("panel_split_min_rows", "panel_split_blocks", "mid_min_blocks", "mid_narrow_min_rows", "skinny_min_blocks_tall"):
        c[name] = int(re.search(r"int %s = (\d+);" % name, common).group(1))
    return c


CONST = _constants()
PB_M, PW_M, TB, TBK, RBK = CONST["PB_M"], CONST["PW_M"], CONST["TB"], CONST["TBK"], CONST["RBK"]
TILE_MIN_ROWS, SPLIT_ROWS, NARROW_ROWS = CONST["TILE_MIN_ROWS"], CONST["panel_split_min_rows"], CONST["mid_narrow_min_rows"]
SKINNY_MAX_PACKED = CONST["SKINNY_MAX_ROWS_PACKED"]

CASES = []


def add(family, dtype, epi, M, N, K, cls=None, B=1, ln=False, packed=False, a_rs=None, a_gap=0, a_bgap=0, a_lead=0, c_gap=0, r_gap=0,
        hd=0, th=0, n_main=0, aux_rows=0, scale=1.0, opts=None, env=None, mis=(), **flags):
    """M = rows per batch.  *_gap: elements between the end of a row and the next one; a_bgap: rows' worth of elements between batches"""
    G = lr.vec_elems(dtype)
    a_rs = (K if a_rs is None else a_rs) + a_gap
    a_bs = (M + a_bgap) * a_rs
    Nc = N // 2 if epi == GLU else N
    d = dict(M_batches=B, rows_per_batch=M, N=N, K=K, a_batch_stride=a_bs, a_row_stride=a_rs, a_lead=a_lead, epilogue=epi, dtype=dtype,
             scale=scale, n_main=n_main, aux_rows=aux_rows, aux_batch_stride=0, w_fragment_major=int(packed), c_head_dim=hd,
             c_head_stride=0, c_tensor_heads=th, c_tensor_stride=0)
    rows_c = n_main if epi == EMF_OUT else M
    if hd:                                                   # [tensor][batch][head][row][hd], a gap of c_gap elements after every row
        d["c_row_stride"] = hd + c_gap
        d["c_head_stride"] = rows_c * d["c_row_stride"] + 8
        heads = th if th else N // hd
        d["c_batch_stride"] = heads * d["c_head_stride"]
        d["c_tensor_stride"] = B * d["c_batch_stride"] + 16 if th else 0
    else:
        d["c_row_stride"] = Nc + c_gap
        d["c_batch_stride"] = rows_c * d["c_row_stride"] + (8 if c_gap else 0)
    d["r_row_stride"] = N + r_gap
    d["r_batch_stride"] = rows_c * d["r_row_stride"] + (8 if r_gap else 0)
    if epi == EMF_OUT:
        d["aux_batch_stride"] = (aux_rows + 1) * N
    for c in ([cls] if cls else (["RANDOM"] if ln else ["EXACT", "RANDOM"])):
        assert not (ln and c == "EXACT")
        name = f"{family}-{'f32' if dtype == F32 else 'bf16'}-e{epi}-{B}x{M}x{N}x{K}" + ("-ln" if ln else "") + ("-fm" if packed else "") + \
               (f"-rs{a_rs}" if a_rs != K else "") + (f"-lead{a_lead}" if a_lead else "") + (f"-cg{c_gap}" if c_gap else "") + \
               (f"-hd{hd}" if hd else "") + (f"-th{th}" if th else "") + ("-mis" + "".join(mis) if mis else "") + \
               "".join(f"-{k}{v}" for k, v in sorted({**(opts or {}), **(env or {})}.items())).replace("SIMULST_", "") + "-" + c.lower()
        assert name not in {x["name"] for x in CASES}, name
        CASES.append(dict(name=name, family=family, flags=flags, d=dict(d), dtype=dtype, cls=c, ln=ln, opts=opts or {}, env=env or {},
                          mis=tuple(mis)))


def _table():
    # ---- skinny ---------------------------------------------------------------------------------------------------------------------
    for dtype in (F32, BF16):
        G = lr.vec_elems(dtype)
        KS = 4 * G
        for M in (1, 15, 16, 17, 33, 63, 64, 65, 255):       # rows: both sides of the 16-row tile and of 64
            add("skinny", dtype, BIAS if M % 2 else RES, M, 33, KS + G, c_gap=8 if M in (16, 65) else 0, r_gap=16, a_gap=G if M > 16 else 0)
        for N in (1, 15, 16, 17, 250):                       # columns, row-major
            add("skinny", dtype, GELU if N in (15, 250) else BIAS, 17, N, 2 * KS, c_gap=8 if N == 16 else 0)
        for N in (16, 32, 48):                               # columns, fragment-major
            add("skinny", dtype, F32OUT if N == 32 else RES, 33, N, KS, packed=True, r_gap=8)
        for K in sorted({G, KS - G, KS, 16 * KS, 16 * KS + G, 520}):      # k: the last k-step short, a whole wave round, one group more
            add("skinny", dtype, RES_GELU if K == 520 else BIAS, 17, 17, K, a_gap=G if K != KS else 0, r_gap=8)
        for K in (KS, 8 * KS, 16 * KS):                      # LayerNorm prologue
            add("skinny", dtype, GELU if K == KS else BIAS, 33, 48, K, ln=True, packed=K == 8 * KS, ln_=1)
        add("skinny", dtype, F32OUT, 17, 17, KS + G, ln=True, ln_=1)          # ... with a short last k-step
        add("skinny", dtype, RES, 5, 17, KS + G, B=3, a_bgap=2, a_gap=G, c_gap=8, r_gap=8)      # rows_per_batch < M, batch stride
        # every (MTs, NTs) the plan picks
        add("skinny", dtype, BIAS, 255, 1024, G, cls="RANDOM", MTs=2, NTs=1)
        add("skinny", dtype, BIAS, 255, 528, G, cls="EXACT", MTs=1, NTs=2)
        # (4, 1): 64-row tiles over a wide output fill the chip once the columns are halved -- fc1 of ~200 co-scheduled rows
        add("skinny", dtype, BIAS, 255, 2048, KS + G, cls="EXACT", MTs=4, NTs=1)
        add("skinny", dtype, RES, 255, 2048, KS + G, cls="RANDOM", MTs=4, NTs=1, r_gap=8, c_gap=8)
        add("skinny", dtype, GELU, 200, 2048, 8 * KS, ln=True, MTs=4, NTs=1, ln_=1)
        add("skinny", dtype, RES, 65, 33, KS + G, env={"SIMULST_SKINNY_MIN_BLOCKS_TALL": 1}, MTs=4, NTs=2, r_gap=8)
        add("skinny", dtype, GELU, 130, 17, 8 * KS, ln=True, env={"SIMULST_SKINNY_MIN_BLOCKS_TALL": 1}, MTs=4, NTs=2, ln_=1)
        add("skinny", dtype, BIAS, 130, 17, 16 * KS, ln=True, env={"SIMULST_SKINNY_MIN_BLOCKS_TALL": 1}, MTs=2, NTs=2, ln_=1)
        # split-K
        add("skinny", dtype, BIAS, 17, 33, 4096, split=True, splits=4)
        add("skinny", dtype, RES, 33, 17, 4104, split=True, splits=4, r_gap=8)          # the last split is short
        add("skinny", dtype, RES, 15, 16, 8192, cls="RANDOM", split=True, splits=8)
        add("skinny", dtype, BIAS, 255, 250, 8192, cls="EXACT", split=True, splits=4)   # mt * nt * 8 > 1024 halves the count
    # ---- wave tile ------------------------------------------------------------------------------------------------------------------
    for dtype in (F32, BF16):
        KS = 4 * lr.vec_elems(dtype)
        for i, M in enumerate(TILE_MIN_ROWS + r for r in (0, 1, 15, 16, 17)):      # 256 .. 273: the first rows the wave tile takes
            add("wave_tile", dtype, (BIAS, RES, GELU, F32OUT, RES_GELU)[i], M, (16, 24, 250, 504, 24)[i], KS if i % 2 else 8 * KS,
                c_gap=8 if i == 1 else 0, r_gap=8, ln_=0)
        add("wave_tile", dtype, BIAS, TILE_MIN_ROWS + 1, 250, KS, ln=True, ln_=1)
        add("wave_tile", dtype, GELU, TILE_MIN_ROWS + 17, 24, 8 * KS, ln=True, packed=False, ln_=1)
        add("wave_tile", dtype, RES, TILE_MIN_ROWS + 16, 48, 8 * KS, packed=True, ln_=0)
    # ---- mid ------------------------------------------------------------------------------------------------------------------------
    low = {"SIMULST_MID_MIN_BLOCKS": 1}
    for dtype in (F32, BF16):
        KS = 4 * lr.vec_elems(dtype)
        for i, M in enumerate(TILE_MIN_ROWS + r for r in (0, 1, 63, 64, 65)):      # 256 .. 321: both sides of the 64-row tile
            add("mid", dtype, (BIAS, RES, GELU, F32OUT, RES_GELU)[i], M, (512, 520, 576, 520, 512)[i], KS if i % 2 else 8 * KS, env=low,
                cls="RANDOM" if i % 2 else "EXACT", c_gap=8 if i == 1 else 0, r_gap=8, tall=0, ln_=0)
        add("mid", dtype, BIAS, TILE_MIN_ROWS + 1, 520, KS, ln=True, env=low, tall=0, ln_=1)
        add("mid", dtype, GELU, TILE_MIN_ROWS + 64, 512, 8 * KS, ln=True, env=low, packed=True, tall=0, ln_=1)
        add("mid", dtype, RES, TILE_MIN_ROWS + 1, 512, 2048, env=low, cls="RANDOM", tall=0, ln_=0)
        narrow = {"SIMULST_MID_NARROW_MIN_ROWS": TILE_MIN_ROWS + 64, "SIMULST_MID_MIN_BLOCKS": 1}
        add("mid", dtype, BIAS, TILE_MIN_ROWS + 64, 64, KS, env=narrow, cls="EXACT", tall=0, ln_=0)
        add("mid", dtype, RES, TILE_MIN_ROWS + 65, 256, 8 * KS, env=narrow, cls="RANDOM", tall=0, ln_=0)
        # ... and at the handle's own threshold (fragment-major weights: above SKINNY_MAX_ROWS), one row below it the wave tile
        add("mid", dtype, BIAS, NARROW_ROWS, 64, KS, packed=True, cls="EXACT", tall=0, ln_=0)
        add("mid", dtype, RES, NARROW_ROWS + 1, 256, 8 * KS, packed=True, cls="RANDOM", tall=0, ln_=0, r_gap=8)
        add("wave_tile", dtype, BIAS, NARROW_ROWS - 1, 64, KS, packed=True, cls="EXACT", ln_=0)
        add("mid", dtype, BIAS, 2048, 2048, KS, cls="EXACT" if dtype == F32 else "RANDOM", tall=1, ln_=0)      # the smallest tall grid
        add("mid", dtype, RES, 2049, 2048, KS, packed=True, cls="RANDOM" if dtype == F32 else "EXACT", tall=1, ln_=0, c_gap=8)
    # ---- split row panel ------------------------------------------------------------------------------------------------------------
    few = {"SIMULST_PANEL_SPLIT_BLOCKS": 64}
    for i, dM in enumerate((0, 1, 127, 129)):
        M = SPLIT_ROWS + dM
        add("panel_split", BF16, (BIAS, GELU, RES, BIAS)[i], M, (512, 528, 512, 2048)[i], (32, 224, 256, 32)[i], packed=True,
            env=few if i < 3 else None, cls="RANDOM" if i % 2 else "EXACT", c_gap=8 if i == 2 else 0, r_gap=8, ln_=0)
        add("panel_split", BF16, (BIAS, GELU, F32OUT, GELU)[i], M, (528, 512, 2048, 512)[i], (224, 256, 32, 32)[i], packed=True, ln=True,
            env=few if i != 2 else None, ln_=1)
    add("panel_split", BF16, BIAS, SPLIT_ROWS + 1, 512, 256, packed=True, hd=64, env=few, cls="EXACT", ln_=0)
    add("panel_split", BF16, BIAS, SPLIT_ROWS + 129, 2048, 224, packed=True, hd=64, c_gap=8, cls="RANDOM", ln_=0)
    # ---- row panel ------------------------------------------------------------------------------------------------------------------
    off = {"WEIGHT_STATIONARY": 0, "PANEL_WIDE": 0}
    P0 = SKINNY_MAX_PACKED // PB_M * PB_M                   # whole panels up to the rows the decode-step kernels keep: 8192
    for i, (M, N, K) in enumerate(((P0 + 1, 16, 32), (P0 + PB_M, 64, 96), (P0 + PB_M + 1, 80, 256), (P0 + 1, 768, 256))):
        add("panel", BF16, (GELU, RES, BIAS, BIAS)[i], M, N, K, packed=True, opts=off if i == 3 else None, cls="RANDOM" if i % 2 else "EXACT",
            c_gap=8 if i == 1 else 0, r_gap=8, ln_=0)
        add("panel", BF16, (BIAS, GELU, GELU, BIAS)[i], M, (16, 64, 80, 64)[i], K, packed=True, ln=True, ln_=1)
    add("panel", BF16, EMF_OUT, P0 // 2 + PB_M // 2 + 3, 64, 96, B=2, packed=True, n_main=P0 // 2 + PB_M // 2, aux_rows=2, cls="EXACT", r_gap=8, ln_=0)
    add("panel", BF16, EMF_OUT, P0 + PB_M + 1 + 2, 80, 256, packed=True, n_main=P0 + PB_M + 1, aux_rows=1, cls="RANDOM", ln_=0)
    # ---- wide row panel -------------------------------------------------------------------------------------------------------------
    nws = {"WEIGHT_STATIONARY": 0}
    W0 = SKINNY_MAX_PACKED // PW_M * PW_M                   # 8192; one row and one 256-row panel + one row more
    add("panel_wide", BF16, BIAS, W0 + 1, 32, 256, packed=True, cls="EXACT")
    add("panel_wide", BF16, BIAS, W0 + PW_M + 1, 96, 256, packed=True, cls="RANDOM", c_gap=8, a_gap=8)
    add("panel_wide", BF16, BIAS, W0 + 1, 768, 256, packed=True, opts=nws, cls="RANDOM")
    add("panel_wide", BF16, BIAS, W0 + PW_M + 1, 768, 256, packed=True, hd=64, cls="EXACT")
    add("panel_wide", BF16, BIAS, W0 + 1, 768, 256, packed=True, hd=64, th=4, cls="RANDOM")
    for m in ("A", "C", "bias"):                             # off their alignment: the 128-row panel takes the call
        add("panel", BF16, BIAS, P0 + 1, 96, 256, packed=True, mis=(m,), cls="RANDOM" if m == "A" else "EXACT", ln_=0)
    # ---- weight-stationary ----------------------------------------------------------------------------------------------------------
    for i, N in enumerate((256, 512, 768, 1024)):
        add("wstat", BF16, BIAS, 8193 + 64 * i, N, 256, packed=True, cls="RANDOM" if i % 2 else "EXACT", pairs=6 if N == 768 else 8,
            c_gap=8 if i == 1 else 0)
    add("wstat", BF16, EMF_OUT, 8200 + 3, 256, 256, packed=True, n_main=8200, aux_rows=2, cls="RANDOM", pairs=8, r_gap=8)
    add("wstat", BF16, EMF_OUT, 4099 + 4, 256, 256, B=2, packed=True, n_main=4099, aux_rows=3, cls="EXACT", pairs=8, a_bgap=1)
    add("wstat", BF16, BIAS, 2731, 768, 256, B=3, packed=True, cls="EXACT", pairs=6, a_bgap=1, c_gap=8)
    # ---- 256 x 256 GLU tiles --------------------------------------------------------------------------------------------------------
    for ring, ks in ((0, (8, TBK - 8, TBK, TBK + 8)), (1, (RBK - 8, RBK, RBK + 8))):
        o = {"CONV_TILE256": 2 if ring else 1}                # (the handle's default is the ring)
        for i, K in enumerate(ks):
            add("tile256", BF16, GLU, (TB * 32, TB * 32 + 1, TB * 33 - 1, TB * 33)[i % 4], (256, 512)[i % 2], K, opts=o, scale=(1.0, 16.0)[i % 2],
                cls="RANDOM" if i % 2 else "EXACT", ring=ring, c_gap=8 if i == 2 else 0)
        # a real causal conv: stride 2 over 16 channels, 5 taps: a_row_stride = 32 < K = 80, a_lead = 64
        add("tile256", BF16, GLU, 4100, 256, 80, B=2, a_rs=32, a_lead=64, opts=o, scale=16.0, cls="RANDOM", ring=ring, conv=True)
    # ---- 128 x 128 and 64 x 64 tiles ------------------------------------------------------------------------------------------------
    for dtype in (F32, BF16):
        G = lr.vec_elems(dtype)
        KS = 4 * G
        epis = (BIAS, GELU, RES, F32OUT, RES_GELU, BIAS, RES)
        for i, M in enumerate((1, 63, 64, 65, 512, 513, 641)):   # a_lead != 0: 64 x 64 up to 512 rows, 128 x 128 above
            add("tile64" if M <= 512 else "tile128", dtype, epis[i], M, (8, 56, 64, 72, 136, 72, 136)[i], (G, 2 * G, KS + G)[i % 3],
                a_lead=G if i % 2 else 2 * G, cls="RANDOM" if i % 2 else "EXACT", c_gap=8 if i == 3 else 0, r_gap=8)
        add("tile64", dtype, RES, 65, 56, KS + G, a_rs=2 * G, a_lead=KS + G)      # overlapping rows; row 0 is left padding alone
        add("tile128", dtype, GELU, 513, 8, KS + G, a_rs=G, a_lead=KS, B=2, cls="RANDOM", conv=True)      # 5 taps over G channels, stride 1
        for i, (M, N) in enumerate(((1, 64), (65, 128), (513, 192))):             # GLU: always the 128 x 128 tile
            add("tile128", dtype, GLU, M, N, (G, 2 * G, KS + G)[i], scale=(1.0, 16.0, 0.5)[i], a_lead=G * (i % 2), c_gap=8 if i == 1 else 0)
        add("tile128", dtype, GLU, 130, 128, 5 * 2 * G, B=2, a_rs=2 * 2 * G, a_lead=4 * 2 * G, scale=16.0, conv=True)      # 5 taps, stride 2
        add("tile64", dtype, EMF_OUT, 63 + 3, 56, 2 * G, B=2, n_main=63, aux_rows=2, r_gap=8)
        add("tile64", dtype, EMF_OUT, 64 + 1, 72, KS + G, n_main=64, aux_rows=0, cls="EXACT")
        add("tile128", dtype, EMF_OUT, 320 + 5, 136, KS + G, B=2, n_main=320, aux_rows=4, cls="RANDOM", c_gap=8)


_table()
BY_NAME = {c["name"]: c for c in CASES}
FAMILIES = ("wstat", "panel_wide", "panel", "panel_split", "mid", "wave_tile", "skinny", "tile256", "tile128", "tile64")


def plan_line(c):
    """the case as a row of tests/linear_plan_table.cpp's `plan` mode (columns of test_linear_plan.py)"""
    from test_linear_plan import CALL_COLS, _handle_cols
    d = c["d"]
    r = dict(dtype=c["dtype"], epi=d["epilogue"], batches=d["M_batches"], rpb=d["rows_per_batch"], N=d["N"], K=d["K"], a_bs=d["a_batch_stride"],
             a_rs=d["a_row_stride"], a_lead=d["a_lead"], c_bs=d["c_batch_stride"], c_rs=d["c_row_stride"], r_bs=d["r_batch_stride"],
             r_rs=d["r_row_stride"], n_main=d["n_main"], aux_rows=d["aux_rows"], aux_bs=d["aux_batch_stride"], ln=int(c["ln"]),
             packed=d["w_fragment_major"], c_hd=d["c_head_dim"], c_hs=d["c_head_stride"], c_th=d["c_tensor_heads"], c_ts=d["c_tensor_stride"])
    return _handle_cols(N_CUS, c["opts"], c["env"]) + [r[k] for k in CALL_COLS] + [int(m in c["mis"]) for m in ("A", "C", "R", "bias")]


# ======================================================================================================================================
# operands
# ======================================================================================================================================
def tdt(dtype):
    return torch.float32 if dtype == F32 else torch.bfloat16


def _rounded(x, dtype):
    """float64 numpy -> the operand dtype (torch tensor)"""
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(tdt(dtype))


def operands(c):
    """-> dict: torch CPU tensors of the raw buffers (A, W, R in the operand dtype; bias, gamma, beta fp32), a0 / r0 = index of the
    element the call's pointer points at, and the same buffers as float64 numpy arrays (suffix 64) for the reference"""
    d, dtype, cls = c["d"], c["dtype"], c["cls"]
    rng = np.random.default_rng(zlib.crc32(c["name"].encode()))
    B, M, N, K, epi = d["M_batches"], d["rows_per_batch"], d["N"], d["K"], d["epilogue"]
    exact = cls == "EXACT"
    draw = (lambda *s: rng.integers(-3, 4, s).astype(np.float64)) if exact else (lambda *s: rng.standard_normal(s))
    quarter = lambda *s: rng.integers(-32, 33, s) / 4.0
    # A: NaN everywhere, values where the descriptor points
    rel, off = lr.a_index(d)
    ok = np.broadcast_to((rel >= 0)[None], off.shape)
    lo, hi = (int(off[ok].min()), int(off[ok].max())) if ok.any() else (0, 0)      # (a window that is left padding alone: nothing read)
    a0 = 256 - min(lo, 0)
    size = a0 + hi + 1 + 256
    vals = draw(size)
    if not exact:
        tall = 2.0 if epi in (GELU, GLU, RES_GELU) else 1000.0
        rows = np.arange(B * M).reshape(B, M)
        for sel, s in ((rows % 8 == 3, tall),) + (((rows % 8 == 6, 2.0 ** -8),) if c["ln"] else ()):
            scale = np.ones(size)
            scale[(off[sel] + a0)[np.broadcast_to((rel >= 0)[None], off.shape)[sel]]] = s
            vals = vals * scale
    A = np.full(size, np.nan)
    A[off[ok] + a0] = vals[off[ok] + a0]
    # W, 16 NaN rows behind a row-major one
    w = draw(N, K)
    if not exact:
        w = w / np.sqrt(K)
        w[np.arange(N) % 8 == 5] *= 1e-3
    w = _rounded(w, dtype).double().numpy()
    if d["w_fragment_major"]:
        W = np.full(N * K + 16 * K, np.nan)
        W[lr.fragment_index(N, K, dtype).ravel()] = w.ravel()
    else:
        W = np.concatenate([w.ravel(), np.full(16 * K, np.nan)])
    bias = np.concatenate([quarter(N) if exact else rng.standard_normal(N), np.full(8, np.nan)]).astype(np.float32)
    out = dict(a0=a0, A=_rounded(A, dtype), W=_rounded(W, dtype), bias=torch.from_numpy(bias), R=None, r0=0, gamma=None, beta=None)
    if epi in (RES, EMF_OUT, RES_GELU):
        rows_c = d["n_main"] if epi == EMF_OUT else M
        b, i = np.repeat(np.arange(B), rows_c), np.tile(np.arange(rows_c), B)
        ridx = lr.c_index(dict(c_batch_stride=d["r_batch_stride"], c_row_stride=d["r_row_stride"]), b, i, N)
        R = np.full(int(ridx.max()) + 1 + 64, np.nan)
        R[ridx] = quarter(*ridx.shape) if exact else rng.standard_normal(ridx.shape)
        out["R"] = _rounded(R, dtype)
    if c["ln"]:
        out["gamma"] = torch.from_numpy((0.8 + 0.4 * rng.random(K)).astype(np.float32))
        out["beta"] = torch.from_numpy((0.1 * rng.standard_normal(K)).astype(np.float32))
    for k in ("A", "W", "bias", "R", "gamma", "beta"):
        out[k + "64"] = None if out[k] is None else out[k].double().numpy()
    return out


def run_reference(c, ops, mut=None):
    return lr.reference(c["d"], ops["A64"], ops["a0"], ops["W64"], ops["bias64"], ops["R64"], ops["r0"], ops["gamma64"], ops["beta64"],
                        mut=mut, splits=c["flags"].get("splits", 1))


# ======================================================================================================================================
# bounds (derived in the docstring of tests/test_hip_linear.py)
# ======================================================================================================================================
def ln_formula32(x, g, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * g + b


def _act_error(f32, f64, x):
    """4 x the largest error of torch's fp32 CPU function against float64 over x and 2049 points spanning its range"""
    p = x[np.isfinite(x)].ravel()
    if p.size > 1 << 16:
        p = np.concatenate([p[:: p.size >> 16], [p.min(), p.max()]])
    v = np.concatenate([p, np.linspace(p.min(), p.max(), 2049)]).astype(np.float32) if p.size else np.zeros(1, dtype=np.float32)
    return 4.0 * float(np.abs(f32(torch.from_numpy(v)).double().numpy() - f64(v.astype(np.float64))).max())


def measured_constants(c, ops, mags):
    """e_gelu / e_tanh / e_sig and the LayerNorm's e32 of this case, all from the CPU"""
    k, epi, pre = {}, c["d"]["epilogue"], mags["pre"]
    if epi in (GELU, RES_GELU):
        k["e_act"] = _act_error(F.gelu, lr.gelu64, pre)
        if c["dtype"] == BF16:
            k["e_act"] = max(k["e_act"], E_GELU_FIT)
    if epi == EMF_OUT:
        k["e_act"] = _act_error(torch.tanh, np.tanh, pre)
    if epi == GLU:
        k["e_act"] = _act_error(torch.sigmoid, lr.sigmoid64, pre)
    if c["ln"]:
        x = torch.from_numpy(lr.effective_a(c["d"], ops["A64"], ops["a0"]))
        y64 = lr.layer_norm64(x.numpy(), ops["gamma64"], ops["beta64"])[0]
        k["e32"] = float(np.abs(ln_formula32(x.float(), ops["gamma"], ops["beta"]).double().numpy() - y64).max())
    return k


def bounds(c, streams, mags, k):
    """-> {stream: per-element bound}.  EXACT classes: 0 for the epilogues without an activation (the caller compares bits)"""
    d, dtype = c["d"], c["dtype"]
    exact = c["cls"] == "EXACT"
    K = d["K"]
    u_op = U8 if dtype == BF16 else U24
    core = (K + 3) * U23 * (mags["S"] + mags["babs"] + mags["rabs"])
    splits = c["flags"].get("splits", 1)
    if splits > 1:
        core = core + splits * U24 * mags["S"]
    if c["ln"]:
        core = core + u_op * mags["S"] + 4.0 * k["e32"] * mags["absw"].sum(1)[None] + 2.0 ** -22 * (mags["ln_gz"] @ mags["absw"].T)
    if exact:
        core = np.zeros_like(core)
    out = {}
    for name, st in streams.items():
        u_st = U24 if (dtype == F32 or d["epilogue"] == F32OUT) else U8
        ref, rows = st["val"], st["rows"]
        if st["act"] is None:
            b = core[rows] + u_st * np.abs(ref)
        elif st["act"] == "gelu":
            b = GELU_LIP * core[rows] + k["e_act"] + u_st * np.abs(ref)
        elif st["act"] == "tanh":
            b = core[rows] + k["e_act"] + u_st * np.abs(ref)
        else:                                                # s * v * sigmoid(g): the product rule, sigmoid' <= 1 / 4, two fp32 products
            v, g = mags["pre"][:, st["vrow"]], mags["pre"][:, st["grow"]]
            b = abs(st["scale"]) * (core[:, st["vrow"]] * lr.sigmoid64(g) + np.abs(v) * (0.25 * core[:, st["grow"]] + k["e_act"])) + \
                (3 * U24 + u_st) * np.abs(ref)
        out[name] = b
    return out


def sentinel_like(n, out_f32):
    return np.full(n, SENT32, dtype=np.uint32).view(np.int32) if out_f32 else np.full(n, SENT16, dtype=np.uint16).view(np.int16)


def round_once(val, out_f32):
    """the float64 reference rounded once to the output dtype, as that dtype's bits.  (EXACT values are multiples of 1 / 4 below 2^22:
    the float32 step in between is exact.)"""
    t = torch.from_numpy(np.ascontiguousarray(val, dtype=np.float64)).float()
    return t.view(torch.int32).numpy() if out_f32 else t.bfloat16().view(torch.int16).numpy()
