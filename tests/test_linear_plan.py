"""simulst_linear's kernel selection (csrc/gemm_plan.cpp) against what the library launched BEFORE the plan existed.

tests/golden/g26_linear_plan.json was recorded from the parent commit's library: `rows` on an MI355X by tools/linear_plan_sweep.py
under rocprofv3 --kernel-trace (the kernels that actually launched, and each dispatch's LDS size), `floor_sha256` from tests/linear_plan_table.cpp built against
that commit's sources and object files, `vocab` from that commit's own predicates called on the host (not a recorded launch: the
fixture's `recorded_from` says how).  The code under test never wrote it.

The CPU test builds tests/linear_plan_table.cpp against the library's object files (no GPU, nothing is launched) and compares the plan
of every row with the recorded launch; the GPU test holds the BIAS / GELU / RES / F32OUT rows to a torch fp32 product.
"""
import glob
import hashlib
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simulst_amd", "csrc")
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "g26_linear_plan.json")))
F32, BF16 = 0, 1
BIAS, GELU, RES, GLU, EMF_OUT, F32OUT, RES_GELU = range(7)
# position of an override in the program's handle columns (column 0: n_cus)
OPT_COL = {"WEIGHT_STATIONARY": 1, "PANEL_WIDE": 2, "CONV_TILE256": 3, "FUSED_ARGMAX": 4}
ENV_COL = {"SIMULST_PANEL_SPLIT_MIN_ROWS": 5, "SIMULST_PANEL_SPLIT_BLOCKS": 6, "SIMULST_MID_MIN_BLOCKS": 7,
           "SIMULST_MID_NARROW_MIN_ROWS": 8, "SIMULST_SKINNY_MIN_BLOCKS_TALL": 9}
CALL_COLS = ("dtype", "epi", "batches", "rpb", "N", "K", "a_bs", "a_rs", "a_lead", "c_bs", "c_rs", "r_bs", "r_rs", "n_main", "aux_rows",
             "aux_bs", "ln", "packed", "c_hd", "c_hs", "c_th", "c_ts")
REFUSALS = ("fragment-major weights need a decode-step shape", "LN prologue needs a decode-step shape", "LN prologue needs K <= 512",
            "epilogue not available for decode-step shapes", "unknown epilogue")


@pytest.fixture(scope="module")
def table_program(tmp_path_factory):
    objs = sorted(glob.glob(os.path.join(CSRC, "build", "*.o")))
    assert objs, "the library's object files (csrc/build/*.o): run __graft_entry__.build() first"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    d = tmp_path_factory.mktemp("linear_plan")
    main_o, prog = str(d / "main.o"), str(d / "linear_plan_table")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                    "-c", os.path.join(ROOT, "tests", "linear_plan_table.cpp"), "-o", main_o], check=True)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-o", prog, main_o] + objs, check=True)
    return prog


def _handle_cols(n_cus, opts, env):
    h = [-1] * 10
    h[0] = n_cus
    for k, v in opts.items():
        h[OPT_COL[k]] = v
    for k, v in env.items():
        h[ENV_COL[k]] = v
    return h


def _plan_lines(prog, mode, lines):
    out = subprocess.run([prog, mode], input="\n".join(" ".join(map(str, ln)) for ln in lines) + "\n", capture_output=True, text=True,
                         check=True).stdout.splitlines()
    assert len(out) == len(lines)
    return out


def _parse(line):
    w = line.split()
    return w[0], {w[i]: [int(x) for x in w[i + 1:i + 4]] if w[i] == "grid" else int(w[i + 1])
                  for i in range(1, len(w)) if w[i].isalpha() or "_" in w[i]}


def _b(v):
    return "true" if v else "false"


def _expected_kernels(r, fam, p):
    """family + variant flags of the plan -> [(kernel-name prefix, suffix, workgroup size)] as rocprofv3 names the launches"""
    ta = "float" if r["dtype"] == F32 else "__hip_bfloat16"
    if fam == "wstat":
        return [("wstat_kernel<", f", {p['pairs']}>", 1024)]
    if fam == "panel_wide":
        return [("panel_wide_kernel<true>", "", 256)]
    if fam in ("panel", "panel_split"):
        return [("panel_kernel<", f", {_b(p['ln'])}>", 256)]
    if fam == "mid":
        return [(f"mid_kernel<{ta}, ", f", {_b(p['ln'])}, {2 if p['tall'] else 1}>", 256)]
    if fam == "wave_tile":
        return [(f"wave_tile_kernel<{ta}, ", f", {_b(p['ln'])}>", 256)]
    if fam == "skinny":
        split = p["splits"] > 1
        ks = [(f"skinny_kernel<{ta}, ", f", {_b(p['ln'])}, {p['NTs']}, {_b(split)}, {p['MTs']}>", 256)]
        return ks + ([(f"splitk_epilogue_kernel<{ta}, ", ">", 256)] if split else [])
    if fam == "tile256":
        return [("tile256_ring_kernel" if p["ring"] else "tile256_glu_kernel", "", 512)]
    edge = {"tile128": 128, "tile64": 64}[fam]
    return [(f"linear_kernel<{ta}, ", f", {edge}, {edge}, {r['epi'] if r['epi'] != F32OUT else BIAS}>", 256)]


def test_plan_equals_the_recorded_dispatch(table_program):
    rows = FIX["rows"]
    # (the sweep passes a residual only to the epilogues that read one: elsewhere R is null, whatever `mis` says)
    lines = [_handle_cols(r["n_cus"], r["opts"], r["env"]) + [r[k] for k in CALL_COLS] +
             [int(m in r["mis"] and (m != "R" or r["epi"] in (RES, EMF_OUT, RES_GELU))) for m in ("A", "C", "R", "bias")] for r in rows]
    out = _plan_lines(table_program, "plan", lines)
    seen, flags, messages, dynamic = set(), set(), set(), set()
    for r, line in zip(rows, out):
        what = f"row {r['id']} {r}: {line}"
        if r["status"] != 0:
            assert not r["kernels"], what
            assert line == f"refused {r['status']} {r['message']}", what
            messages.add(r["message"])
            continue
        fam, p = _parse(line)
        assert fam != "refused", what
        want = _expected_kernels(r, fam, p)
        assert len(want) == len(r["kernels"]), what
        for (pre, suf, wg), k in zip(want, r["kernels"]):
            assert k["name"].startswith(pre) and k["name"].endswith(suf), what
            assert k["wg"] == [wg, 1, 1], what
        k0 = r["kernels"][0]
        assert k0["grid"] == p["grid"], what
        if p["splits"] > 1:
            M = r["batches"] * r["rpb"]
            assert r["kernels"][1]["grid"] == [(M * r["N"] + 255) // 256, 1, 1], what
        # `lds` is the csv trace's column: the kernel's STATIC allocation, rounded up (0 for wstat and tile256, which have none);
        # `lds_dispatch` is the group-segment size of the recorded dispatch, static + dynamic.  The plan's dynamic request is the
        # dispatch's size where the kernel has no static LDS, and nothing where it has.
        assert k0["lds_dispatch"] <= k0["lds"] or k0["lds"] == 0, what
        assert p["lds"] == (k0["lds_dispatch"] if k0["lds"] == 0 else 0), what
        if p["lds"]:
            dynamic.add(fam)
        seen.add(fam)
        flags |= {(fam, f, p[f]) for f in ("ln", "tall", "ring", "pairs", "MTs", "NTs") if (fam, f) in
                  {("panel", "ln"), ("panel_split", "ln"), ("mid", "ln"), ("mid", "tall"), ("wave_tile", "ln"), ("skinny", "ln"),
                   ("skinny", "MTs"), ("skinny", "NTs"), ("tile256", "ring"), ("wstat", "pairs")}}
        if fam == "skinny":
            flags.add(("skinny", "split", p["splits"] > 1))
    assert seen == {"wstat", "panel_wide", "panel", "panel_split", "mid", "wave_tile", "skinny", "tile256", "tile128", "tile64"}
    want_flags = {(f, "ln", v) for f in ("panel", "panel_split", "mid", "wave_tile", "skinny") for v in (0, 1)}
    want_flags |= {("mid", "tall", 0), ("mid", "tall", 1), ("tile256", "ring", 0), ("tile256", "ring", 1), ("wstat", "pairs", 6), ("wstat", "pairs", 8),
                   ("skinny", "split", False), ("skinny", "split", True)}
    want_flags |= {("skinny", "MTs", v) for v in (1, 2, 4)} | {("skinny", "NTs", v) for v in (1, 2)}
    assert flags == want_flags and dynamic == {"wstat", "tile256"}
    assert all(any(t in m for m in messages) for t in REFUSALS) and len(messages) == len(REFUSALS), messages


def test_vocabulary_argmax_plan_equals_the_recorded_choice(table_program):
    """both sides of the split-panel threshold, of the decode-step row limit and of every shape test of the fused greedy pick, with and
    without a final LayerNorm"""
    rows = FIX["vocab"]
    out = _plan_lines(table_program, "vocab", [r["handle"] + [r["B"], r["V"], r["D"], r["ln"]] for r in rows])
    assert [r["expect"] for r in rows] == out
    assert {o.split()[0] for o in out} == {"none", "mid", "panel_split"}
    # a model without a final LayerNorm: the split panel has no fp32-pair output there, the 64 x 64 tile runs on both sides of its threshold
    assert {(r["B"], o.split()[0]) for r, o in zip(rows, out) if not r["ln"] and r["V"] == 4096 and r["handle"][4:6] == [-1, -1]} >= \
        {(2559, "mid"), (2560, "mid"), (8192, "mid")}
    assert any(r["ln"] and r["B"] == 2560 and o.startswith("panel_split") for r, o in zip(rows, out))


def test_retire_floor_equals_the_recorded_table(table_program):
    """sl_retire_floor_rows for B = 1 .. 9000 at the defaults and at one override of each of the five GEMM thresholds"""
    out = subprocess.run([table_program, "floor"], capture_output=True, check=True).stdout
    assert out.count(b"\n") == 6 * 9000
    for s, B, f in FIX["floor_samples"]:
        assert f"{s} {B} {f}\n".encode() in out
    assert hashlib.sha256(out).hexdigest() == FIX["floor_sha256"]


# ---- GPU: the recorded rows' results against a torch fp32 product -----------------------------------------------------------------------
def _handle(handles, r):
    from simulst_amd import _lib
    from simulst_amd.ops import Ops
    key = json.dumps([r["opts"], r["env"]], sort_keys=True)
    if key not in handles:
        for k, v in r["env"].items():
            os.environ[k] = str(v)
        try:
            handles[key] = Ops()
        finally:
            for k in r["env"]:
                del os.environ[k]
        for k, v in r["opts"].items():
            handles[key].h.set_option(getattr(_lib, "OPT_" + k), v)
    return handles[key]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_recorded_rows_against_torch_fp32(dtype):
    """EVERY BIAS / GELU / RES / F32OUT call of the fixture that launched, exactly as recorded -- batches, overlapping rows, a_lead,
    head-major and tensor-heads outputs, operands off their alignment, the row's handle overrides -- with and without the LayerNorm
    prologue: tolerances and input scaling of test_decode_gemm_row_tiles.  The reference product is taken from the strided view of A
    that the call describes; head-major output is permuted back to rows."""
    import ctypes as C
    import torch
    from simulst_amd._lib import LinearDesc
    tdt = torch.float32 if dtype == F32 else torch.bfloat16
    es = 4 if dtype == F32 else 2
    tol = dict(atol=2e-4, rtol=2e-4) if dtype == F32 else dict(atol=6e-2, rtol=3e-2)
    g = torch.Generator(device="cuda").manual_seed(26)
    rn = lambda *shape: torch.randn(*shape, generator=g, device="cuda")
    geom = lambda r: (r["batches"], r["rpb"], r["N"], r["K"], r["a_bs"], r["a_rs"], r["a_lead"])
    rows = sorted((r for r in FIX["rows"] if r["dtype"] == dtype and r["epi"] in (BIAS, GELU, RES, F32OUT) and r["status"] == 0), key=geom)
    assert len(rows) == sum(1 for r in FIX["rows"] if r["dtype"] == dtype and r["epi"] in (BIAS, GELU, RES, F32OUT) and r["kernels"])
    assert {(r["epi"], r["ln"]) for r in rows} >= {(e, l) for e in (BIAS, GELU, RES) for l in (0, 1)} | {(F32OUT, 1)}
    handles, have = {}, None
    for r in rows:
        B, M, N, K = r["batches"], r["rpb"], r["N"], r["K"]
        key = (geom(r), r["epi"], r["ln"], r["packed"], r["c_hd"], r["c_th"], tuple(r["mis"]), json.dumps([r["opts"], r["env"]], sort_keys=True))
        ops = _handle(handles, r)
        if have != geom(r):                                    # one geometry's operands at a time
            have = geom(r)
            # A as the call describes it: element (b, i, k) at b * a_bs + i * a_rs - a_lead + k, zero in front of a batch's first frame
            store = rn((B - 1) * r["a_bs"] + (M - 1) * r["a_rs"] + K + 16).to(tdt)
            rel = (torch.arange(M, device="cuda") * r["a_rs"] - r["a_lead"])[:, None] + torch.arange(K, device="cuda")[None, :]
            idx = (torch.arange(B, device="cuda") * r["a_bs"])[:, None, None] + rel[None]
            Aeff = torch.where((rel >= 0)[None], store[idx.clamp(min=0)], torch.zeros((), dtype=tdt, device="cuda")).reshape(B * M, K)
            W = (rn(N, K) / K ** 0.5).to(tdt)
            Wp = None
            b, res = rn(N), rn(B * M, N).to(tdt)
            gam, bet = torch.rand(K, generator=g, device="cuda") + 0.5, rn(K) * 0.1
            ref = Aeff.float() @ W.float().t() + b
            refn = torch.nn.functional.layer_norm(Aeff.float(), (K,), gam, bet).to(tdt).float() @ W.float().t() + b
        if r["packed"] and Wp is None:
            Wp = ops.pack_fragment_major(W)
        # operands off their alignment, as recorded: A / C / R start 8 bytes past a 16-byte boundary, the bias 2 bytes past a float's
        mis = r["mis"]
        keep = []

        def at(t, off):                                        # the same bytes `off` bytes into a fresh (256-byte aligned) allocation
            raw = t.contiguous().view(-1).view(torch.uint8)
            buf = torch.zeros(raw.numel() + 32, dtype=torch.uint8, device="cuda")
            buf[off:off + raw.numel()] = raw
            keep.append(buf)
            return buf.data_ptr() + off
        pA = at(store, 8) if "A" in mis else store.data_ptr()
        pB = at(b, 2) if "bias" in mis else b.data_ptr()
        want = refn if r["ln"] else ref
        pR = 0
        if r["epi"] == RES:
            pR = at(res, 8) if "R" in mis else res.data_ptr()
            want = want + res.float()
        if r["epi"] == GELU:
            want = torch.nn.functional.gelu(want)
        odt = torch.float32 if r["epi"] == F32OUT else tdt
        out = torch.zeros(r["c_elems"] + 16, dtype=odt, device="cuda")
        pC = out.data_ptr() + (8 if "C" in mis else 0)
        d = LinearDesc(B, M, N, K, r["a_bs"], r["a_rs"], r["a_lead"], r["c_bs"], r["c_rs"], r["r_bs"], r["r_rs"], r["epi"], dtype, 1.0, 0, 0, 0,
                       gam.data_ptr() if r["ln"] else None, bet.data_ptr() if r["ln"] else None, r["packed"],
                       r["c_hd"], r["c_hs"], r["c_th"], r["c_ts"])
        ops.h.check(ops.lib.simulst_linear(ops.h.ptr, C.byref(d), C.c_void_p(pA), C.c_void_p((Wp if r["packed"] else W).data_ptr()),
                                           C.c_void_p(pB), C.c_void_p(pR), C.c_void_p(pC), C.c_void_p(0)), f"row {r['id']}")
        osz = out.element_size()
        y = out.view(torch.uint8)[8:8 + r["c_elems"] * osz].clone().view(odt) if "C" in mis else out[:r["c_elems"]]
        if r["c_hd"]:                                          # [head][row][c_hd] (tensors of c_th heads follow each other) -> rows
            assert B == 1 and r["c_rs"] == r["c_hd"] and r["c_hs"] == M * r["c_hd"] and (not r["c_th"] or r["c_ts"] == r["c_th"] * r["c_hs"])
            y = y.view(N // r["c_hd"], M, r["c_hd"]).permute(1, 0, 2).reshape(M, N)
        else:
            assert r["c_rs"] == N and r["c_bs"] == M * N
            y = y.view(B * M, N)
        err = (y.float() - want).abs()
        print(f"row {r['id']} B={B} M={M} N={N} K={K} a_rs={r['a_rs']} epi={r['epi']} ln={r['ln']} packed={r['packed']} c_hd={r['c_hd']} "
              f"mis={mis}: max abs err {float(err.max()):.3e}")
        torch.testing.assert_close(y.float(), want, **tol, msg=lambda m: f"row {r['id']} {key}: {m}")
