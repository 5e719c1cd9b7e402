#!/usr/bin/env python3
"""simulst_linear at every switch point of its kernel selection (csrc/gemm_plan.cpp) and the neighbours on either side.

  run    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/linear_plan_sweep.py run OUT.json
         calls simulst_linear over ROWS on seeded inputs; per row: the call, the handle's n_cus and overrides, status + message of a
         refused call, SHA-256 of the output bytes.  Two fills (output, aux) precede every call: they separate the rows in the trace
         (the inputs are made on the host, so no other fill runs).
  merge  python3 tools/linear_plan_sweep.py merge OUT.json DIR FIXTURE.json
         adds to every row the kernels that launched (name, grid in workgroups, workgroup size, LDS bytes) from the trace under DIR.
  lds    python3 tools/linear_plan_sweep.py lds FIXTURE.json RESULTS.json
         a second `run` of the same rows under rocprofv3 --kernel-trace --output-format json: adds every dispatch's group-segment size
         (static + dynamic LDS) as `lds_dispatch`; the csv's LDS column is the kernel's static allocation only.
  cmp    python3 tools/linear_plan_sweep.py cmp A.json B.json      equal kernels and equal output bytes, row by row

tests/golden/g26_linear_plan.json is `merge`'s output for the library of the commit BEFORE the plan existed; tests/test_linear_plan.py
holds the plan to it.  SIMULST_LIB_PATH selects the library as everywhere.
"""
import csv
import glob
import hashlib
import json
import os
import re
import sys

F32, BF16 = 0, 1
BIAS, GELU, RES, GLU, EMF_OUT, F32OUT, RES_GELU = range(7)
OPT_NAMES = ("WEIGHT_STATIONARY", "PANEL_WIDE", "CONV_TILE256", "FUSED_ARGMAX")
LIB_KERNELS = ("linear_kernel", "skinny_kernel", "splitk_epilogue_kernel", "mid_kernel", "wave_tile_kernel", "panel_kernel",
               "panel_wide_kernel", "wstat_kernel", "tile256_")


def row(dtype, epi, M, N, K, *, packed=None, ln=False, batches=1, a_rs=None, a_bs=None, a_lead=0, mis=(), opts=None, env=None,
        c_hd=0, c_hs=0, c_th=0, c_ts=0, note=""):
    """M rows per batch.  packed defaults to bf16.  mis: which of "A", "C", "R", "bias" start off their natural alignment."""
    packed = (dtype == BF16) if packed is None else packed
    a_rs = K if a_rs is None else a_rs
    a_bs = (M * a_rs + K + a_lead + 7) // 8 * 8 if a_bs is None else a_bs
    n_out = N // 2 if epi == GLU else N
    r = dict(dtype=dtype, epi=epi, batches=batches, rpb=M, N=N, K=K, a_bs=a_bs, a_rs=a_rs, a_lead=a_lead, packed=int(packed), ln=int(ln),
             c_hd=c_hd, c_hs=c_hs, c_th=c_th, c_ts=c_ts, mis=list(mis), opts=opts or {}, env=env or {}, note=note)
    if c_hd:                                       # [batch][tensor][head][row][c_hd]
        heads = N // c_hd
        r.update(c_rs=c_hd, c_bs=heads * M * c_hd, c_elems=batches * heads * M * c_hd)
    else:
        r.update(c_rs=n_out, c_bs=M * n_out, c_elems=batches * M * n_out)
    r.update(r_rs=N, r_bs=M * N, n_main=0, aux_rows=0, aux_bs=0)
    if epi == EMF_OUT:
        r.update(n_main=M - 8, aux_rows=8, aux_bs=8 * N)
    return r


def rows():
    R = []
    D = 256
    # ---- row counts of decode-step shapes (bf16, fragment-major): 255 / 256 skinny -> tiles, 2559 / 2560 split panel, 3071 / 3072 narrow
    for M in (255, 256):
        for N in (768, 256):
            for ln in (False, True):
                R.append(row(BF16, BIAS, M, N, D, ln=ln))
        R.append(row(F32, GELU, M, 768, 128))
        R.append(row(F32, RES, M, 256, 128, ln=True))
    for M in (2559, 2560):
        for epi, ln in ((BIAS, True), (GELU, True), (F32OUT, True), (BIAS, False), (GELU, False), (RES, False), (RES, True), (F32OUT, False),
                        (RES_GELU, False)):
            R.append(row(BF16, epi, M, 2048, D, ln=ln))
        R.append(row(BF16, BIAS, M, 768, D, ln=True, note="too narrow for two column steps per workgroup"))
        R.append(row(BF16, BIAS, M, 2048, D, packed=False) if M <= 2048 else row(BF16, BIAS, M, 2048, 288, note="K over the panel's"))
        R.append(row(BF16, BIAS, M, 1536, D, c_hd=64, c_hs=M * 64, note="head-major"))
        R.append(row(BF16, BIAS, M, 1536, D, c_hd=64, c_hs=M * 64, c_th=8, c_ts=8 * M * 64, note="tensor heads"))
    for M in (3071, 3072):
        for epi, ln in ((RES, False), (BIAS, True), (F32OUT, True)):
            R.append(row(BF16, epi, M, 256, D, ln=ln))
        R.append(row(BF16, BIAS, M, 48, D))
        R.append(row(BF16, BIAS, M, 64, D))
        R.append(row(BF16, RES, M, 256, 288, note="nine k-steps"))
    # ---- 2048 / 2049 rows with row-major weights, 8191 / 8192 / 8193 with fragment-major ones
    for M in (2048, 2049):
        for dtype in (BF16, F32):
            R.append(row(dtype, BIAS, M, 512, 128, packed=False))
            R.append(row(dtype, GELU, M, 512, 128, packed=False, ln=True))
    for M in (8191, 8192, 8193):
        for epi, N, ln in ((EMF_OUT, 256, False), (BIAS, 768, False), (BIAS, 512, False), (BIAS, 1024, False), (BIAS, 576, False),
                           (BIAS, 384, False), (BIAS, 1280, False), (BIAS, 528, False), (GELU, 1280, False), (BIAS, 768, True),
                           (GELU, 512, True), (RES, 256, False), (RES, 768, False), (F32OUT, 512, True), (F32OUT, 512, False),
                           (RES_GELU, 512, False), (BIAS, 256, False)):
            R.append(row(BF16, epi, M, N, D, ln=ln))
        R.append(row(BF16, BIAS, M, 512, D, packed=False))
        R.append(row(BF16, BIAS, M, 768, D, c_hd=64, c_hs=M * 64, note="head-major"))
        R.append(row(BF16, BIAS, M, 768, 128, note="short contraction"))
    for opts in ({"WEIGHT_STATIONARY": 0}, {"WEIGHT_STATIONARY": 0, "PANEL_WIDE": 0}, {"PANEL_WIDE": 0}):
        R.append(row(BF16, BIAS, 8193, 768, D, opts=opts))
        R.append(row(BF16, EMF_OUT, 8193, 256, D, opts=opts))
    for mis in ("A", "C", "R", "bias"):
        R.append(row(BF16, BIAS, 8193, 768, D, mis=(mis,)))
        R.append(row(BF16, EMF_OUT, 8193, 256, D, mis=(mis,)))
        R.append(row(BF16, BIAS, 8193, 1280, D, mis=(mis,)))
    # ---- 4095 / 4096 rows with the Emformer epilogue, and what else the tall panels take
    for M in (4095, 4096):
        for packed in (True, False):
            R.append(row(BF16, EMF_OUT, M, 256, D, packed=packed))
        R.append(row(BF16, BIAS, 1, 256, D, batches=M, note="one row per batch"))
    R.append(row(BF16, EMF_OUT, 4096, 256, D, a_rs=128, note="overlapping rows"))
    R.append(row(BF16, EMF_OUT, 4096, 256, D, a_lead=64, note="a_lead"))
    R.append(row(BF16, EMF_OUT, 4096, 256, 288))
    R.append(row(BF16, EMF_OUT, 4096, 248, D, packed=False))
    R.append(row(BF16, EMF_OUT, 4096, 248, D, note="N % 16"))
    R.append(row(F32, EMF_OUT, 600, 256, 64))
    # ---- 512 / 513 rows outside the decode-step shapes: 64 x 64 against 128 x 128 tiles
    for M in (512, 513):
        for dtype in (F32, BF16):
            R.append(row(dtype, BIAS, M, 200, 64, packed=False, a_rs=32, note="overlapping rows"))
            R.append(row(dtype, RES_GELU, M, 200, 64, packed=False, a_lead=32, note="a_lead"))
            R.append(row(dtype, GLU, M, 128, 64, packed=False))
            R.append(row(dtype, EMF_OUT, M, 128, 64, packed=False))
            R.append(row(dtype, F32OUT, M, 72, 64, packed=False, a_rs=32))
        R.append(row(BF16, BIAS, M, 256, 64, a_rs=32, note="fragment-major, overlapping rows"))
        R.append(row(BF16, GELU, M, 200, 64, packed=False, a_rs=32, ln=True))
    # ---- block-count rules
    for M in (320, 384):
        R.append(row(BF16, BIAS, M, 512, D))
    R.append(row(BF16, BIAS, 320, 512, D, env={"SIMULST_MID_MIN_BLOCKS": 40}))
    for M, N in ((64, 4096), (64, 4064), (48, 3200), (48, 2720), (16, 256), (130, 4096), (33, 1040)):
        R.append(row(BF16, BIAS, M, N, D))
        R.append(row(F32, F32OUT, M, N, 128, ln=True))
    for M in (1472, 1473, 1536):
        R.append(row(BF16, RES, M, 256, 2048))
    R.append(row(BF16, RES, 1472, 256, 2048, env={"SIMULST_SKINNY_MIN_BLOCKS_TALL": 184}))
    R.append(row(BF16, RES, 256, 256, 2048, note="M == N"))
    for N in (1024, 1040):
        R.append(row(BF16, RES, 64, N, 4096))
    # ---- contraction depths: 8 and 16 k-steps and one more, 4096 and the vector below it
    for dtype, ks in ((BF16, 32), (F32, 16)):
        for K in (8 * ks, 9 * ks):
            R.append(row(dtype, BIAS, 512, 768, K, ln=True))
            R.append(row(dtype, BIAS, 512, 768, K))
            R.append(row(dtype, GELU, 512, 256, K, ln=True))
            R.append(row(dtype, GELU, 2048, 256, K, ln=True, note="64-row tiles keep two k-steps per wave"))
        for K in (16 * ks, 17 * ks):
            R.append(row(dtype, BIAS, 64, 256, K, ln=True))
            R.append(row(dtype, F32OUT, 300, 512, K, ln=True))
        g = 32 // (2 if dtype == BF16 else 4)
        for K in (4096 - g, 4096, 8192):
            R.append(row(dtype, RES, 64, 256, K))
            R.append(row(dtype, BIAS, 64, 256, K, ln=True))
        R.append(row(dtype, BIAS, 300, 512, 8 * ks + g, packed=False, note="K % k-step"))
    R.append(row(BF16, BIAS, 300, 512, 272, note="fragment-major, K % 64 bytes"))
    # ---- widths
    for N in (63, 64, 511, 512):
        R.append(row(BF16, BIAS, 2048, N, D, packed=False))
        R.append(row(F32, BIAS, 512, N, 128, packed=False))
    R.append(row(BF16, BIAS, 512, 63, D, note="fragment-major, N % 16"))
    R.append(row(BF16, BIAS, 512, 496, D))
    # ---- 256 x 256 GLU tiles
    for M in (8191, 8192):
        for N in (512, 384):
            R.append(row(BF16, GLU, M, N, 64, packed=False))
    for v in (0, 1, 2):
        R.append(row(BF16, GLU, 2048, 512, 64, packed=False, batches=4, a_rs=32, a_lead=32, opts={"CONV_TILE256": v}, note="overlapping rows, a_lead"))
    R.append(row(BF16, GLU, 8192, 512, 64, packed=False, mis=("C",)))
    R.append(row(F32, GLU, 8192, 512, 64, packed=False))
    R.append(row(BF16, GLU, 8192, 512, 64, note="fragment-major"))
    # ---- the remaining thresholds, each moved once
    R.append(row(BF16, BIAS, 2048, 2048, D, ln=True, env={"SIMULST_PANEL_SPLIT_MIN_ROWS": 2048}))
    R.append(row(BF16, BIAS, 2560, 2048, D, ln=True, env={"SIMULST_PANEL_SPLIT_BLOCKS": 20}))
    R.append(row(BF16, BIAS, 2560, 2048, D, ln=True, env={"SIMULST_PANEL_SPLIT_BLOCKS": 128}))
    R.append(row(BF16, RES, 1024, 256, D, env={"SIMULST_MID_NARROW_MIN_ROWS": 1024, "SIMULST_MID_MIN_BLOCKS": 16}))
    R.append(row(BF16, RES, 3072, 256, D, opts={"FUSED_ARGMAX": 0}))
    # ---- an epilogue the library does not know, on a decode-step shape and on a tiled one
    R.append(row(BF16, 7, 64, 256, D))
    R.append(row(BF16, 7, 300, 512, D, note="64 x 64 decode tile"))
    R.append(row(F32, 7, 512, 200, 64, packed=False, a_rs=32))
    for i, r in enumerate(R):
        r["id"] = i
    return R


def run(out_path):
    import ctypes as C
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from simulst_amd import _lib
    from simulst_amd._lib import LinearDesc
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(26)
    n_in, n_res = 18 << 20, 18 << 20
    pool = {BF16: (torch.randn(n_in, generator=g) * 0.5).to(torch.bfloat16).to(dev), F32: (torch.randn(n_in, generator=g) * 0.5).to(dev)}
    res = {BF16: torch.randn(n_res, generator=g).to(torch.bfloat16).to(dev), F32: torch.randn(n_res, generator=g).to(dev)}
    vec = torch.randn(3, 8192 + 64, generator=g).to(dev)                      # bias, gamma, beta
    out = torch.empty((18 << 20) * 4 + 256, dtype=torch.uint8, device=dev)
    aux = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    lib = _lib.load()
    handles = {}
    R = rows()
    for r in R:
        key = json.dumps([r["opts"], r["env"]], sort_keys=True)
        if key not in handles:
            for k, v in r["env"].items():
                os.environ[k] = str(v)
            try:
                h = _lib.Handle()
            finally:
                for k in r["env"]:
                    del os.environ[k]
            for k, v in r["opts"].items():
                h.set_option(getattr(_lib, "OPT_" + k), v)
            handles[key] = h
        h = handles[key]
        es = 2 if r["dtype"] == BF16 else 4
        os_ = 4 if (r["epi"] == F32OUT or r["dtype"] == F32) else 2
        a_need = (r["batches"] - 1) * r["a_bs"] + r["rpb"] * r["a_rs"] + r["K"]
        assert a_need + 64 <= n_in and r["N"] * r["K"] + 64 <= n_in and r["batches"] * r["rpb"] * r["N"] + 64 <= n_res, r
        c_bytes = r["c_elems"] * os_
        assert c_bytes + 64 <= out.numel() and r["N"] <= 8192 and r["K"] <= 8192
        mis = r["mis"]
        # a_lead elements in front of a batch's first row are never read (zero frames), the pointer still has to allow the subtraction
        pA = pool[r["dtype"]].data_ptr() + 64 * es + (8 if "A" in mis else 0)
        pW = pool[r["dtype"]].data_ptr() + 128 * es
        pR = res[r["dtype"]].data_ptr() + (8 if "R" in mis else 0)
        pB = vec[0].data_ptr() + (2 if "bias" in mis else 0)
        pC = out.data_ptr() + (8 if "C" in mis else 0)
        out[:c_bytes + 64].zero_()
        aux.zero_()
        d = LinearDesc(r["batches"], r["rpb"], r["N"], r["K"], r["a_bs"], r["a_rs"], r["a_lead"], r["c_bs"], r["c_rs"], r["r_bs"], r["r_rs"],
                       r["epi"], r["dtype"], 1.0, r["n_main"], r["aux_rows"], r["aux_bs"],
                       vec[1].data_ptr() if r["ln"] else None, vec[2].data_ptr() if r["ln"] else None, r["packed"],
                       r["c_hd"], r["c_hs"], r["c_th"], r["c_ts"])
        needs_r = r["epi"] in (RES, EMF_OUT, RES_GELU)
        rc = lib.simulst_linear(h.ptr, C.byref(d), C.c_void_p(pA), C.c_void_p(pW), C.c_void_p(pB), C.c_void_p(pR if needs_r else 0),
                                C.c_void_p(pC), C.c_void_p(aux.data_ptr() if r["epi"] == EMF_OUT else 0))
        r["n_cus"] = n_cus
        r["status"] = rc
        r["message"] = lib.simulst_last_error(h.ptr).decode() if rc else ""
        torch.cuda.synchronize()
        hsh = hashlib.sha256(out[:c_bytes + 64].cpu().numpy().tobytes())
        if r["epi"] == EMF_OUT:
            hsh.update(aux.cpu().numpy().tobytes())
        r["sha256"] = hsh.hexdigest()
    json.dump({"rows": R}, open(out_path, "w"), indent=0)
    print(f"{len(R)} rows, {sum(1 for r in R if r['status'])} refused -> {out_path}")


def merge(run_path, trace_dir, out_path):
    R = json.load(open(run_path))["rows"]
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    toks = []
    for t in sorted(csv.DictReader(open(files[0])), key=lambda t: int(t["Start_Timestamp"])):
        name = t["Kernel_Name"]
        if any(k in name for k in LIB_KERNELS):
            wg = [int(t["Workgroup_Size_" + a]) for a in "XYZ"]
            grid = [int(t["Grid_Size_" + a]) // w for a, w in zip("XYZ", wg)]
            toks.append(dict(name=_short(name), grid=grid, wg=wg, lds=int(t["LDS_Block_Size"])))
        elif "FillFunctor" in name:                                          # (device-to-host copies show up as kernels too: ignored)
            toks.append(None)
    assert sum(1 for t in toks if t is None) == 2 * len(R) and toks[0] is None, "two fills per row and nothing else in front"
    i = 0
    for r in R:
        assert toks[i] is None and toks[i + 1] is None, (r["id"], toks[i:i + 2])
        i += 2
        r["kernels"] = []
        while i < len(toks) and toks[i] is not None:
            r["kernels"].append(toks[i])
            i += 1
        assert bool(r["kernels"]) == (r["status"] == 0), r
    assert i == len(toks)
    json.dump({"rows": R}, open(out_path, "w"), indent=0)
    print(f"{len(R)} rows, {sum(len(r['kernels']) for r in R)} launches -> {out_path}")


def _short(name):
    m = re.match(r"(?:void )?(?:\(anonymous namespace\)::)?([\w:]+(?:<.*>)?)\(", name)
    return m.group(1) if m else name


def lds(fixture_path, results_path):
    """The csv trace's LDS column is a kernel's STATIC allocation.  rocprofv3 --output-format json keeps the group-segment size of every
    DISPATCH (static + dynamic): from the results file of a `run` of the same rows, add it to every recorded kernel as `lds_dispatch`."""
    fx = json.load(open(fixture_path))
    d = json.load(open(results_path))
    if isinstance(d, dict):                                    # rocprofv3's own file; a list: (name, start, group_segment_size, wg, grid) already
        r = d["rocprofiler-sdk-tool"][0]
        syms = {k["kernel_id"]: k for k in r["kernel_symbols"]}
        d = [dict(name=syms[x["dispatch_info"]["kernel_id"]].get("formatted_kernel_name") or syms[x["dispatch_info"]["kernel_id"]]["kernel_name"],
                  start=x["start_timestamp"], group_segment_size=x["dispatch_info"]["group_segment_size"],
                  wg=x["dispatch_info"]["workgroup_size"], grid=x["dispatch_info"]["grid_size"]) for x in r["buffer_records"]["kernel_dispatch"]]
    ours = [x for x in sorted(d, key=lambda x: x["start"]) if any(k in x["name"] for k in LIB_KERNELS)]
    recorded = [k for r in fx["rows"] for k in r["kernels"]]
    assert len(ours) == len(recorded), (len(ours), len(recorded))
    for k, x in zip(recorded, ours):
        assert k["name"] == _short(x["name"]) and k["grid"] == [x["grid"][a] // x["wg"][a] for a in "xyz"], (k, x)
        k["lds_dispatch"] = x["group_segment_size"]
    open(fixture_path, "w").write(json.dumps(fx, indent=0) + "\n")
    print(f"{len(recorded)} launches, {sum(1 for k in recorded if k['lds_dispatch'] > k['lds'])} with more than their static LDS")


def cmp(a_path, b_path):
    A, B = json.load(open(a_path))["rows"], json.load(open(b_path))["rows"]
    assert len(A) == len(B)
    same = lambda ka, kb: [{f: v for f, v in k.items() if f != "lds_dispatch"} for k in ka] == [{f: v for f, v in k.items() if f != "lds_dispatch"} for k in kb]
    bad_k = [a["id"] for a, b in zip(A, B) if not same(a["kernels"], b["kernels"]) or a["status"] != b["status"] or a["message"] != b["message"]]
    bad_o = [a["id"] for a, b in zip(A, B) if a["sha256"] != b["sha256"]]
    print(json.dumps(dict(rows=len(A), launches=sum(len(a["kernels"]) for a in A), refused=sum(1 for a in A if a["status"]),
                          rows_with_other_kernels_or_status=bad_k, rows_with_other_output_bytes=bad_o)))
    return 1 if bad_k or bad_o else 0


if __name__ == "__main__":
    sys.exit({"run": run, "merge": merge, "lds": lds, "cmp": cmp}[sys.argv[1]](*sys.argv[2:]))
