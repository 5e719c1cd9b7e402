"""simulst_linear's ten kernel families against the float64 reference of tests/linear_ref.py, through the C ABI, at their tile edges.

Every case of tests/linear_cases.py is one simulst_linear call exactly as its descriptor says (tests/test_linear_ref_cpu.py asserts that
each reaches the family and variant it declares).  The reference runs on the CPU.  Per addressed output element, with
S = sum_k |a_k| |w_k| (|z_k| for a LayerNorm-ed row), b the bias and r the residual element:

  fp32 path    (K + 3) 2^-23 (S + |b| + |r|).  bf16 x bf16 products are exact in fp32; K - 1 additions of the accumulation in any order
               (each partial sum is at most S: error (K - 1) 2^-24 S to first order, the term allows twice that for the products of the
               fp32 path and the second order), the bias add, the residual add and one spare.
  split-K      + splits 2^-24 S: every split's partial sum is rounded once more when it is stored.
  LayerNorm    the reference keeps z unrounded; the kernel's z carries the error of an fp32 LayerNorm,
               e_ln(k) = 4 e32 + 2^-22 (|gamma_k| |zhat_k| + |beta_k|) -- the front-end LayerNorm's bound, e32 = the largest error of the
               same formula in torch float32 on the CPU against float64 over the case's rows -- and is rounded to the operand dtype:
               + sum_k |w_k| (u |z_k| + e_ln(k)), u = 2^-8 (bf16) or 2^-24 (fp32).
  activations  gelu: 1.13 x (the above) + e_act (1.13 = sup |gelu'|); tanh: 1 x + e_act; GLU s v sigmoid(g): |s| (E_v sigmoid(g) +
               |v| (E_g / 4 + e_act)) + 3 * 2^-24 |ref| (product rule, sigmoid' <= 1 / 4, the fp32 products).  e_act is measured as e_gelu
               in test_hip_front_end.py: 4 x the largest error of torch's fp32 CPU function against float64 over the case's
               pre-activations and 2049 points spanning them; in bf16 the GELU is at least the 7.1e-7 csrc/common.h states for its fit.
  store        + 2^-8 |ref| for bf16 outputs, + 2^-24 |ref| for fp32 ones (F32OUT is fp32 whatever the operands).
  EXACT class  operands are small integers and quarters: every partial sum is exact in fp32 in any order.  BIAS / RES / F32OUT (and the
               main rows of EMF_OUT) must EQUAL the reference rounded once to the output dtype, bit for bit; activations are held to
               e_act + u |ref|.

Also asserted, in every case: every element of C and aux that the reference does not list keeps its NaN sentinel bits (the gaps between
N and c_row_stride, the undropped last summary, 4096 elements in front and behind); no NaN reaches an addressed output although every
element of A, W's tail, the bias' tail and R that the call must not use is NaN; three runs of every split-K and weight-stationary case
give identical bits; simulst_pack_fragment_major equals the header's index map bit for bit.

Deviations from the issue's recipe, each about the test and none about a kernel (reasons in tests/linear_cases.py): W carries
1 / sqrt(K); the tall rows are x2 instead of x1000 under GELU / GLU / RES_GELU; LayerNorm cases add rows scaled by 2^-8 so that eps is
visible; the bf16 GELU's e_act is the larger of the measured one and the fit's; the GLU's relative term is (3 * 2^-24 + u) |ref|, in
the EXACT class too, where the issue has e_act + u |ref|: scale * v * sigmoid(g) is two fp32 products of rounded factors besides the
store, which a correct fp32 kernel cannot avoid (4 u instead of 1 u in fp32, invisible beside 2^-8 in bf16).  No caller in
simulst_amd/*.py passes the same tensor as C and R (ops.linear's callers give a fresh `out` or another buffer), so there is no
aliasing case.

Measured on an MI355X (worst |got - ref| / bound, RANDOM class, then the EXACT class in brackets: 0 = bit-equal throughout, else the
activations against e_act + u |ref|).  No test takes more than 1.1 s, the file (32 tests) 7.5 s.  Constants from the CPU of the same run: e_gelu
2.0e-6 .. 4.6e-6, e_tanh 1.2e-7, e_sigmoid 3.0e-7 .. 3.5e-7, e32 3.2e-7 .. 1.1e-6.
  wstat       bf16 0.988 (0.633)                        panel_wide  bf16 0.988 (0)
  panel       bf16 0.992 (0.996)                        panel_split bf16 0.995 (0)
  mid         fp32 0.112 (0.140)   bf16 0.995 (0.996)   wave_tile   fp32 0.097 (0.140)   bf16 0.991 (0.996)
  skinny      fp32 0.210 (0.140)   bf16 0.995 (0.988)   tile256     bf16 0.994 (0.996)
  tile128     fp32 0.087 (0.213)   bf16 0.992 (0.996)   tile64      fp32 0.150 (0.161)   bf16 0.981 (0.966)
bf16 figures near 1 are the store's rounding alone.  Every derived term held untouched; every guard element was intact, no NaN reached
an output, every EXACT BIAS / RES / F32OUT case was bit-equal, and the split-K and weight-stationary cases repeated their bits: nothing
was found in the kernels and none changed.
"""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

import linear_cases as lc
import linear_ref as lr
from linear_ref import BF16, F32, F32OUT

pytestmark = pytest.mark.gpu

FRONT = 4096                          # sentinel elements in front of and behind C / aux
PAD = 1 << 16                         # further NaN elements behind A and W on the device
WORST, HANDLES = {}, {}
T0 = time.time()


def _handle(c):
    from simulst_amd import _lib
    from simulst_amd.ops import Ops
    key = repr((sorted(c["opts"].items()), sorted(c["env"].items())))
    if key not in HANDLES:
        for k, v in c["env"].items():
            os.environ[k] = str(v)
        try:
            HANDLES[key] = Ops()
        finally:
            for k in c["env"]:
                del os.environ[k]
        for k, v in c["opts"].items():
            HANDLES[key].h.set_option(getattr(_lib, "OPT_" + k), v)
    return HANDLES[key]


def _chunks():
    """the cases of a family and dtype, in runs of at most 16 cases or ~4e9 multiply-adds of reference"""
    out = []
    for fam in lc.FAMILIES:
        for dtype in (F32, BF16):
            run, cost = [], 0
            for c in (c for c in lc.CASES if c["family"] == fam and c["dtype"] == dtype):
                d = c["d"]
                w = d["M_batches"] * d["rows_per_batch"] * d["N"] * (d["K"] + 64)
                if run and (len(run) == 16 or cost + w > 4e9):
                    out.append(run)
                    run, cost = [], 0
                run.append(c)
                cost += w
            if run:
                out.append(run)
    return out


CHUNKS = _chunks()


def _chunk_id(run):
    return f"{run[0]['family']}-{'f32' if run[0]['dtype'] == F32 else 'bf16'}-{run[0]['name'].split('-', 2)[2]}"


def _dev(t, off, keep, tail=0):
    """the tensor's bytes `off` bytes into a fresh 256-byte aligned device allocation (+ `tail` NaN elements): its address"""
    raw = t.contiguous().view(-1).view(torch.uint8)
    fill = torch.full((tail,), float("nan"), dtype=t.dtype).view(torch.uint8) if tail else raw[:0]
    buf = torch.zeros(raw.numel() + fill.numel() + 32, dtype=torch.uint8, device="cuda")
    buf[off:off + raw.numel()] = raw.cuda()
    buf[off + raw.numel():off + raw.numel() + fill.numel()] = fill.cuda()
    keep.append(buf)
    return buf.data_ptr() + off


def _out_buffer(n, out_f32, off, keep):
    """FRONT + n + FRONT sentinel elements (+ the 8 bytes of a misaligned start); -> (device tensor of bits, address of element 0)"""
    es = 4 if out_f32 else 2
    bits = torch.from_numpy(lc.sentinel_like(2 * FRONT + n + 8, out_f32)).cuda()
    keep.append(bits)
    return bits, bits.data_ptr() + FRONT * es + off


def _read(bits, n, out_f32, off):
    es = 4 if out_f32 else 2
    raw = bits.view(torch.uint8)[off:off + (2 * FRONT + n) * es].cpu().clone()
    return raw.view(torch.int32 if out_f32 else torch.int16).numpy()


def _launch(ops, c, o, ptr, pC, pAux):
    from simulst_amd._lib import LinearDesc
    d = c["d"]
    desc = LinearDesc(d["M_batches"], d["rows_per_batch"], d["N"], d["K"], d["a_batch_stride"], d["a_row_stride"], d["a_lead"],
                      d["c_batch_stride"], d["c_row_stride"], d["r_batch_stride"], d["r_row_stride"], d["epilogue"], c["dtype"], d["scale"],
                      d["n_main"], d["aux_rows"], d["aux_batch_stride"], ptr["gamma"] or None, ptr["beta"] or None, d["w_fragment_major"],
                      d["c_head_dim"], d["c_head_stride"], d["c_tensor_heads"], d["c_tensor_stride"])
    ops.h.check(ops.lib.simulst_linear(ops.h.ptr, C.byref(desc), C.c_void_p(ptr["A"]), C.c_void_p(ptr["W"]), C.c_void_p(ptr["bias"]),
                                       C.c_void_p(ptr["R"]), C.c_void_p(pC), C.c_void_p(pAux)), c["name"])
    torch.cuda.synchronize()


def _run_case(c):
    ops = _handle(c)
    o = lc.operands(c)
    streams, mags = lc.run_reference(c, o)
    bnd = lc.bounds(c, streams, mags, lc.measured_constants(c, o, mags))
    d, mis, keep = c["d"], c["mis"], []
    es = 4 if c["dtype"] == F32 else 2
    ptr = dict(A=_dev(o["A"], 8 if "A" in mis else 0, keep, PAD) + o["a0"] * es, W=_dev(o["W"], 0, keep, PAD),
               bias=_dev(o["bias"], 2 if "bias" in mis else 0, keep), R=0, gamma=0, beta=0)
    if o["R"] is not None:
        ptr["R"] = _dev(o["R"], 0, keep) + o["r0"] * es
    if c["ln"]:
        ptr["gamma"], ptr["beta"] = _dev(o["gamma"], 0, keep), _dev(o["beta"], 0, keep)
    out_f32 = c["dtype"] == F32 or d["epilogue"] == F32OUT
    size = {name: int(st["idx"].max()) + 1 if st["idx"].size else 1 for name, st in streams.items()}
    offC = 8 if "C" in mis else 0
    cbits, pC = _out_buffer(size["C"], out_f32, offC, keep)
    abits, pAux = _out_buffer(size["aux"], out_f32, 0, keep) if "aux" in streams else (None, 0)
    _launch(ops, c, o, ptr, pC, pAux)
    got = {"C": _read(cbits, size["C"], out_f32, offC)}
    if abits is not None:
        got["aux"] = _read(abits, size["aux"], out_f32, 0)
    if c["flags"].get("split") or c["family"] == "wstat":     # the same bits, run after run
        for _ in range(2):
            _launch(ops, c, o, ptr, pC, pAux)
            assert np.array_equal(_read(cbits, size["C"], out_f32, offC), got["C"]), (c["name"], "C differs between runs")
            if abits is not None:
                assert np.array_equal(_read(abits, size["aux"], out_f32, 0), got["aux"]), (c["name"], "aux differs between runs")
    key = (c["family"], "bf16" if c["dtype"] == BF16 else "f32")
    for name, st in streams.items():
        bits, idx = got[name], st["idx"].ravel() + FRONT
        untouched = np.ones(bits.size, bool)
        untouched[idx] = False
        sent = lc.sentinel_like(1, out_f32)[0]
        bad = np.flatnonzero(untouched & (bits != sent))
        assert bad.size == 0, (c["name"], name, "written outside the addressed elements, first offsets", (bad[:8] - FRONT).tolist())
        vals = torch.from_numpy(bits[idx].copy())
        vals = (vals.view(torch.float32) if out_f32 else vals.view(torch.bfloat16)).double().numpy()
        assert np.isfinite(vals).all(), (c["name"], name, "NaN / inf in an addressed output (or an element not written), first",
                                        st["idx"].ravel()[np.flatnonzero(~np.isfinite(vals))[:8]].tolist())
        ref = st["val"].ravel()
        if c["cls"] == "EXACT" and st["act"] is None:
            want = lc.round_once(ref, out_f32)
            ne = np.flatnonzero(bits[idx] != want)
            assert ne.size == 0, (c["name"], name, "not the rounded reference at", st["idx"].ravel()[ne[:8]].tolist(), vals[ne[:8]], ref[ne[:8]])
            WORST.setdefault(key + ("exact",), 0.0)
            continue
        if vals.size == 0:
            continue
        err = np.abs(vals - ref)
        with np.errstate(divide="ignore", invalid="ignore"):      # (an EXACT GLU value of 0: bound 0, and the error must be 0)
            q = np.where(err == 0.0, 0.0, err / bnd[name].ravel())
        w = int(np.argmax(q))
        k2 = key + (c["cls"].lower(),)
        WORST[k2] = max(WORST.get(k2, 0.0), float(q[w]))
        assert q[w] <= 1.0, (c["name"], name, "|got - ref| / bound", float(q[w]), "at", int(st["idx"].ravel()[w]), "got", vals[w], "ref", ref[w],
                             "bound", float(bnd[name].ravel()[w]))


@pytest.mark.parametrize("run", CHUNKS, ids=_chunk_id)
def test_linear_against_fp64(run):
    for c in run:
        _run_case(c)
    fam, dt = run[0]["family"], "bf16" if run[0]["dtype"] == BF16 else "f32"
    print(" ".join(f"worst |got - ref| / bound so far, {fam} {dt} {cls}: {WORST[(fam, dt, cls)]:.4f};" for cls in ("exact", "random")
                   if (fam, dt, cls) in WORST) + f" {time.time() - T0:.1f} s since the file was loaded")


def test_the_chunks_hold_every_case_of_every_family():
    """the parametrisation above runs all of the table: ten families, both dtypes where a family has fp32 kernels.  (Reads CHUNKS, not
    what ran: it holds under any selection of tests.)  Prints the worst ratios of whatever ran before it in this process."""
    assert sorted(c["name"] for run in CHUNKS for c in run) == sorted(c["name"] for c in lc.CASES)
    assert {run[0]["family"] for run in CHUNKS} == set(lc.FAMILIES)
    for fam in ("skinny", "wave_tile", "mid", "tile128", "tile64"):
        assert {run[0]["dtype"] for run in CHUNKS if run[0]["family"] == fam} == {F32, BF16}
    for key in sorted(WORST):
        print(f"worst |got - ref| / bound, {' '.join(key)}: {WORST[key]:.4f}" + (" (bit-equal)" if key[2] == "exact" and WORST[key] == 0.0 else ""))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_pack_fragment_major_is_the_header_index_map(dtype):
    from simulst_amd.ops import Ops
    ops = Ops()
    KS = 4 * lr.vec_elems(dtype)
    for N, K in ((16, KS), (48, 8 * KS), (768, 256)):
        w = torch.randn(N, K, generator=torch.Generator().manual_seed(N + K)).to(lc.tdt(dtype))
        got = ops.pack_fragment_major(w.cuda()).cpu().view(-1)
        want = torch.empty(N * K, dtype=w.dtype)
        want[torch.from_numpy(lr.fragment_index(N, K, dtype).ravel())] = w.view(-1)
        bits = torch.int32 if dtype == F32 else torch.int16
        assert torch.equal(got.view(bits), want.view(bits)), (N, K)
