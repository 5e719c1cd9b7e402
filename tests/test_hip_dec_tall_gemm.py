"""The pipelined tile of the decode step's tall fc2 (csrc/dec_gemm_tall.hip, SIMULST_OPT_DEC_TALL_FFN): bit for bit the bytes of the
simulst_linear launch it replaces (skinny_kernel's four interleaved k-step streams, added ((p0 + p1) + p2) + p3, then bias, residual,
one rounding), so the decode loops' tokens and logits do not depend on the option and neither the retire floor nor simulst_linear's
plan changes.  Kernel level: raw bytes against simulst_linear, a torch fp64 product with the bf16 tolerances of test_linear_plan.py,
guard elements around C.  Loop level: simulst_mma_decode (wait-k 5), simulst_cif_decode and a ragged batch that retires rows, option on
and off.  CPU: the plan's flag over B = 1 .. 9000 from a host program built against the library's object files."""
import glob
import os
import subprocess

import pytest
import torch

from simulst_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simulst_amd", "csrc")
D = 256
ROW_LIMIT = 8192          # gemm_plan.h SKINNY_MAX_ROWS_PACKED: the decode-step GEMMs' row limit
CHAIN_FFN_MAX = 1024      # handle.cpp dec_chain_ffn_max_rows
PANEL_SPLIT_MIN = 2560    # handle.cpp panel_split_min_rows


# ---- CPU: the flag of the decode plan --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flag_table(tmp_path_factory):
    objs = sorted(glob.glob(os.path.join(CSRC, "build", "*.o")))
    assert objs, "the library's object files (csrc/build/*.o): run __graft_entry__.build() first"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    d = tmp_path_factory.mktemp("dec_tall_plan")
    main_o, prog = str(d / "main.o"), str(d / "dec_tall_plan_table")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                    "-c", os.path.join(ROOT, "tests", "dec_tall_plan_table.cpp"), "-o", main_o], check=True)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-o", prog, main_o] + objs, check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SIMULST_")}      # the handle's defaults
    out = subprocess.run([prog], capture_output=True, text=True, check=True, env=env).stdout.split()
    vals = list(map(int, out))
    assert len(vals) == 7 * 9000 * 5
    table = {}
    for i in range(0, len(vals), 5):
        table[(vals[i], vals[i + 1])] = (vals[i + 2], vals[i + 3], vals[i + 4])
    return table


def test_plan_flag_over_rows(flag_table):
    """off while the feed-forward chain runs (B <= 1024), on from 1025 rows to the decode-step row limit, off beyond it; off with the
    option off, for fp32, for the one-launch-per-GEMM hook, for row-major weights and where simulst_linear would not run its
    k-interleaved tile (D = 512); the CIF loop reads the same flag"""
    for s in (0, 4):
        for B in range(1, 9001):
            tall, chain_ffn, fc1 = flag_table[(s, B)]
            assert tall == int(CHAIN_FFN_MAX < B <= ROW_LIMIT), (s, B, tall)
            # fc1: where simulst_linear runs the split row panel (handle.cpp panel_split_min_rows = 2560); below, its launch is the
            # 64 x 64 tile, which keeps its kernel
            assert fc1 == int(PANEL_SPLIT_MIN <= B <= ROW_LIMIT), (s, B, fc1)
            assert not ((tall or fc1) and chain_ffn)
    for s in (1, 2, 3, 5):
        assert not any(flag_table[(s, B)][0] or flag_table[(s, B)][2] for B in range(1, 9001)), s
    assert not any(flag_table[(6, B)][0] for B in range(1, 9001))          # D = 512: fc2 is the 64 x 64 tile's


# ---- GPU: the launch against simulst_linear ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


GUARD = 64


def _guarded(res):
    """res in the middle of a buffer with GUARD sentinel elements on either side; returns (buffer, the [B, D] view)"""
    B, N = res.shape
    buf = torch.full((GUARD + B * N + GUARD,), 1234.0, device=res.device, dtype=res.dtype)
    mid = buf[GUARD:GUARD + B * N].view(B, N)
    mid.copy_(res)
    return buf, mid


@pytest.mark.gpu
@pytest.mark.parametrize("F", [2048, 2080])
@pytest.mark.parametrize("B", [1025, 1040, 4096])
def test_tall_fc2_equals_simulst_linear_bytes(ops, B, F):
    """rows 1025 (one live row in the last 16-row tile), 1040 (65 row tiles: a partial workgroup tile), 4096; F = 2080 is 65 k-steps,
    a k tail that is no whole chunk.  C aliases R in both launches."""
    import ctypes as C
    g = torch.Generator(device="cuda").manual_seed(1000 * B + F)
    rn = lambda *shape: torch.randn(*shape, generator=g, device="cuda")
    A = rn(B, F).to(torch.bfloat16)
    W = (rn(D, F) / F ** 0.5).to(torch.bfloat16)
    b, res = rn(D), rn(B, D).to(torch.bfloat16)
    Wp = ops.pack_fragment_major(W)
    want64 = A.double() @ W.double().t() + b.double() + res.double()
    buf_old, x_old = _guarded(res)
    buf_new, x_new = _guarded(res)
    ops.linear(A, Wp, b, epilogue=_lib.EPI_BIAS_RES, residual=x_old, out=x_old, w_fragment_major=True)
    vp = C.c_void_p
    ops.h.check(ops.lib.simulst_dec_tall_gemm(ops.h.ptr, vp(A.data_ptr()), vp(Wp.data_ptr()), vp(b.data_ptr()), vp(x_new.data_ptr()),
                                              vp(x_new.data_ptr()), B, D, F, _lib.BF16), "simulst_dec_tall_gemm")
    torch.cuda.synchronize()
    diff = (x_new.view(torch.int16) != x_old.view(torch.int16)).sum().item()
    print(f"B {B} F {F}: {diff} of {B * D} outputs differ from simulst_linear; max |err| vs fp64 "
          f"{(x_new.double() - want64).abs().max().item():.4f}")
    assert torch.equal(x_new.view(torch.int16), x_old.view(torch.int16)), diff
    torch.testing.assert_close(x_new.double(), want64, atol=6e-2, rtol=3e-2)
    for buf in (buf_new, buf_old):
        assert (buf[:GUARD] == 1234.0).all() and (buf[-GUARD:] == 1234.0).all()


@pytest.mark.gpu
def test_tall_fc2_refuses_other_shapes(ops):
    """fp32, a contraction simulst_linear splits (K = 4096) or keeps on another kernel (N = 512): E_SHAPE, nothing launched"""
    import ctypes as C
    t = torch.zeros(16, device="cuda", dtype=torch.bfloat16)
    vp = C.c_void_p(t.data_ptr())
    for B, N, K, dt in ((2048, 256, 2048, _lib.F32), (2048, 256, 4096, _lib.BF16), (2048, 512, 2048, _lib.BF16), (9000, 256, 2048, _lib.BF16)):
        assert ops.lib.simulst_dec_tall_gemm(ops.h.ptr, vp, vp, vp, vp, vp, B, N, K, dt) == -2, (B, N, K, dt)          # SIMULST_E_SHAPE


@pytest.mark.gpu
@pytest.mark.parametrize("F", [2048, 2080])
@pytest.mark.parametrize("B", [2561, 2576, 4096])
def test_tall_fc1_equals_simulst_linear_bytes(ops, B, F):
    """LN + fc1 + GELU against simulst_linear's split row panel, which takes this shape from 2560 rows on: 2561 rows (one live row in the
    last 16-row tile), 2576 (161 row tiles: a partial 128-row panel), 4096; F = 2080 is 32.5 column steps (a half step and a workgroup
    with one step).  fp64 reference: LayerNorm in fp64, rounded to bf16 where the kernels round it, product, bias, erf GELU."""
    import ctypes as C
    g = torch.Generator(device="cuda").manual_seed(2000 * B + F)
    rn = lambda *shape: torch.randn(*shape, generator=g, device="cuda")
    x = rn(B, D).to(torch.bfloat16)
    W = (rn(F, D) / D ** 0.5).to(torch.bfloat16)
    b = rn(F)
    gam, bet = torch.rand(D, generator=g, device="cuda") + 0.5, rn(D) * 0.1
    Wp = ops.pack_fragment_major(W)
    z = torch.nn.functional.layer_norm(x.double(), (D,), gam.double(), bet.double()).to(torch.bfloat16)
    want64 = torch.nn.functional.gelu(z.double() @ W.double().t() + b.double())
    buf_old, h_old = _guarded(torch.zeros(B, F, device="cuda", dtype=torch.bfloat16))
    buf_new, h_new = _guarded(torch.zeros(B, F, device="cuda", dtype=torch.bfloat16))
    ops.linear(x, Wp, b, epilogue=_lib.EPI_BIAS_GELU, out=h_old, ln=(gam, bet), w_fragment_major=True)
    vp = C.c_void_p
    ops.h.check(ops.lib.simulst_dec_tall_fc1(ops.h.ptr, vp(x.data_ptr()), vp(Wp.data_ptr()), vp(b.data_ptr()), vp(gam.data_ptr()),
                                             vp(bet.data_ptr()), vp(h_new.data_ptr()), B, F, D, _lib.BF16), "simulst_dec_tall_fc1")
    torch.cuda.synchronize()
    diff = (h_new.view(torch.int16) != h_old.view(torch.int16)).sum().item()
    print(f"fc1 B {B} F {F}: {diff} of {B * F} outputs differ from simulst_linear; max |err| vs fp64 "
          f"{(h_new.double() - want64).abs().max().item():.4f}")
    assert torch.equal(h_new.view(torch.int16), h_old.view(torch.int16)), diff
    torch.testing.assert_close(h_new.double(), want64, atol=6e-2, rtol=3e-2)
    for buf in (buf_new, buf_old):
        assert (buf[:GUARD] == 1234.0).all() and (buf[-GUARD:] == 1234.0).all()


@pytest.mark.gpu
def test_tall_fc1_refuses_other_shapes(ops):
    """fp32, rows below the split row panel's (simulst_linear runs the 64 x 64 tile there), K > 256, a narrow output: E_SHAPE"""
    import ctypes as C
    t = torch.zeros(16, device="cuda", dtype=torch.bfloat16)
    vp = C.c_void_p(t.data_ptr())
    for B, N, K, dt in ((4096, 2048, 256, _lib.F32), (1040, 2048, 256, _lib.BF16), (4096, 2048, 512, _lib.BF16), (4096, 256, 256, _lib.BF16)):
        assert ops.lib.simulst_dec_tall_fc1(ops.h.ptr, vp, vp, vp, vp, vp, vp, B, N, K, dt) == -2, (B, N, K, dt)      # SIMULST_E_SHAPE


# ---- GPU: the decode loops with the option on and off ------------------------------------------------------------------------------------
def _handles():
    from simulst_amd.ops import Ops
    o_on, o_off = Ops(), Ops()
    assert o_on.h.get_option(_lib.OPT_DEC_TALL_FFN) == 1
    o_off.h.set_option(_lib.OPT_DEC_TALL_FFN, 0)
    for o in (o_on, o_off):
        o.h.set_option(_lib.OPT_FUSED_ARGMAX, 0)          # both write fp32 logits: the final step's are compared
        o.h.timer_enable(_lib.K_DEC_TALL_GEMM, True)
    return o_on, o_off


def _tall_launches(o):
    return o.h.timer_read(_lib.K_DEC_TALL_GEMM)[1]


def _frames(B, T, seed):
    fb = torch.randn(B, T, 80, generator=torch.Generator().manual_seed(seed))
    L = torch.randint(T // 2, T + 1, (B,), generator=torch.Generator().manual_seed(seed + 1))
    L[0] = T
    for b in range(B):
        fb[b, L[b]:] = 0
    return fb.cuda().to(torch.bfloat16), L


def _untie(cfg, w):
    w["decoder.embed_tokens.weight"][cfg.eos] = 0
    # an UNTIED output projection: with the tied random embedding a row repeats one token forever, a degenerate check
    w["decoder.output_projection.weight"] = torch.randn(cfg.vocab, cfg.embed_dim, generator=torch.Generator().manual_seed(5)) \
        * cfg.embed_dim ** -0.5


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1040, 2576])
def test_mma_decode_waitk_tokens_and_logits_do_not_depend_on_the_option(B):
    """simulst_mma_decode, wait-k 5, 6 forced steps, 2 decoder layers: tokens and the final step's fp32 logits.  1040 rows: fc2 on the
    tall tile; 2576 rows: fc1 as well (two launches of the class per layer and step)"""
    from simulst_amd.config import mma_model_s
    from simulst_amd.model import SimulSTModel
    from simulst_amd.weights import init_model
    T, U = 160, 6
    fb, L = _frames(B, T, 30)
    cfg = mma_model_s(encoder_layers=1, decoder_layers=2, simul_attn_type="waitk_fixed_pre_decision", waitk_lagging=5)
    w = init_model(cfg, seed=21)
    _untie(cfg, w)
    o_on, o_off = _handles()
    got = []
    for o in (o_on, o_off):
        toks, info = SimulSTModel(cfg, w, dtype=torch.bfloat16, ops=o).generate_offline(fb, L, n_steps=U, mask_eos=True)
        got.append((toks.clone(), info["state"].ws["logits"].clone()))
    torch.cuda.synchronize()
    assert _tall_launches(o_on) == U * cfg.decoder_layers * (2 if B >= PANEL_SPLIT_MIN else 1) and _tall_launches(o_off) == 0
    assert torch.equal(got[0][0], got[1][0]), (got[0][0] != got[1][0]).sum().item()
    assert torch.equal(got[0][1].view(torch.int32), got[1][1].view(torch.int32))
    assert len(set(got[0][0].flatten().tolist())) > 50         # not a degenerate hypothesis


@pytest.mark.gpu
def test_cif_decode_tokens_and_logits_do_not_depend_on_the_option():
    """simulst_cif_decode, 1040 rows, 6 forced steps, 2 decoder layers"""
    from simulst_amd.cif import CIFTransformerModel
    from simulst_amd.config import cif_transformer_s
    from simulst_amd.weights import init_model
    B, T, U = 1040, 160, 6
    fb, L = _frames(B, T, 40)
    cfg = cif_transformer_s(encoder_layers=1, decoder_layers=2, cif_beta=1.0)
    w = init_model(cfg, seed=21)
    w["encoder.cif_layer.alpha_proj.4.weight"] = w["encoder.cif_layer.alpha_proj.4.weight"] * 4
    w["encoder.cif_layer.alpha_proj.4.bias"] = w["encoder.cif_layer.alpha_proj.4.bias"] - 1.0
    _untie(cfg, w)
    o_on, o_off = _handles()
    got = []
    for o in (o_on, o_off):
        m = CIFTransformerModel(cfg, w, dtype=torch.bfloat16, ops=o)
        toks = m.generate_offline(fb, L, n_steps=U, mask_eos=True)[0]
        st, = m.decoder._offline_states.values()
        got.append((toks.clone(), st["ws"]["logits"].clone()))
    torch.cuda.synchronize()
    assert _tall_launches(o_on) == U * cfg.decoder_layers and _tall_launches(o_off) == 0
    assert torch.equal(got[0][0], got[1][0]), (got[0][0] != got[1][0]).sum().item()
    assert torch.equal(got[0][1].view(torch.int32), got[1][1].view(torch.int32))
    assert len(set(got[0][0].flatten().tolist())) > 50


@pytest.mark.gpu
def test_ragged_batch_that_retires_rows_does_not_depend_on_the_option():
    """greedy_offline_ragged over 1072 rows whose caps make the call shrink to 1040 rows (still above the feed-forward chain's rows:
    the tall tile at another row count) and then to 608 (the chains): every kept token identical with the option on and off"""
    from simulst_amd.config import mma_model_s
    from simulst_amd.model import SimulSTModel
    from simulst_amd.weights import init_model
    B, T = 1072, 160
    fb, L = _frames(B, T, 50)
    steps = [24] * 600 + [16] * 430 + [8] * (B - 1030)
    cfg = mma_model_s(encoder_layers=1, decoder_layers=2, simul_attn_type="waitk_fixed_pre_decision", waitk_lagging=5)
    w = init_model(cfg, seed=21)
    _untie(cfg, w)
    o_on, o_off = _handles()
    got = []
    for o in (o_on, o_off):
        m = SimulSTModel(cfg, w, dtype=torch.bfloat16, ops=o)
        enc = m.encoder.forward(fb, L)
        toks, _ = m.decoder.greedy_offline_ragged(enc["encoder_out_btd"], enc["encoder_lengths"], steps, False)
        got.append(toks.clone())
    torch.cuda.synchronize()
    assert _tall_launches(o_on) == 16 * cfg.decoder_layers and _tall_launches(o_off) == 0      # steps 0 .. 15 run above 1024 rows
    assert torch.equal(got[0], got[1]), (got[0] != got[1]).sum().item()
    assert len(set(got[0].flatten().tolist())) > 50
