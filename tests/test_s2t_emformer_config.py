"""CPU-side checks of the s2t_emformer model (full encoder-decoder attention, SIMULST_ATTN_FULL): the arch resolves to it, its
checkpoints keep the plain decoder key set, the fixture g23 (the reference's own S2TEmformerModel.build_model) agrees on the key set,
and the entry points that have no meaning for a model without a policy refuse it before anything reaches the device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_pins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G23 = os.path.join(ROOT, "tests", "golden", "g23_s2t_emformer.npz")
E_ARG = -4


def test_arch_resolves_to_full_attention():
    from simulst_amd.checkpoint import config_from_args
    from simulst_amd.config import cif_transformer_s, mma_model_s
    c = config_from_args({"arch": "s2t_emformer_s"})
    assert c.model == "s2t_emformer" and c.simul_attn_type == "full" and c.attn_type == "full"
    assert c.pre_decision_ratio == 1 and c.ctc_layer is False
    assert (c.embed_dim, c.num_heads, c.ffn_dim, c.decoder_layers, c.encoder_layers) == (256, 4, 2048, 6, 12)
    assert (c.segment_length, c.segment_left_context, c.segment_right_context, c.max_memory_size) == (64, 128, 32, 5)
    # policy flags a checkpoint may carry do not turn it into a simultaneous model
    c2 = config_from_args({"arch": "s2t_emformer_s", "simul_attn_type": "waitk_fixed_pre_decision", "waitk_lagging": 3,
                           "waitk_testtime": 5, "energy_bias": True})
    assert c2.attn_type == "full" and not c2.energy_bias
    # the other archs resolve exactly as before
    assert config_from_args({"arch": "mma_model_s"}) == mma_model_s(mass_preservation=False)
    assert config_from_args({}) == mma_model_s(mass_preservation=False)
    assert config_from_args({"arch": "cif_transformer_s"}) == cif_transformer_s()
    assert config_from_args({"arch": "mma_model_s", "waitk_testtime": 7}).waitk_lagging == 7


def test_init_model_plain_decoder_keys():
    from simulst_amd.config import s2t_emformer_s
    from simulst_amd.weights import init_model
    w = init_model(s2t_emformer_s(decoder_layers=2, encoder_layers=1))
    ea = sorted(k for k in w if ".layers.0.encoder_attn." in k)
    assert set(ea) == {f"decoder.layers.0.encoder_attn.{n}_proj.{m}" for n in ("q", "k", "v", "out") for m in ("weight", "bias")}
    assert not any("_soft" in k or "energy_bias" in k for k in w)


def test_fixture_key_set_equals_init_model():
    from simulst_amd.checkpoint import config_from_args
    from simulst_amd.weights import init_model
    g = np.load(G23)
    args = {k[5:]: g[k].item() for k in g.files if k.startswith("args.")}
    cfg = config_from_args(dict(args, arch="s2t_emformer_s"))
    from dataclasses import replace
    w = init_model(replace(cfg, vocab=g["w:decoder.embed_tokens.weight"].shape[0]))     # the task dictionary's size
    keys = [str(k) for k in g["keys"]]
    assert sorted(keys) == sorted(k for k in w if k.startswith("decoder."))
    for k, shp in zip(keys, g["shapes"]):
        assert tuple(w[k].shape) == tuple(int(s) for s in shp if s > 0), k


def test_checkpoint_round_trip(tmp_path):
    from simulst_amd import checkpoint
    from simulst_amd.config import s2t_emformer_s
    from simulst_amd.weights import init_model
    cfg = s2t_emformer_s(decoder_layers=2, encoder_layers=1)
    sd = init_model(cfg, seed=3)
    args = {"arch": "s2t_emformer_s", "decoder_layers": 2, "encoder_layers": 1}
    p = str(tmp_path / "asr.pt")
    checkpoint.save_fairseq_layout(p, args, sd)
    st = checkpoint.read_checkpoint(p)
    c = checkpoint.config_from_args(st["cfg"]["model"])
    assert c == cfg
    up = checkpoint.upgrade_state_dict(st["model"], c, strict=True)
    assert set(up) == set(sd) and not any("_soft" in k for k in up)
    for k in sd:
        assert torch.equal(up[k], sd[k].float()), k
    bad = {k: v for k, v in sd.items() if k != "decoder.layers.1.encoder_attn.v_proj.weight"}
    with pytest.raises(KeyError):
        checkpoint.upgrade_state_dict(bad, c, strict=True)
    extra = dict(sd)
    extra["decoder.layers.0.encoder_attn.energy_bias"] = torch.zeros(1)
    with pytest.raises(KeyError):
        checkpoint.upgrade_state_dict(extra, c, strict=True)


def test_model_class_refuses_a_policy_config():
    from simulst_amd.config import tiny
    from simulst_amd.model import S2TEmformerModel, refuse_offline_model
    with pytest.raises(ValueError):
        S2TEmformerModel(tiny(), {}, device="cpu")

    class Fake:
        cfg = tiny(model="s2t_emformer", simul_attn_type="full")
    with pytest.raises(ValueError, match="full attention"):
        refuse_offline_model(Fake(), "agent")
    Fake.cfg = tiny()
    refuse_offline_model(Fake(), "agent")


def test_full_declared_and_bound():
    from simulst_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "simulst_hip.h")).read(), flags=re.S)
    assert re.search(r"SIMULST_ATTN_FULL\s*=\s*4", src)
    assert _lib.ATTN_FULL == 4 and _lib.ATTN_ENUM["full"] == 4
    assert _lib.load().simulst_version() == abi_pins.VERSION


@pytest.fixture
def handle():
    from simulst_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.simulst_create(ctypes.byref(h), None) == 0
    yield lib, h
    assert lib.simulst_destroy(h) == 0


@pytest.fixture
def host_buf():
    """host memory for every pointer argument: never dereferenced by a refused call"""
    buf = (ctypes.c_int64 * 4096)()
    return buf, ctypes.addressof(buf)


def test_refusals_on_host_buffers(handle, host_buf):
    from simulst_amd import _lib
    lib, h = handle
    _, p = host_buf
    FULL = _lib.ATTN_FULL
    # not a simultaneous policy: no step probabilities
    assert lib.simulst_step_p_choose(h, p, p, 0.0, p, p, 2, 16, 2, 16, 1, 1, FULL, 3, p, 0, _lib.F32) == E_ARG
    assert lib.simulst_step_p_choose_padded(h, p, p, 0.0, p, p, 2, 16, 16, 2, 16, 1, 1, FULL, 0.3, _lib.F32) == E_ARG
    # ... and no streaming
    d = _lib.DecoderDesc()
    d.B, d.D, d.H, d.F, d.V, d.n_layers, d.cap, d.S_cap = 2, 32, 2, 64, 64, 1, 8, 16
    d.dtype, d.attn_type, d.ratio = _lib.F32, FULL, 1
    layers = (_lib.DecLayer * 1)()
    ctl = _lib.StreamCtl()
    ctl.active = ctl.read_flag = ctl.online = ctl.done = ctl.hyp = p
    ctl.cap = 8
    assert lib.simulst_mma_stream_steps(h, ctypes.byref(d), layers, p, ctypes.byref(ctl), 1) == E_ARG
    # an attention type beyond FULL
    assert lib.simulst_policy_cross_attention(h, p, p, p, p, p, 0.0, p, p, p, p, p, 2, 2, 16, 16, 1, 5, 3, 0, 0, _lib.F32) == E_ARG
    assert lib.simulst_decoder_cross_attention(h, p, p, p, p, p, p, None, 2, 2, 16, 16, 5, 0, _lib.F32) == E_ARG
    assert lib.simulst_step_p_choose(h, p, p, 0.0, p, p, 2, 16, 2, 16, 1, 1, 5, 3, p, 0, _lib.F32) == E_ARG
