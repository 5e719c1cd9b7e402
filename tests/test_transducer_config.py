"""CPU-side checks of the transducer_model plumbing: arch resolution, the state-dict key set against fixture g25 (the reference's own
TransducerDecoder), the checkpoint round trip and its strict refusals, lazy registration, and that nothing moved for the models that
were there before."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G25 = os.path.join(ROOT, "tests", "golden", "g25_transducer.npz")


def test_arch_resolution():
    from simulst_amd.checkpoint import config_from_args
    from simulst_amd.config import ModelConfig, cif_transformer_s, mma_model_s, s2t_emformer_s, transducer_model_s
    c = config_from_args({"arch": "transducer_model_s"})
    assert c == transducer_model_s()
    assert c.model == "transducer_model" and c.simul_attn_type == "none" and c.downsample == 8 and c.ctc_layer is False
    assert (c.embed_dim, c.num_heads, c.ffn_dim, c.decoder_layers, c.encoder_layers) == (256, 4, 2048, 6, 12)
    assert config_from_args({"arch": "transducer_model_s", "downsample": 4}).downsample == 4
    # policy flags a checkpoint may carry mean nothing to it
    c2 = config_from_args({"arch": "transducer_model_s", "simul_attn_type": "waitk_fixed_pre_decision", "waitk_testtime": 5})
    assert c2 == c
    # the other archs resolve exactly as before; --downsample is the transducer's flag alone
    assert ModelConfig().downsample == 1
    assert config_from_args({"arch": "mma_model_s"}) == mma_model_s(mass_preservation=False)
    assert config_from_args({}) == mma_model_s(mass_preservation=False)
    assert config_from_args({"arch": "mma_model_s", "downsample": 4}) == mma_model_s(mass_preservation=False)
    assert config_from_args({"arch": "cif_transformer_s"}) == cif_transformer_s()
    assert config_from_args({"arch": "s2t_emformer_s"}) == s2t_emformer_s()
    assert config_from_args({"arch": "mma_model_s", "waitk_testtime": 7}).waitk_lagging == 7


def test_fixture_key_set_equals_init_model():
    from dataclasses import replace
    from simulst_amd.checkpoint import config_from_args
    from simulst_amd.weights import init_model
    g = np.load(G25)
    args = {k[5:]: g[k].item() for k in g.files if k.startswith("args.")}
    cfg = config_from_args(dict(args, arch="transducer_model_s"))
    assert cfg.downsample == 4 and cfg.model == "transducer_model"
    w = init_model(replace(cfg, vocab=g["w:decoder.embed_tokens.weight"].shape[0]))
    keys = [str(k) for k in g["keys"]]
    assert sorted(keys) == sorted(k for k in w if k.startswith("decoder."))
    assert not any("encoder_attn" in k for k in keys)
    for k, shp in zip(keys, g["shapes"]):
        assert tuple(w[k].shape) == tuple(int(s) for s in shp if s > 0), k
    # the joiner's output projection is the decoder's: one tensor under two names, in the reference's state dict too
    assert np.array_equal(g["w:decoder.joiner.output_projection.weight"], g["w:decoder.output_projection.weight"])
    assert w["decoder.joiner.output_projection.weight"] is w["decoder.output_projection.weight"]


def test_checkpoint_round_trip(tmp_path):
    from simulst_amd import checkpoint
    from simulst_amd.config import transducer_model_s
    from simulst_amd.weights import init_model
    cfg = transducer_model_s(decoder_layers=2, encoder_layers=1, downsample=4)
    sd = init_model(cfg, seed=3)
    args = {"arch": "transducer_model_s", "decoder_layers": 2, "encoder_layers": 1, "downsample": 4}
    p = str(tmp_path / "rnnt.pt")
    checkpoint.save_fairseq_layout(p, args, sd)
    st = checkpoint.read_checkpoint(p)
    c = checkpoint.config_from_args(st["cfg"]["model"])
    assert c == cfg
    up = checkpoint.upgrade_state_dict(st["model"], c, strict=True)
    assert set(up) == set(sd)
    for k in sd:
        assert torch.equal(up[k], sd[k].float()), k
    for missing in ("decoder.joiner.source_projection.bias", "decoder.joiner.target_projection.weight"):
        with pytest.raises(KeyError):
            checkpoint.upgrade_state_dict({k: v for k, v in sd.items() if k != missing}, c, strict=True)
    extra = dict(sd)
    extra["decoder.layers.0.encoder_attn.k_proj.weight"] = torch.zeros(256, 256)
    with pytest.raises(KeyError, match="encoder-attention"):
        checkpoint.upgrade_state_dict(extra, c, strict=True)
    # an export that dropped the alias still loads: the joiner projects with the decoder's output projection
    alias = {k: v for k, v in sd.items() if k != "decoder.joiner.output_projection.weight"}
    up = checkpoint.upgrade_state_dict(alias, c, strict=True)
    assert torch.equal(up["decoder.joiner.output_projection.weight"], sd["decoder.output_projection.weight"])


# sha256 over (name, bytes) of every tensor of init_model(cfg, seed=999), computed on the commit before the transducer was added
PARENT_HASHES = {"mma_model_s": (101, "775f60215cb9e7c1"), "cif_transformer_s": (94, "777ddce29744b667"),
                 "s2t_emformer_s": (93, "7681340f081affbb")}


@pytest.mark.parametrize("arch", sorted(PARENT_HASHES))
def test_init_model_of_the_other_models_is_unchanged(arch):
    from simulst_amd import config
    from simulst_amd.weights import init_model
    cfg = getattr(config, arch)(conv_channels=64, embed_dim=32, ffn_dim=64, num_heads=2, encoder_layers=2, decoder_layers=2, vocab=64,
                                conv_pos=16, conv_pos_groups=4)
    w = init_model(cfg, seed=999)
    m = hashlib.sha256()
    for k in sorted(w):
        m.update(k.encode())
        m.update(w[k].contiguous().numpy().tobytes())
    assert (len(w), m.hexdigest()[:16]) == PARENT_HASHES[arch]
    assert not any("joiner" in k for k in w)


def test_agents_refuse_the_model():
    from simulst_amd.config import tiny
    from simulst_amd.model import refuse_offline_model

    class Fake:
        cfg = tiny(model="transducer_model", simul_attn_type="none", downsample=4)
    with pytest.raises(ValueError, match="transducer_model"):
        refuse_offline_model(Fake(), "agent")


def test_lazy_registration_in_a_fresh_process():
    """importing the streaming models leaves three registered models; asking for the transducer arch brings its module in"""
    code = """
import argparse, sys
import simulst_amd.model, simulst_amd.cif
from simulst_amd import registry
assert sorted(registry.MODEL_REGISTRY) == ["cif_transformer", "mma_model", "s2t_emformer"], sorted(registry.MODEL_REGISTRY)
assert "simulst_amd.transducer" not in sys.modules
m = registry.build_model_from_args(argparse.Namespace(arch="transducer_model_s", downsample=4))
assert type(m).__name__ == "TransducerModel" and m.cfg.model == "transducer_model" and m.cfg.downsample == 4
assert m.decoder is None                      # weights arrive with load_state_dict
assert "transducer_model" in registry.MODEL_REGISTRY and registry.ARCH_REGISTRY["transducer_model_s"][0] == "transducer_model"
registry.ensure_registered("transducer_model")          # idempotent
try:
    registry.build_model_from_args(argparse.Namespace(arch="transducer_model_xl"))
except KeyError:
    pass
else:
    raise AssertionError("unknown arch accepted")
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
