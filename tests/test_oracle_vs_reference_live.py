"""The oracle against the REFERENCE ITSELF at full model size (s2t_emformer_s encoder, mma_model_s decoder, wait-k 5), on the
same weights and inputs.  The other committed golden fixtures pin the oracle at small dimensions; this pins it at the dimensions
every GPU parity test and the bench use.  The reference's outputs were recorded by tests/golden/gen_golden_full_size.py (g21)
on weights this test regenerates (simulst_amd.weights.init_model, seed 999, untied output projection)."""
import torch

from conftest import load_golden


def test_oracle_equals_reference_at_full_model_size():
    from oracle import agent as oag
    from oracle.configs import from_model_config
    from simulst_amd.config import mma_model_s
    from simulst_amd.weights import init_model
    g, _ = load_golden("g21_full_size")
    seed = int(g["seed"])
    cfg = mma_model_s(waitk_lagging=5)
    w = init_model(cfg, seed=seed)
    w["decoder.output_projection.weight"] = torch.randn(cfg.vocab, cfg.embed_dim,
                                                        generator=torch.Generator().manual_seed(5)) * cfg.embed_dim ** -0.5
    ref_toks, ref_enc, L = g["tokens"], g["encoder_out"], g["lengths"]
    B, steps = ref_toks.shape
    fb = torch.stack([torch.randn(int(L[i]), 80, generator=torch.Generator().manual_seed(999 + i)) for i in range(B)])
    ecfg, dcfg = from_model_config(cfg)
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    with torch.no_grad():
        toks, _, enc = oag.greedy_offline(w, ecfg, dcfg, fb, L, n_steps=steps, mask_eos=True)
    assert len(set(ref_toks.flatten().tolist())) >= 4, "degenerate fixture"
    assert torch.equal(toks, ref_toks), (toks, ref_toks)
    diff = float((enc["encoder_out"][0] - ref_enc).abs().max())
    assert diff <= 1e-4 * max(1.0, float(ref_enc.abs().max())), diff
