#!/usr/bin/env python3
"""g22_agent_surface.json: the reference agent's side of tests/test_agent_surface.py, recorded by RUNNING the reference's
FairseqSimulSTAgent (agents/default_agent.py) in the build container.

  calls.<force_finish>   {"seen": what the SimulEval-style driver saw (actions, encoder state shapes, predictions, segments),
                          "trace": how the agent called the recording model} for the test's event script
  word_merger            per random unit stream: the units, max_len, and every (units_to_segment result, queue after the call)

The agent module is imported by file path from /root/reference (never copied) over stub `simuleval` / `fairseq` modules whose
names resolve to this package's SimulEval stand-ins; the recording model, the event script and the unit streams are the test
module's own, so the test replays exactly the same episodes through this package's agent.

    python tests/golden/gen_golden_agent_surface.py
"""
import importlib.util
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF_AGENT = "/root/reference/codebase/agents/default_agent.py"

import test_agent_surface as tas  # noqa: E402


def load_reference_agent():
    """agents/default_agent.py by file path over stub simuleval / fairseq modules (nothing is copied)."""
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    from simulst_amd import simuleval_agent as mine
    saved = {k: sys.modules.get(k) for k in ("simuleval", "simuleval.agents", "simuleval.states", "fairseq",
                                             "fairseq.data", "fairseq.data.audio", "fairseq.data.audio.audio_utils")}
    mod("simuleval", READ_ACTION=mine.READ_ACTION, WRITE_ACTION=mine.WRITE_ACTION, DEFAULT_EOS=mine.DEFAULT_EOS)
    mod("simuleval.agents", SpeechAgent=mine.SpeechAgent)
    mod("simuleval.states", ListEntry=mine.ListEntry, SpeechStates=mine.SpeechStates)
    mod("fairseq", utils=None, checkpoint_utils=None, tasks=None)
    mod("fairseq.data")
    mod("fairseq.data.audio")
    mod("fairseq.data.audio.audio_utils", _get_kaldi_fbank=None, _get_torchaudio_fbank=None)
    try:
        spec = importlib.util.spec_from_file_location("_ref_default_agent", REF_AGENT)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return m


def record_calls(ref_mod, force_finish):
    from simulst_amd.harness import Dictionary
    model = tas.RecordingModel(tas.call_script(force_finish))
    agent = object.__new__(ref_mod.FairseqSimulSTAgent)            # its __init__ needs fairseq + a checkpoint
    agent.model, agent.gpu, agent.dict, agent.pre_tokenizer = model, False, {"tgt": Dictionary(tas.SYMBOLS, 2)}, None
    agent.pre_decision_ratio = getattr(model.decoder.layers[0].encoder_attn, "pre_decision_ratio", 1)
    agent.full_sentence, agent.force_finish = False, force_finish
    agent.stride_ms = model.encoder.conv_layer_stride() * 10
    agent.right_context, agent.segment_length = model.encoder.right_context, model.encoder.segment_length
    agent.max_len = lambda x: min(1 * x + 0, model.max_decoder_positions())
    agent.feature_extractor = types.SimpleNamespace(clear_cache=lambda: None)
    seen = tas._drive(agent, model, tas.FEED)
    return {"seen": seen, "trace": model.trace}


def main():
    ref_mod = load_reference_agent()

    def make_segment(tgt):
        ref = object.__new__(ref_mod.FairseqSimulSTAgent)
        ref.dict, ref.pre_tokenizer = {"tgt": tgt}, None

        def segment(q, states, target, max_len):
            ref.max_len = lambda x: max_len
            return ref.units_to_segment(q, states)
        return segment
    out = {"calls": {str(ff): record_calls(ref_mod, ff) for ff in (False, True)},
           "word_merger": tas.merger_steps(make_segment)}
    with open(os.path.join(HERE, "g22_agent_surface.json"), "w") as f:
        json.dump(out, f, ensure_ascii=False, separators=(",", ":"))
        f.write("\n")
    print("g22_agent_surface.json:", {k: len(v["trace"]) for k, v in out["calls"].items()}, "trace entries,",
          sum(len(c["steps"]) for c in out["word_merger"]), "units_to_segment calls")


if __name__ == "__main__":
    main()
