"""The handle's tunables (csrc/handle.cpp: simulst_create's environment overrides, simulst_set_option, simulst_get_option) against
what the library did BEFORE they were one table, and the decoder of SIMULST_OPT_FFN_WAVES (csrc/ffn_variant.h) against its mapping.

tests/golden/g27_handle_options.json was recorded from the parent commit's common.h and handle.cpp with tests/handle_options_table.cpp,
once per build flavour (`python tests/test_handle_options.py record <that commit's csrc> <fixture>`); the code under test never wrote
it.  Each row holds the statuses of the row's simulst_set_option calls and, as differences from the flavour's untouched handle, every
tunable field and every simulst_get_option answer.  No GPU: nothing is launched, simulst_create leaves n_cus 0.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simulst_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "g27_handle_options.json")
FLAVOURS = {"product": [],
            "experiments": ["-DSL_EXPERIMENTS", "-DSIMULST_EXPERIMENTS"],
            "debug_hooks": ["-DSL_EXPERIMENTS", "-DSIMULST_EXPERIMENTS", "-DSL_DEBUG_HOOKS", "-DSIMULST_DEBUG_HOOKS"]}
ENV = ["PANEL_SPLIT_MIN_ROWS", "PANEL_SPLIT_BLOCKS", "MID_MIN_BLOCKS", "MID_NARROW_MIN_ROWS", "SKINNY_MIN_BLOCKS_TALL", "FUSE_Q_MAX_ROWS",
       "DEC_CHAIN", "DEC_CHAIN_MIN_ROWS", "DEC_CHAIN_MAX_ROWS", "DEC_CHAIN_FFN_MAX_ROWS", "DEC_TALL_FFN", "DEC_TALL_MIN_ROWS",
       "DEC_CHAIN_XMODE", "DEC_CHAIN_LDS_BYTES", "DEC_ATTN_CHAIN_MAX_ROWS", "DEC_VOCAB_CHAIN_SPLIT", "DEC_EMBED_QKV_CHAIN",
       "DEC_CHAIN_ROWS32", "DEC_CHAIN_ROWS32_MIN", "DEC_FUSE_FFN_QKV", "CONV_TILE256", "WEIGHT_STATIONARY", "PANEL_WIDE",
       "POLICY_LDS_BYTES", "FUSED_ARGMAX", "DEC_ATTN_CHAIN_ROWS", "DEC_FUSE_PROJ_CROSS", "EA_GENERAL"]
ENV_VALUES = ["0", "1", "2", "3", "4", "7", "16", "17", "100000", "-5", "abc"]
OPTION_IDS = list(range(17)) + [99]
OPTION_VALUES = [-1, 0, 1, 2, 3, 4, 5, 8, 16, 17] + list(range(41, 48)) + list(range(81, 88)) + [1024]
# SIMULST_OPT_FFN_WAVES -> (pipelined, waves, packed, uniform) while F <= 2048, and the build flavours that accept the code
FFN_PIPELINED = {0: (4, 0, 1), 41: (4, 0, 0), 42: (4, 1, 0), 43: (4, 0, 1), 45: (4, 0, 2), 47: (4, 0, 3), 81: (8, 0, 0), 82: (8, 1, 0),
                 83: (8, 0, 1), 87: (8, 0, 3)}
FFN_LEGAL = {"product": [0, 4, 8, 43], "experiments": [0, 4, 8, 41, 43, 45, 47, 81, 83, 87],
             "debug_hooks": [0, 4, 8, 41, 42, 43, 45, 47, 81, 82, 83, 87]}
FFN_BLOCK4_MAX_F = 2048                                      # FFG<4>::MAX_F of csrc/ffn_fused.hip


def _inputs():
    """the untouched handle first, then every environment variable alone, the feed-forward chain's row limit with and without the tall
    tile's, and every option id with every value"""
    lines = [";"]
    lines += [f"SIMULST_{name}={v} ;" for name in ENV for v in ENV_VALUES]
    lines += ["SIMULST_DEC_CHAIN_FFN_MAX_ROWS=512 ;", "SIMULST_DEC_CHAIN_FFN_MAX_ROWS=512 SIMULST_DEC_TALL_MIN_ROWS=2000 ;",
              "SIMULST_DEC_TALL_MIN_ROWS=2000 ;"]
    lines += [f"; {opt} {v}" for opt in OPTION_IDS for v in OPTION_VALUES]
    return lines


def _build(csrc, out_dir):
    """tests/handle_options_table.cpp + <csrc>/handle.cpp in each flavour (the three compilers run side by side)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    jobs = {}
    for name, flags in FLAVOURS.items():
        prog = os.path.join(str(out_dir), "handle_options_" + name)
        jobs[name] = (prog, subprocess.Popen([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "-I" + csrc,
                                              "-I" + os.path.join(ROOT, "include")] + flags +
                                             [os.path.join(ROOT, "tests", "handle_options_table.cpp"), os.path.join(csrc, "handle.cpp"), "-o", prog]))
    for name, (prog, p) in jobs.items():
        assert p.wait() == 0, f"hipcc failed for the {name} flavour"
    return {name: prog for name, (prog, _) in jobs.items()}


def _parse(line):
    w = line.split()
    i_f, i_g = w.index("fields"), w.index("get")
    assert w[0] == "set"
    return [int(x) for x in w[1:i_f]], dict(zip(w[i_f + 1:i_g:2], map(int, w[i_f + 2:i_g:2]))), w[i_g + 1:]


def _table(prog):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SIMULST_")}
    lines = _inputs()
    out = subprocess.run([prog, "table"], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, env=env).stdout.splitlines()
    assert len(out) == len(lines)
    return [_parse(o) for o in out]


def _record(csrc, path):
    import tempfile
    fix = {"recorded_from": "tests/handle_options_table.cpp built with common.h and handle.cpp of commit a547a10 (the parent of the commit that "
                            "made the options one table), once per flavour: product, -DSL_EXPERIMENTS -DSIMULST_EXPERIMENTS, and those with "
                            "-DSL_DEBUG_HOOKS -DSIMULST_DEBUG_HOOKS.  Inputs: _inputs() of tests/test_handle_options.py, in that order.  Per "
                            "flavour: `default` = fields and get answers (status:value for ids 0 .. 16 and 99) of the untouched handle; each row = "
                            "[set statuses, fields that differ from default, get answers that differ (by position)].",
           "inputs": len(_inputs()), "flavours": {}}
    with tempfile.TemporaryDirectory() as d:
        for name, prog in _build(csrc, d).items():
            rows = _table(prog)
            _, f0, g0 = rows[0]
            fix["flavours"][name] = {"default": {"fields": f0, "get": g0},
                                     "rows": [[s, {k: v for k, v in f.items() if v != f0[k]}, {str(i): x for i, x in enumerate(g) if x != g0[i]}]
                                              for s, f, g in rows]}
    with open(path, "w") as fh:
        json.dump(fix, fh, separators=(",", ":"))
        fh.write("\n")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return _build(CSRC, tmp_path_factory.mktemp("handle_options"))


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_every_status_field_and_read_back_equals_the_record(programs, flavour):
    fix = json.load(open(FIXTURE))
    lines = _inputs()
    want = fix["flavours"][flavour]
    assert fix["inputs"] == len(lines) == len(want["rows"])
    f0, g0 = want["default"]["fields"], want["default"]["get"]
    got = _table(programs[flavour])
    for line, (s, f, g), (ws, wf, wg) in zip(lines, got, want["rows"]):
        assert s == ws, f"{flavour} '{line}': set_option statuses {s}, recorded {ws}"
        assert f == {**f0, **wf}, f"{flavour} '{line}': fields"
        assert g == [wg.get(str(i), x) for i, x in enumerate(g0)], f"{flavour} '{line}': get_option"
    # the record itself distinguishes the flavours and refuses something in each (a fixture of all-equal rows would prove nothing)
    assert any(ws != [0] for ws, _, _ in want["rows"] if ws) and any(wf for _, wf, _ in want["rows"])


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_ffn_variant_decoder_equals_the_mapping(programs, flavour):
    """every code the flavour accepts at F = 64, 2048 (the pipelined form's last), 2112 and 4096"""
    cases = [(c, F) for c in FFN_LEGAL[flavour] for F in (64, 2048, 2112, 4096)]
    out = subprocess.run([programs[flavour], "ffn"], input="".join(f"{c} {F}\n" for c, F in cases), capture_output=True, text=True,
                         check=True).stdout.splitlines()
    assert len(out) == len(cases)
    for (c, F), o in zip(cases, out):
        if c in FFN_PIPELINED and F <= 2048:
            want = (1,) + FFN_PIPELINED[c]
        elif c in FFN_PIPELINED and c != 0:                  # a pipelined code above the pipelined form's F: the block form, 8 waves
            want = (0, 8, 0, 0)
        else:                                                # 0, 4: 4 waves while the fc1 bias fits their LDS; 8: 8 waves
            want = (0, 4 if c != 8 and F <= FFN_BLOCK4_MAX_F else 8, 0, 0)
        assert tuple(int(x) for x in o.split()) == want, f"{flavour} code {c} F {F}: {o}"


if __name__ == "__main__":
    assert len(sys.argv) == 4 and sys.argv[1] == "record", "usage: test_handle_options.py record <csrc of the commit to record> <fixture.json>"
    _record(sys.argv[2], sys.argv[3])
