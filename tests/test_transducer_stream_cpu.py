"""Host side of the transducer's simultaneous decoding: ``emit_delays`` (pooled emit position -> the chunk the token is written
at) against a per-token walk over the chunks, the record builder, and the header's statement of the open-source form of the
joiner entry points.  No GPU."""
import os
import re

import pytest

from simulst_amd.transducer_agent import emit_delays, records_from_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def walk(emit, n_tokens, enc_len, k, schedule):
    """token by token, chunk by chunk: a row sits at chunk c and takes the next one while its token's position is not available.
    Position e is available at chunk c when the encoder has released the whole window of e (or all it has, for the partial last
    window); the true last position only once the source has ended (the final chunk)."""
    last_pos = -(-enc_len // k) - 1
    c, out = 0, []
    for e in emit[:n_tokens]:
        while True:
            released = schedule[c]
            whole_window = released >= (e + 1) * k or released >= enc_len
            if whole_window and (e < last_pos or c == len(schedule) - 1):
                break
            c += 1
        out.append(c)
    return out


def schedule_of(enc_len, seg=16):
    """rows released per chunk by a 16-row-segment encoder that holds 4 look-ahead rows back until the next chunk (the end)"""
    out, n = [], 0
    while n + seg < enc_len:
        n += seg
        out.append(max(n - 4, 0))          # 4 look-ahead rows are released with the next segment
    out.append(enc_len)
    return out


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("enc_len", [96, 95, 64, 33, 50, 17])
def test_emit_delays_against_the_walk(k, enc_len):
    """k = 3 does not divide the 16-row segments; 95 / 33 / 50 / 17 leave a partial last window for k = 8 (and some for k = 3)"""
    sched = schedule_of(enc_len)
    S = -(-enc_len // k)
    hyps = [list(range(S)),                                   # one token per position, the forced last one included
            [0, 0, 1, 3, 9 % S, S - 1, S - 1],                # repeated positions, then the forced position twice
            [S - 1],                                          # straight to the end
            [max(S - 2, 0)] * 3]                              # the last position that is NOT forced
    for emit in hyps:
        emit = sorted(emit)
        got = emit_delays(emit, len(emit), enc_len, k, sched)
        assert got == walk(emit, len(emit), enc_len, k, sched), (k, enc_len, emit)
        assert got == sorted(got) and all(0 <= c < len(sched) for c in got)
        assert emit_delays(emit, 2, enc_len, k, sched) == got[:2]
    # a token at the forced last position is written at the final chunk only
    assert emit_delays([S - 1], 1, enc_len, k, sched) == [len(sched) - 1]
    if S >= 2 and len(sched) >= 2 and sched[0] >= k:
        assert emit_delays([0], 1, enc_len, k, sched) == [0]


def test_emit_delays_short_source_and_empty_hypothesis():
    # a source shorter than one chunk: one release, everything at chunk 0 -- also when it is shorter than one window
    assert emit_delays([0, 0, 1], 3, 12, 8, [12]) == [0, 0, 0]
    assert emit_delays([0, 0], 2, 3, 8, [3]) == [0, 0]
    assert emit_delays([0], 1, 1, 1, [1]) == [0]
    # an empty hypothesis (also of a source without an encoder row)
    assert emit_delays([], 0, 40, 8, [12, 28, 40]) == []
    assert emit_delays([5, 5], 0, 40, 8, [12, 28, 40]) == []
    assert emit_delays([], 0, 0, 8, [0]) == []
    # ragged lengths over one schedule shape: the partial last window (rows 32 .. 36 of 37) needs the final chunk
    assert emit_delays([0, 1, 3, 4], 4, 37, 8, [12, 28, 37]) == [0, 1, 2, 2]
    assert walk([0, 1, 3, 4], 4, 37, 8, [12, 28, 37]) == [0, 1, 2, 2]
    # a window that is complete before the end is not the last position: 40 rows, position 3 = rows 24 .. 31
    assert emit_delays([3, 4], 2, 40, 8, [12, 28, 32, 40]) == [2, 3]


def test_records_from_chunks_cut_at_eos_and_cap():
    positions = [100, 180, 260]
    rec = records_from_chunks([7, 8, 2, 9], [0, 1, 1, 2], [0, 1, 1, 2], positions, lambda x: 50, 2, 2615, lambda c: [12, 28, 40][c])
    assert rec["tokens"] == [7, 8, 2] and rec["emit"] == [0, 1, 1] and rec["actions"] == "RWRWW"
    assert rec["delays_ms"] == [1015, 1815, 1815] and rec["n_enc"] == 28
    # the cap rule: more tokens than max_len(frames read) ends the row
    rec = records_from_chunks([7, 8, 9, 9], [0, 0, 0, 0], [0, 0, 0, 1], positions, lambda x: 0.02 * x, 2, 2615, lambda c: c)
    assert rec["tokens"] == [7, 8, 9] and rec["actions"] == "RWWW"
    rec = records_from_chunks([], [], [], positions, lambda x: 5, 2, 2615, lambda c: c)
    assert rec["tokens"] == [] and rec["actions"] == "RRR" and rec["AL"] == 0.0


def test_header_documents_the_open_source_form():
    """all four joiner entry points (and the blank mask) state what a negative src_len means"""
    with open(os.path.join(ROOT, "include", "simulst_hip.h")) as f:
        text = f.read()
    for name in ("simulst_joiner_scan", "simulst_joiner_emit", "simulst_joiner_scan_beam", "simulst_joiner_mask_blank"):
        at = text.index(f"int {name}(")
        comment = text[text.rindex("/*", 0, at):at]
        assert re.search(r"OPEN source|open source", comment), name
        assert "-1" in comment, name
    at = text.index("int simulst_joiner_emit_beam(")
    comment = text[text.rindex("/*", 0, at):at]              # the beam pair shares one comment
    assert "simulst_joiner_scan_beam" in comment and "emit_log[r] = -1" in comment
    emit = text[text.rindex("/*", 0, text.index("int simulst_joiner_emit(")):text.index("int simulst_joiner_emit(")]
    assert "WAITS" in emit and "at_eos[b] = -1" in emit


def test_package_exports_the_agents():
    import simulst_amd
    from simulst_amd import transducer_agent
    assert simulst_amd.TransducerAgent is transducer_agent.TransducerAgent
    assert simulst_amd.BatchedTransducerStreamingAgent is transducer_agent.BatchedTransducerStreamingAgent
    assert simulst_amd.emit_delays is emit_delays
