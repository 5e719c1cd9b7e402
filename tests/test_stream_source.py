"""The chunk protocol of the synthetic harness (simulst_amd/stream_source.py) against a stub encoder: chunk sizes and positions, the
``finish`` rule in its three spellings, source time, the encoder feed in both modes, the self-paced round loop and the lockstep
bookkeeping.  No GPU."""
import pytest
import torch

from simulst_amd.stream_source import (SHIFT_SIZE, WINDOW_SIZE, ChunkSchedule, FrameSource, LockstepLog, chunk_positions,
                                       encoder_chunks, offline_states, run_rounds, source_ms)

SEG, RC, STRIDE, D = 4, 1, 4, 3
FIRST, NEXT = (SEG + RC) * STRIDE, SEG * STRIDE                       # 20 frames, then 16
TS = [1, 19, 20, 21, 36, 37, 100]


class StubEncoder:
    """segment 4, right context 1, stride 4.  Releases one row per ``STRIDE`` frames, the last ``RC`` of them only with ``finish``
    (a table per call); ``infer`` and ``forward`` return zeros of those shapes and log their calls."""
    segment_length, right_context = SEG, RC

    def __init__(self, skew_at=None):
        self.calls, self.skew_at = [], skew_at

    def conv_layer_stride(self):
        return STRIDE

    def stream_row_schedule(self, positions):
        return [p // STRIDE if i == len(positions) - 1 else max(p // STRIDE - RC, 0) for i, p in enumerate(positions)]

    def infer(self, src_tokens, src_lengths, state, finish=False):
        assert src_lengths.tolist() == [src_tokens.size(1)] * src_tokens.size(0)
        pos, c = src_tokens.size(1), len(self.calls)
        rows = pos // STRIDE if finish else max(pos // STRIDE - RC, 0)
        n = rows - state.get("rows", 0) + (1 if c == self.skew_at else 0)
        state["rows"] = rows
        self.calls.append((pos, finish))
        return {"encoder_out_btd": torch.zeros(src_tokens.size(0), n, D)}

    def forward(self, src_tokens, src_lengths):
        self.calls.append(("forward", src_lengths.tolist()))
        skew = 1 if self.skew_at == "forward" else 0
        B, n = src_tokens.size(0), src_tokens.size(1) // STRIDE + skew
        return {"encoder_out_btd": torch.arange(B * n * D, dtype=torch.float32).view(B, n, D),
                "encoder_lengths": torch.div(src_lengths, STRIDE, rounding_mode="floor") + skew}


def walk(T):
    """the B = 1 loop: take the first size, then the next, until the source has ended -> (positions, flags)"""
    src, positions, flags, expected = FrameSource(torch.zeros(T, 80)), [], [], FIRST
    while not src.finished:
        flags.append(src.take(expected))
        positions.append(src.pos)
        expected = NEXT
    return positions, flags


@pytest.mark.parametrize("T", TS)
def test_positions_finish_flag_and_timing(T):
    sched = ChunkSchedule(StubEncoder(), T, max_len=lambda x: 0.1 * x + 2)
    assert (sched.first_frames, sched.next_frames) == (FIRST, NEXT)
    positions, flags = walk(T)
    assert sched.positions == positions == chunk_positions(T, SEG, RC, STRIDE * SHIFT_SIZE)
    assert positions[-1] == T and positions[0] == min(FIRST, T)
    assert all(b - a == NEXT for a, b in zip(positions[:-2], positions[1:-1]))
    # the three spellings of ``finish``: what take returns (fewer frames than asked, or the source ended), the last position, finished
    assert flags == [i == len(positions) - 1 for i in range(len(positions))]
    assert sched.rows == StubEncoder().stream_row_schedule(positions)
    assert sched.ms == [source_ms(p) for p in positions] == [p * SHIFT_SIZE + WINDOW_SIZE - SHIFT_SIZE for p in positions]
    assert sched.total_ms == source_ms(T) == FrameSource(torch.zeros(T, 80)).total_ms()
    assert sched.max_len == [int(0.1 * p + 2) for p in positions]
    assert ChunkSchedule(StubEncoder(), T).max_len is None


def test_source_ms_and_frame_source():
    assert source_ms(0) == 0 and source_ms(1) == 25 and source_ms(96) == 975
    src = FrameSource(torch.zeros(30, 80))
    assert (src.pos, src.finished, src.elapsed_ms(), src.total_ms()) == (0, False, 0, 315)
    assert src.take(20) is False and src.elapsed_ms() == 215
    assert src.take(16) is True and (src.pos, src.finished, src.elapsed_ms()) == (30, True, 315)
    empty = FrameSource(torch.zeros(0, 80))
    assert empty.finished and empty.elapsed_ms() == 0 and empty.total_ms() == WINDOW_SIZE - SHIFT_SIZE


@pytest.mark.parametrize("T", TS)
def test_feed_chunked(T):
    enc = StubEncoder()
    sched = ChunkSchedule(enc, T)
    positions, flags = walk(T)
    got = list(encoder_chunks(enc, torch.zeros(2, T, 80), sched, "chunked"))
    assert [(c, pos, fin) for c, pos, fin, _ in got] == [(i, p, f) for i, (p, f) in enumerate(zip(positions, flags))]
    assert enc.calls == list(zip(positions, flags))                    # ``finish`` goes to infer on the last call only
    rows = [0] + sched.rows
    assert [tuple(new.shape) for *_, new in got] == [(2, rows[i + 1] - rows[i], D) for i in range(len(positions))]


@pytest.mark.parametrize("T", TS)
def test_feed_chunked_raises_at_the_chunk_that_differs(T):
    n = len(walk(T)[0])
    for bad in sorted({0, n // 2, n - 1}):
        enc = StubEncoder(skew_at=bad)
        it = encoder_chunks(enc, torch.zeros(1, T, 80), ChunkSchedule(enc, T))
        for _ in range(bad):
            next(it)
        with pytest.raises(RuntimeError, match=f"after chunk {bad}, stream_row_schedule predicted"):
            next(it)
        assert len(enc.calls) == bad + 1


@pytest.mark.parametrize("T", TS)
def test_feed_offline(T):
    enc = StubEncoder()
    sched = ChunkSchedule(enc, T)
    positions, flags = walk(T)
    fb = torch.zeros(2, T, 80)
    got = list(encoder_chunks(enc, fb, sched, "offline"))
    assert enc.calls == [("forward", [T, T])]
    assert [(c, pos, fin) for c, pos, fin, _ in got] == [(i, p, f) for i, (p, f) in enumerate(zip(positions, flags))]
    whole = StubEncoder().forward(fb, torch.tensor([T, T]))["encoder_out_btd"]
    assert torch.equal(torch.cat([new for *_, new in got], 1), whole)
    assert [new.size(1) for *_, new in got] == [b - a for a, b in zip([0] + sched.rows, sched.rows)]
    with pytest.raises(RuntimeError, match="offline encoder returned"):
        encoder_chunks(StubEncoder(skew_at="forward"), fb, sched, "offline")
    with pytest.raises(ValueError):
        encoder_chunks(enc, fb, sched, "streaming")


def test_offline_states_ragged():
    """the whole-source hand-over: every row against the schedule of its own length"""
    enc = StubEncoder()
    Ls = [100, 37, 21]
    out, lengths = offline_states(enc, torch.zeros(3, 100, 80), Ls, [ChunkSchedule(enc, t) for t in Ls])
    assert out.shape == (3, 25, D) and lengths.tolist() == [25, 9, 5]
    with pytest.raises(RuntimeError):
        offline_states(enc, torch.zeros(3, 100, 80), Ls, [ChunkSchedule(enc, 100)] * 3)


@pytest.mark.parametrize("T", [21, 100])
@pytest.mark.parametrize("mode", ["chunked", "offline"])
def test_feed_early_stop(T, mode):
    """a consumer that stops after the first chunk: no streaming call was made for a chunk nobody took"""
    enc = StubEncoder()
    it = encoder_chunks(enc, torch.zeros(1, T, 80), ChunkSchedule(enc, T), mode)
    for c, pos, finish, new in it:
        break
    assert enc.calls == ([(FIRST, False)] if mode == "chunked" else [("forward", [T])])
    it.close()
    assert len(enc.calls) == 1


def rounds(first, bound, done_after):
    sizes = []
    run_rounds(sizes.append, lambda: sum(sizes) >= done_after, first, bound, "rows unfinished")
    return sizes


def test_run_rounds():
    """Up to 64 rounds to a call until ``first`` have run, then up to 8 and never past ``bound``.  With first = 70, bound = 75 and
    rows done after 71 rounds the third call therefore asks for the 5 rounds left to the bound (min(8, 75 - 70)), as the loops this
    function replaces did -- not for 1; with the bound one round behind ``first`` (the CIF form's geometry) it is 64, 6, 1."""
    assert rounds(70, 75, 71) == [64, 6, 5]
    assert rounds(70, 71, 71) == [64, 6, 1]
    assert rounds(70, 90, 71) == [64, 6, 8]
    assert rounds(70, 90, 60) == [64]                                  # one look per call: rows that met EOS early end it there
    assert rounds(200, 203, 203) == [64, 64, 64, 8, 3]
    sizes = []
    with pytest.raises(RuntimeError, match="rows unfinished"):
        run_rounds(sizes.append, lambda: False, 70, 75, "rows unfinished")
    assert sizes == [64, 6, 5]


def test_lockstep_log():
    """three rows over three chunks: row 0 writes two tokens after chunk 1 and is done; row 1 writes one token after chunk 1, two
    after chunk 2 and ends at chunk 3 without another; row 2 never writes"""
    log = LockstepLog(3)
    log.read()
    log.wrote([2, 1, 0], [1, 0, 0])
    assert log.alive == [1, 2] and log.n_written == [2, 1, 0]
    log.read()
    log.wrote([2, 3, 0], [1, 0, 0])
    log.read()
    log.wrote([2, 3, 0], [1, 1, 0])
    assert log.alive == [2]
    assert ["".join(a) for a in log.actions] == ["RWW", "RWRWWR", "RRR"]
    hyp = torch.tensor([[7, 2, 0, 0], [5, 6, 2, 0], [0, 0, 0, 0]])
    delays = torch.tensor([[215, 215, 0, 0], [215, 375, 375, 0], [0, 0, 0, 0]], dtype=torch.int32)
    recs = log.records(hyp, delays, 535, "n_enc", lambda b: 10 + b)
    assert recs == [
        {"tokens": [7, 2], "delays_ms": [215, 215], "actions": "RWW", "AL": (215 + (215 - 1 / (2 / 535))) / 2, "n_enc": 10},
        {"tokens": [5, 6, 2], "delays_ms": [215, 375, 375], "actions": "RWRWWR", "AL": (215 + (375 - 1 / (3 / 535)) + (375 - 2 / (3 / 535))) / 3,
         "n_enc": 11},
        {"tokens": [], "delays_ms": [], "actions": "RRR", "AL": 0.0, "n_enc": 12}]
    assert all(type(d) is int for r in recs for d in r["delays_ms"])
