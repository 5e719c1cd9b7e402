"""The chunk protocol of the synthetic harness (DESIGN.md "Synthetic harness"), stated once for every streaming agent:

* the first READ offers (segment + right context) * stride fbank frames, every later one segment * stride
  (agents/default_agent.py:367,407), fewer at the end;
* the READ that ends the source carries ``finish`` (the encoder flushes its look-ahead rows, agents/default_agent.py:303-342);
* a token is stamped with the source milliseconds released so far, ``source_ms``.

Host code only: nothing here loads the native library, so the protocol is tested without a GPU (tests/test_stream_source.py).
"""
import torch

SHIFT_SIZE, WINDOW_SIZE = 10, 25


def source_ms(pos: int) -> int:
    """milliseconds of source released after pos fbank frames"""
    return 0 if pos == 0 else pos * SHIFT_SIZE + WINDOW_SIZE - SHIFT_SIZE


def total_source_ms(T: int) -> int:
    """the length of a whole source of T frames: one window even when it holds no frame (Average Lagging divides by it)"""
    return source_ms(T) or WINDOW_SIZE - SHIFT_SIZE


def chunk_frames(segment_length: int, right_context: int, stride_ms: int):
    """(frames the first READ offers, frames every later READ offers)"""
    return (segment_length + right_context) * stride_ms // SHIFT_SIZE, segment_length * stride_ms // SHIFT_SIZE


def chunk_positions(T: int, segment_length: int, right_context: int, stride_ms: int):
    """Source frames offered after each READ, cumulative; the last entry is T."""
    expected, nxt = chunk_frames(segment_length, right_context, stride_ms)
    pos, out = 0, []
    while pos < T:
        pos = min(pos + expected, T)
        out.append(pos)
        expected = nxt
    return out


class FrameSource:
    def __init__(self, fbank: torch.Tensor):
        self.fbank = fbank
        self.pos = 0
        self.finished = self.finish = fbank.size(0) == 0

    def read(self, n: int):
        """Release the next n frames, fewer at the end.  ``finish`` is the flag the encoder call over them carries: fewer frames than
        asked, or the source ended.  The two say the same (the read clamps at the end, and chunk_positions ends exactly there)."""
        start = self.pos
        self.pos = min(self.pos + n, self.fbank.size(0))
        self.finished = self.pos >= self.fbank.size(0)
        self.finish = self.pos - start < n or self.finished

    def take(self, expected: int) -> bool:
        self.read(expected)
        return self.finish

    def elapsed_ms(self):
        return source_ms(self.pos)

    def total_ms(self):
        return total_source_ms(self.fbank.size(0))


class ChunkSchedule:
    """Everything the protocol fixes for a source of T frames before a single frame is read: ``positions`` (frames offered after each
    READ), ``rows`` (encoder rows released, cumulative: encoder.stream_row_schedule), ``ms`` (source time of every READ), ``max_len``
    (the agent's length cap at every READ; None for an agent without one) and ``total_ms``."""

    def __init__(self, enc, T: int, max_len=None):
        stride_ms = enc.conv_layer_stride() * SHIFT_SIZE
        self.first_frames, self.next_frames = chunk_frames(enc.segment_length, enc.right_context, stride_ms)
        self.positions = chunk_positions(T, enc.segment_length, enc.right_context, stride_ms)
        self.rows = list(enc.stream_row_schedule(self.positions))
        self.ms = [source_ms(p) for p in self.positions]
        self.max_len = [int(max_len(p)) for p in self.positions] if max_len is not None else None
        self.total_ms = total_source_ms(T)


class ChunkedAgent:
    """What the four agent families share: the chunk geometry of the model's encoder and the schedule of a source of T frames.
    ``max_len`` (frames read -> tokens allowed) is each agent's own."""
    max_len = None

    def _init_chunks(self, model):
        enc = model.encoder
        self.stride_ms = enc.conv_layer_stride() * SHIFT_SIZE
        self.right_context, self.segment_length = enc.right_context, enc.segment_length
        self.first_frames, self.next_frames = chunk_frames(self.segment_length, self.right_context, self.stride_ms)
        self.eos = model.cfg.eos
        self._schedules = {}

    def _chunk_positions(self, T: int):
        return chunk_positions(T, self.segment_length, self.right_context, self.stride_ms)

    def _schedule(self, T: int) -> ChunkSchedule:
        """cached per T: a ragged self-paced batch asks for one schedule per distinct length, every batch again"""
        if T not in self._schedules:
            self._schedules[T] = ChunkSchedule(self.model.encoder, T, self.max_len)
        return self._schedules[T]


def _emformer(enc, name: str):
    """The Emformer's own ``infer`` / ``forward`` of enc.  CIFEncoder, the only subclass that overrides them, integrates the rows
    behind the encoder; the batched forms and the CTC head do not want that."""
    from .encoder import S2TEmformerEncoder
    fn = getattr(S2TEmformerEncoder if isinstance(enc, S2TEmformerEncoder) else type(enc), name)
    return lambda *a, **kw: fn(enc, *a, **kw)


def offline_states(enc, fbank: torch.Tensor, Ls, schedules):
    """One offline forward over whole sources of Ls[b] frames (fbank [B, T, 80] padded) -> (rows [B, n, D], their lengths [B] on the
    device).  The lengths must be the rows schedules[b] releases in all."""
    e = _emformer(enc, "forward")(fbank, torch.tensor(Ls, device=fbank.device))
    got, want = e["encoder_lengths"].tolist(), [s.rows[-1] for s in schedules]
    if got != want:
        raise RuntimeError(f"offline encoder returned {got} rows, stream_row_schedule predicted {want}")
    return e["encoder_out_btd"], e["encoder_lengths"]


def encoder_chunks(enc, fbank: torch.Tensor, schedule: ChunkSchedule, encoder: str = "chunked"):
    """The encoder rows of B sources of equal length, chunk by chunk: yields (c, pos, finish, new rows [B, n, D]).
    "chunked": the streaming encoder over fbank[:, :pos], one call per chunk, run when the consumer asks for that chunk -- a consumer
    that stops early leaves no call behind.  "offline": one forward, run here, cut at the rows the schedule releases."""
    if encoder not in ("chunked", "offline"):
        raise ValueError(f"encoder={encoder!r}: 'chunked' or 'offline'")
    B, n = fbank.size(0), len(schedule.positions)
    if encoder == "offline":
        out, _ = offline_states(enc, fbank, [schedule.positions[-1]] * B, [schedule] * B)
        return ((c, pos, c == n - 1, out[:, (schedule.rows[c - 1] if c else 0):schedule.rows[c]])
                for c, pos in enumerate(schedule.positions))
    infer = _emformer(enc, "infer")

    def chunked():
        state, got = {}, 0
        for c, pos in enumerate(schedule.positions):
            new = infer(fbank[:, :pos], torch.full((B,), pos), state, finish=c == n - 1)["encoder_out_btd"]
            got += new.size(1)
            if got != schedule.rows[c]:
                raise RuntimeError(f"streaming encoder released {got} rows after chunk {c}, stream_row_schedule predicted "
                                   f"{schedule.rows[c]}")
            yield c, pos, c == n - 1, new
    return chunked()


def run_rounds(step, finished, first: int, bound: int, what: str):
    """The device loop of a self-paced form: ``step(n)`` launches n rounds, ``finished()`` is the one read-back per call.  No row can
    finish in fewer than ``first`` rounds, so that many go out (64 to a call) before the first look; short calls (8) after it.  A run
    still unfinished after ``bound`` rounds is an error."""
    n_run = 0
    while True:
        n = max(1, min(64, first - n_run) if n_run < first else min(8, bound - n_run))
        step(n)
        n_run += n
        if finished():
            return
        if n_run >= bound:
            raise RuntimeError(what)


class LockstepLog:
    """Host bookkeeping of a lockstep form whose WRITEs happen in a device loop: the READ / WRITE string of every row, the tokens it
    holds, and the rows still running."""

    def __init__(self, B: int):
        self.actions = [[] for _ in range(B)]
        self.n_written = [0] * B
        self.alive = list(range(B))

    def read(self):
        for b in self.alive:
            self.actions[b].append("R")

    def wrote(self, n_prev, done):
        """n_prev[b]: tokens row b holds now; done[b]: it has ended"""
        for b in self.alive:
            self.actions[b].extend("W" * (n_prev[b] - self.n_written[b]))
            self.n_written[b] = n_prev[b]
        self.alive = [b for b in self.alive if not done[b]]

    def records(self, hyp, delays, total_ms, extra_key, extra_of):
        from .latency import average_lagging
        hyp_h, delays_h = hyp.tolist(), delays.tolist()
        recs = []
        for b, n in enumerate(self.n_written):
            d = [int(x) for x in delays_h[b][:n]]
            recs.append({"tokens": hyp_h[b][:n], "delays_ms": d, "actions": "".join(self.actions[b]),
                         "AL": average_lagging(d, total_ms), extra_key: extra_of(b)})
        return recs
