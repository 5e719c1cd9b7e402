"""transducer_model on MI355X: inference of models/transducer_model.py:28-212 -- the Emformer encoder, an average-pool
downsample of its states (AvgPool1dTBCPad, :79-98), a self-attention-only prediction network (fairseq's TransformerDecoder with
no_encoder_attn, :101-122,158-162) and the joiner (:28-76) with its greedy emission (:163-209).

Per decode step the reference scores every source position of every row against the whole vocabulary,
``W_out tanh(source_projection(pooled[b, s]) + target_projection(features[b]))``, as a [B, S, V] tensor, and keeps an argmax per
position.  Here ``P = source_projection(pooled)`` is computed once per utterance, and a step is: the prediction network on the
per-op kernels, ``g = target_projection(features)``, simulst_joiner_scan (blank logit and best non-blank per remaining position, on
the matrix cores, never the [B, S, V] tensor), simulst_joiner_emit (the first position whose non-blank wins, the blank forced out
at the row's last position), and simulst_linear of the emitted position's tanh row.

Beam search (``beam_offline``, ``TransducerModel.generate``): simulst_amd/beam.py's loop over that step, every one of the
Bs * beam rows with its own prev_emit and prediction-network K/V prefix.  P stays [Bs, S', D]: simulst_joiner_scan_beam /
simulst_joiner_emit_beam read it at row / beam and skip finished sentences, and simulst_transducer_beam_reorder moves the K/V
prefixes and prev_emit behind every selection.  The blank (bos) is an ordinary candidate token wherever it is not forced out, as
fairseq's SequenceGenerator over the reference's decoder treats it.  ``forward`` + ``reorder_incremental_state`` are that
decoder's call shape for an outside generator.

The module registers nothing at import (the local registries hold the three models of the streaming agents); ``register()`` adds
``transducer_model`` / ``transducer_model_s``, and registry.build_model_from_args / checkpoint.load call it when that name is asked
for.

Scoring a given translation (the forward value of criterion/rnnt_criterion.py:82-147): ``forward_lattice`` runs the prediction
network over the whole target at once (``features_teacher_forced``), then simulst_joiner_lattice -- log p(blank) and log p(label) of
every (source position, target position) cell, the reference's [B, S', U + 1, V] logits never written -- and
``TransducerModel.score_reference`` adds simulst_rnnt_forward: the log-likelihood summed over all monotonic alignments, the best
alignment with the frame each token is emitted at, and the "offline path" term.  Gradients (the training criterion), FastEmit (it
acts on gradients only) and label smoothing are out of scope.

Simultaneous decoding (``open_source`` / ``append_source`` / ``step_online``; the agents are in simulst_amd/transducer_agent.py):
the source grows window by window and the scan / emit kernels are told so by a negative src_len (-1 - available positions): no
position is forced, and a row in which none of the available positions emits WAITS -- prev_emit, z and its target position stay.
That is the case the reference's rollback (:214-239, not callable as written) exists for; here nothing is rolled back, the step
commits per row.  What is written this way is what ``greedy_offline`` writes; only the delays are new.
"""
import math
from typing import Dict, List, Optional

import torch

from .config import ModelConfig
from .decoder import (_DecoderLayerView, _Dictionary, ensure_positions, feed_forward_block, load_decoder_stack, regrow,
                      self_attention_block, source_lengths)
from .encoder import S2TEmformerEncoder
from .model import FairseqModelSurface, _default, s2t_emformer_s
from .ops import EPI_BIAS_F32OUT, Ops

BLANK = 0          # the blank is bos (models/transducer_model.py:140,176,195)
BLANK_AT_EOS = -1e4


class TransducerWeights:
    """prediction network + joiner weights on the device"""

    def __init__(self, w: Dict[str, torch.Tensor], cfg: ModelConfig, device, dtype, ops: Ops, prefix="decoder"):
        W, Bv = load_decoder_stack(self, w, cfg, device, dtype, prefix)
        p = prefix
        # joiner (:28-58)
        self.w_src, self.b_src = W(f"{p}.joiner.source_projection.weight"), Bv(f"{p}.joiner.source_projection.bias")
        self.w_tgt = W(f"{p}.joiner.target_projection.weight")
        self.out_proj_fm = ops.pack_joiner_weight(self.out_proj)        # the scan's B operand (rows padded to whole 16-column tiles)
        torch.cuda.synchronize(device)


class TransducerState:
    """Device-resident incremental state of one hypothesis batch: the self-attention caches, P, src_len', prev_emit, g."""

    def __init__(self, cfg: ModelConfig, B: int, cap: int, device, dtype):
        H, d = cfg.num_heads, cfg.head_dim
        self.B, self.cap = B, cap
        self.k_cache = [torch.zeros(B, H, cap, d, device=device, dtype=dtype) for _ in range(cfg.decoder_layers)]
        self.v_cache = [torch.zeros(B, H, cap, d, device=device, dtype=dtype) for _ in range(cfg.decoder_layers)]
        self.n_prev = torch.zeros(B, device=device, dtype=torch.int32)
        self.n_prev_host = 0
        self.kv_rows = 0                 # K/V positions written so far, the uncommitted newest one included (forward())
        self.reorder_buf = None          # beam.ReorderBuffers: second K/V + prev_emit set of the beam reorder
        self.P = None                    # [B, S', D] fp32
        self.pooled = None               # [B, S', D] model dtype
        self.src_len = None              # [B] int32 (src_len')
        self.prev_emit = torch.zeros(B, device=device, dtype=torch.int32)
        self.g = None                    # [B, D] fp32, the last step's target projection
        self.enc_rows = -1               # encoder rows the pooled states were made from (forward())
        # the emit position BEFORE the step that wrote token t (forward(): a repeated prefix restarts from it)
        self.emit_before: List[torch.Tensor] = []

    def grow(self, cap: int):
        if cap > self.cap:
            if self.reorder_buf is not None:
                self.reorder_buf.grow(cap)           # both sets
            else:
                self.k_cache, self.v_cache = regrow(self.k_cache, cap), regrow(self.v_cache, cap)
            self.cap = cap


class TransducerDecoder:
    """Mirror of models/transducer_model.py:TransducerDecoder (inference, incremental)."""

    STATE_KEY = "simulst_amd.transducer_state"

    def __init__(self, cfg: ModelConfig, weights: Dict[str, torch.Tensor], device="cuda", dtype=torch.float32,
                 ops: Optional[Ops] = None, prefix="decoder", lattice_logits_cap_bytes: int = 1 << 30):
        if cfg.downsample < 1:
            raise ValueError(f"--downsample {cfg.downsample}: a window of at least 1")
        self.cfg = cfg
        self.lattice_logits_cap_bytes = int(lattice_logits_cap_bytes)      # forward_lattice(return_logits=True) refuses above it
        self.device, self.dtype = torch.device(device), dtype
        self.ops = ops or Ops()
        self.w = TransducerWeights(weights, cfg, self.device, dtype, self.ops, prefix)
        self.embed_scale = 1.0 if cfg.no_scale_embedding else math.sqrt(cfg.embed_dim)
        self.layers = [_DecoderLayerView(cfg, l) for l in range(cfg.decoder_layers)]
        self.dictionary = _Dictionary(cfg)

    def max_positions(self):
        return self.cfg.max_target_positions

    # ------------------------------------------------------------------ source side
    def new_state(self, B: int, cap: int = 128) -> TransducerState:
        ensure_positions(self.w, cap + self.cfg.padding_idx + 2)
        return TransducerState(self.cfg, B, cap, self.device, self.dtype)

    def downsample(self, enc_btd: torch.Tensor, enc_len: torch.Tensor, T: Optional[int] = None):
        """AvgPool1dTBCPad (:79-98) -> (pooled [B, S', D], src_len' [B] int32).  T: the batch's longest valid length (the reference's
        time dimension; read from enc_len when not given).  downsample == 1: the reference has no pooling op (:104-108)."""
        lens = enc_len.to(device=self.device, dtype=torch.int32).contiguous()
        if T is None:
            T = int(lens.max().item())
        T = max(1, min(int(T), enc_btd.size(1)))
        return self.ops.transducer_pool(enc_btd, lens, T_max=T, k=self.cfg.downsample)

    def set_source(self, st: TransducerState, enc_btd: torch.Tensor, enc_len: torch.Tensor, T: Optional[int] = None,
                   rows: Optional[int] = None):
        """pool the encoder states and project them once per utterance: P = source_projection(pooled) (:64), fp32.  rows: the
        state's row count when several rows share an utterance (beam search: P stays per utterance, the step's buffers are per row)"""
        Bs, _, D = enc_btd.shape
        st.pooled, st.src_len = self.downsample(enc_btd.to(self.dtype), enc_len, T)
        S = st.pooled.size(1)
        st.P = self.ops.linear(st.pooled.view(Bs * S, D), self.w.w_src, self.w.b_src, epilogue=EPI_BIAS_F32OUT).view(Bs, S, D)
        B = Bs if rows is None else int(rows)
        n_split = Ops.joiner_split(B, S, self.cfg.vocab, self.dtype)
        st.blank_logit = torch.empty(B, S, device=self.device, dtype=torch.float32)
        st.best = torch.empty(B, S, n_split, device=self.device, dtype=torch.float32)
        st.best_idx = torch.empty(B, S, n_split, device=self.device, dtype=torch.int32)
        st.z = torch.empty(B, D, device=self.device, dtype=self.dtype)
        st.at_eos = torch.empty(B, device=self.device, dtype=torch.int32)
        st.prev_emit.zero_()
        st.emit_before = []
        st.enc_rows = enc_btd.size(1)

    # ------------------------------------------------------------------ one decode step
    def features(self, st: TransducerState, last_tokens: torch.Tensor) -> torch.Tensor:
        """prediction network on the newest token of [bos] + hypothesis (:158-162): TransformerDecoder.extract_features with
        self-attention + GELU feed-forward layers only -> [B, D]"""
        ops, cfg, Wd = self.ops, self.cfg, self.w
        ensure_positions(Wd, st.cap + cfg.padding_idx + 2)
        if st.n_prev_host == 0:          # prev_output_tokens[:, 0] = bos (:144), whatever the caller's first token is
            last_tokens = torch.full_like(last_tokens, BLANK)
        pos_row = (st.n_prev + (cfg.padding_idx + 1)).contiguous()
        x = ops.embed_tokens(last_tokens, Wd.E, Wd.pos, pos_row, self.embed_scale)

        def attend(qkv, l):
            return ops.decoder_self_attention(qkv, st.k_cache[l], st.v_cache[l], st.n_prev)

        for l, L in enumerate(Wd.layers):
            x = self_attention_block(ops, L, x, attend, l)
            x = feed_forward_block(ops, L, x)
        return ops.layernorm(x, Wd.ln_g, Wd.ln_b)

    def step(self, st: TransducerState, last_tokens: torch.Tensor) -> torch.Tensor:
        """One target position for every row: last_tokens [B] int64 (the newest of [bos] + hypothesis) -> logits [B, V] fp32 of
        the position each row emits at (:163-209); st.prev_emit moves there."""
        ops, V = self.ops, self.cfg.vocab
        feats = self.features(st, last_tokens.to(device=self.device, dtype=torch.int64).contiguous())
        st.g = ops.linear(feats, self.w.w_tgt, None, epilogue=EPI_BIAS_F32OUT)            # target_projection, no bias (:40-44)
        ops.joiner_scan(st.P, st.g, self.w.out_proj_fm, st.prev_emit, st.src_len, st.blank_logit, st.best, st.best_idx, V=V, blank=BLANK)
        ops.joiner_emit(st.P, st.g, st.blank_logit, st.best, st.best_idx, st.prev_emit, st.src_len, st.z, st.at_eos, V=V, blank=BLANK)
        logits = ops.linear(st.z, self.w.out_proj, None, epilogue=EPI_BIAS_F32OUT)
        return ops.joiner_mask_blank(logits, st.at_eos, blank=BLANK)

    def commit(self, st: TransducerState):
        """Advance the target position after a token is kept (the K/V row appended by step() becomes permanent)."""
        st.n_prev += 1
        st.n_prev_host += 1
        if st.n_prev_host + 1 >= st.cap:
            st.grow(2 * st.cap)

    def greedy_offline(self, enc_btd: torch.Tensor, enc_len: torch.Tensor, n_steps: int, mask_eos: bool = False,
                       T: Optional[int] = None, *, mask_first_eos: bool = True, until_all_eos: bool = False):
        """Batched greedy decode (beam 1; pad never, EOS masked at the first step as SequenceGenerator's min_len 1 unless
        mask_first_eos=False).  Returns (tokens [B, n_steps] int64, emit [B, n_steps] int32 -- the pooled frame each token was
        emitted at, state).  until_all_eos: the loop looks every 8 steps whether every row has written an EOS and stops there;
        the returned tokens / emit then have that many columns (the simultaneous evaluation form, which cuts every row at its
        EOS anyway)."""
        cfg, ops = self.cfg, self.ops
        B = enc_btd.size(0)
        st = self.new_state(B, cap=n_steps + 2)
        self.set_source(st, enc_btd, enc_len, T)
        toks = torch.full((B,), BLANK, device=self.device, dtype=torch.int64)
        out = torch.empty(n_steps, B, device=self.device, dtype=torch.int64)
        emit = torch.empty(n_steps, B, device=self.device, dtype=torch.int32)
        n_done = n_steps
        for s in range(n_steps):
            logits = self.step(st, toks)
            toks = ops.greedy_argmax(logits, pad_idx=cfg.padding_idx, eos_idx=cfg.eos, mask_eos=mask_eos or (mask_first_eos and s == 0),
                                     out=out[s])
            emit[s].copy_(st.prev_emit)
            self.commit(st)
            if until_all_eos and s % 8 == 7 and bool((out[:s + 1] == cfg.eos).any(0).all().item()):
                n_done = s + 1
                break
        return out[:n_done].t().contiguous(), emit[:n_done].t().contiguous(), st

    # ------------------------------------------------------------------ a source that grows (simultaneous decoding)
    def open_source(self, st: TransducerState, S_cap: int):
        """Start an OPEN source of up to S_cap pooled positions (more make the buffers grow): P, the scan buffers and z are
        allocated, no position is available yet (st.avail = 0) and every row is open (st.open = 1).  The kernels read
        st.src_len = -1 - avail for an open row (include/simulst_hip.h: nothing is forced, a row may wait), avail for a closed one."""
        B, D, dev = st.B, self.cfg.embed_dim, self.device
        S_cap = max(int(S_cap), 1)
        st.P = torch.zeros(B, S_cap, D, device=dev, dtype=torch.float32)
        st.pooled = torch.zeros(B, S_cap, D, device=dev, dtype=self.dtype)
        self._scan_buffers(st, S_cap)
        st.z = torch.zeros(B, D, device=dev, dtype=self.dtype)
        st.at_eos = torch.full((B,), -1, device=dev, dtype=torch.int32)
        st.prev_emit.zero_()
        st.emit_before = []
        st.enc_rows = 0
        st.avail_host, st.open_host = [0] * B, [1] * B
        st.done = torch.zeros(B, device=dev, dtype=torch.int32)          # rows a driver has ended: they scan nothing and wait
        st.left = torch.zeros(B, max(self.cfg.downsample - 1, 1), D, device=dev, dtype=self.dtype)     # rows of an incomplete window
        st.left_host = [0] * B
        st.g, st.g_fresh = None, False
        st.n_wrote = 0                                                   # rows that wrote in the last step_online round (host)
        st.scan_hi = torch.zeros(B, device=dev, dtype=torch.int32)       # positions below it hold the scan of the row's current g
        st.n_prev.zero_()
        st.n_prev_host = 0
        self.sync_source(st)

    def _scan_buffers(self, st: TransducerState, S: int):
        B, dev = st.B, self.device
        n_split = Ops.joiner_split(B, S, self.cfg.vocab, self.dtype)
        st.blank_logit = torch.empty(B, S, device=dev, dtype=torch.float32)
        st.best = torch.empty(B, S, n_split, device=dev, dtype=torch.float32)
        st.best_idx = torch.empty(B, S, n_split, device=dev, dtype=torch.int32)

    def sync_source(self, st: TransducerState):
        """st.avail / st.open / st.src_len on the device from the host counts.  A row the driver has ended (st.done), and a closed
        row without a single position, read as open with nothing available: they wait."""
        i32 = dict(device=self.device, dtype=torch.int32)
        st.avail, st.open = torch.tensor(st.avail_host, **i32), torch.tensor(st.open_host, **i32)
        waits = (st.open != 0) | (st.avail == 0)
        st.src_len = torch.where(st.done != 0, torch.full_like(st.avail, -1), torch.where(waits, -1 - st.avail, st.avail)).contiguous()

    def _grow_source(self, st: TransducerState, S_need: int):
        S_old = st.P.size(1)
        if S_need <= S_old:
            return
        S_new = max(S_need, 2 * S_old)
        for name in ("P", "pooled"):
            old = getattr(st, name)
            new = torch.zeros(old.size(0), S_new, old.size(2), device=old.device, dtype=old.dtype)
            new[:, :S_old] = old
            setattr(st, name, new)
        self._scan_buffers(st, S_new)
        st.scan_hi.zero_()                                   # the scan buffers' layout changed: every row scans from prev_emit again

    def append_source(self, st: TransducerState, enc_rows: torch.Tensor, n_new, finish=False):
        """More encoder states for an open source: enc_rows [B, n, D], of which the first n_new[b] are row b's (an int: every row's);
        finish (one flag, or one per row): the source of the row ends here.  Only COMPLETE windows of k = cfg.downsample encoder
        rows are pooled (simulst_transducer_pool) and projected into P; the < k rows behind them are carried to the next call.  On
        finish the partial last window is flushed as the mean of its valid rows -- what AvgPool1dTBCPad gives a row that is not the
        batch's longest -- and the row is closed: its last position is then forced as in the offline decode."""
        cfg, ops, k = self.cfg, self.ops, self.cfg.downsample
        B, n, D = enc_rows.shape
        assert B == st.B
        n_new = [int(n_new)] * B if isinstance(n_new, int) else [int(x) for x in (n_new.tolist() if torch.is_tensor(n_new) else n_new)]
        fin = [bool(finish)] * B if isinstance(finish, (bool, int)) else [bool(x) for x in finish]
        assert len(n_new) == B and len(fin) == B and all(0 <= x <= n for x in n_new)
        for b in range(B):
            if not st.open_host[b] and (n_new[b] > 0 or st.left_host[b] > 0):
                raise ValueError(f"append_source: the source of row {b} is closed")
        total = [st.left_host[b] + n_new[b] for b in range(B)]
        lens = [t if fin[b] else t // k * k for b, t in enumerate(total)]               # the rows pooled now
        wins = [(x + k - 1) // k for x in lens]
        enc_rows = enc_rows.to(device=self.device, dtype=self.dtype)
        uniform = len(set(st.left_host)) == 1 and len(set(n_new)) == 1 and len(set(st.avail_host)) == 1 and len(set(wins)) == 1
        rows = (max(total) + k - 1) // k * k                                           # whole windows: the pool never clips one
        if rows > 0:
            X = torch.zeros(B, rows, D, device=self.device, dtype=self.dtype)
            if uniform:
                l0 = st.left_host[0]
                X[:, :l0] = st.left[:, :l0]
                X[:, l0:l0 + n_new[0]] = enc_rows[:, :n_new[0]]
            else:
                for b in range(B):
                    l0 = st.left_host[b]
                    X[b, :l0] = st.left[b, :l0]
                    X[b, l0:l0 + n_new[b]] = enc_rows[b, :n_new[b]]
            keep = [t - x for t, x in zip(total, lens)]                                # the rows behind the last complete window
            if uniform and len(set(keep)) == 1:
                st.left[:, :keep[0]] = X[:, lens[0]:total[0]]
            else:
                for b in range(B):
                    st.left[b, :keep[b]] = X[b, lens[b]:total[b]]
            st.left_host = keep
        W = max(wins)
        if W > 0:
            self._grow_source(st, max(a + w for a, w in zip(st.avail_host, wins)))
            Y, _ = ops.transducer_pool(X, torch.tensor(lens, device=self.device, dtype=torch.int32), T_max=W * k, k=k)       # [B, W, D]
            Pn = ops.linear(Y.view(B * W, D), self.w.w_src, self.w.b_src, epilogue=EPI_BIAS_F32OUT).view(B, W, D)
            if uniform:
                a0 = st.avail_host[0]
                st.pooled[:, a0:a0 + W] = Y
                st.P[:, a0:a0 + W] = Pn
            else:
                for b in range(B):
                    a0, w = st.avail_host[b], wins[b]
                    st.pooled[b, a0:a0 + w] = Y[b, :w]
                    st.P[b, a0:a0 + w] = Pn[b, :w]
        for b in range(B):
            st.avail_host[b] += wins[b]
            if fin[b]:
                st.open_host[b] = 0
        st.enc_rows += max(n_new) if n_new else 0
        self.sync_source(st)

    def step_online(self, st: TransducerState, last_tokens: torch.Tensor, *, recompute_g: bool = False):
        """One round over an open source: last_tokens [B] int64 -> (logits [B, V] fp32, wrote [B] bool).  A row writes if one of
        its available positions emits (or its source is closed: the last position is forced); its logits row, st.prev_emit and
        st.z are then those of ``step``, and the round is committed for it: st.n_prev[b] += 1.  A row that WAITS keeps prev_emit,
        z and n_prev -- nothing is rolled back, the K/V row the round appended at n_prev[b] is overwritten by the next one -- and
        its logits row is meaningless.  st.n_wrote is the number of rows that wrote, on the host (the round's one read-back).
        The waiting rows keep their g: while NO row has written since g was computed (the round behind a new chunk, when every
        live row waits), the next round skips the prediction network and scans only the positions that arrived since
        (st.scan_hi).  The cache is per batch, not per row: once some row has written, the network and the scan run for every
        row again, which gives a waiting row the bits it had.  recompute_g=True is the simpler form that does so every round
        (tools/transducer_stream_bench.py times the two)."""
        ops, V = self.ops, self.cfg.vocab
        toks = last_tokens.to(device=self.device, dtype=torch.int64).contiguous()
        if recompute_g or not st.g_fresh or st.g is None:
            toks = torch.where(st.n_prev == 0, torch.full_like(toks, BLANK), toks)          # a row's first input is bos (:144)
            feats = self.features(st, toks)
            st.g = ops.linear(feats, self.w.w_tgt, None, epilogue=EPI_BIAS_F32OUT)
            st.scan_hi.zero_()
        lo = torch.maximum(st.prev_emit, st.scan_hi)
        ops.joiner_scan(st.P, st.g, self.w.out_proj_fm, lo, st.src_len, st.blank_logit, st.best, st.best_idx, V=V, blank=BLANK)
        st.scan_hi.copy_(torch.where(st.done != 0, st.scan_hi, st.avail))
        ops.joiner_emit(st.P, st.g, st.blank_logit, st.best, st.best_idx, st.prev_emit, st.src_len, st.z, st.at_eos, V=V, blank=BLANK)
        logits = ops.linear(st.z, self.w.out_proj, None, epilogue=EPI_BIAS_F32OUT)
        ops.joiner_mask_blank(logits, st.at_eos, blank=BLANK)
        wrote = st.at_eos >= 0
        st.n_prev += wrote.to(torch.int32)
        n_wrote, n_max = torch.stack([wrote.sum().to(torch.int32), st.n_prev.max()]).tolist()            # the round's one look at the device
        st.n_wrote = int(n_wrote)
        st.g_fresh = n_wrote == 0                  # g belongs to the rows' prefixes: it stays while none of them grows
        st.n_prev_host = int(n_max)
        if st.n_prev_host + 1 >= st.cap:
            st.grow(2 * st.cap)
        return logits, wrote

    # ------------------------------------------------------------------ beam search
    def beam_offline(self, enc_btd: torch.Tensor, enc_len: torch.Tensor, max_len, *, beam: int, lenpen: float = 1.0, nbest: int = 1,
                     chunk: int = 8, T: Optional[int] = None):
        """Beam search with fairseq's SequenceGenerator semantics (simulst_amd/beam.py, DESIGN.md "Beam search") over the
        reference's incremental transducer step: enc_btd [Bs, S_in, D], enc_len [Bs], max_len an int or one cap per sentence (at
        most max_len[s] tokens and EOS).  Row s * beam + j carries its own prev_emit and prediction-network K/V prefix; its logits
        row is the joiner's row at the position it emits at, the blank forced to -1e4 at the sentence's last pooled position and an
        ordinary candidate everywhere else.  The source is set once for the Bs sentences (P is not replicated); behind every
        selection the step is committed and simulst_transducer_beam_reorder moves K/V prefixes and prev_emit into the state's
        second set, and the sets swap.  Returns (tokens [Bs, nbest, L] int64, lengths [Bs, nbest] int32, scores [Bs, nbest] fp32,
        positional scores [Bs, nbest, L] fp32, emit [Bs, nbest, L] int32 -- the pooled frame each token of the hypothesis (its EOS
        included) was emitted at, -1 behind it --, stats {"steps"}), on the device; L = max(max_len) + 1."""
        from .beam import BeamSearch, ReorderBuffers, check_args, sentence_caps
        cfg, ops, V = self.cfg, self.ops, self.cfg.vocab
        Bs = enc_btd.size(0)
        caps = sentence_caps(max_len, Bs)
        check_args(beam, nbest, V)
        R = Bs * beam
        bs = BeamSearch(ops, caps, beam=beam, V=V, eos=cfg.eos, pad=cfg.padding_idx, lenpen=lenpen, nbest=nbest, device=self.device)
        st = self.new_state(R, cap=bs.L + 2)
        self.set_source(st, enc_btd.to(self.device), enc_len, T, rows=R)
        buf = ReorderBuffers.of(st, extra=("prev_emit",))
        cap0 = st.cap
        emit_log = torch.full((bs.L, R), -1, device=self.device, dtype=torch.int32)

        def logits_fn(t, toks):
            feats = self.features(st, toks)
            st.g = ops.linear(feats, self.w.w_tgt, None, epilogue=EPI_BIAS_F32OUT)
            ops.joiner_scan_beam(st.P, st.g, self.w.out_proj_fm, st.prev_emit, st.src_len, bs.finished, st.blank_logit, st.best,
                                 st.best_idx, group=beam, V=V, blank=BLANK)
            ops.joiner_emit_beam(st.P, st.g, st.blank_logit, st.best, st.best_idx, st.prev_emit, st.src_len, bs.finished, st.z,
                                 st.at_eos, emit_log[t], group=beam, V=V, blank=BLANK)
            logits = ops.linear(st.z, self.w.out_proj, None, epilogue=EPI_BIAS_F32OUT)
            return ops.joiner_mask_blank(logits, st.at_eos, blank=BLANK)

        def after_select(t):
            self.commit(st)
            assert st.cap == cap0, "beam state outgrew its capacity"
            ops.transducer_beam_reorder(buf.desc, buf.src, buf.dst, st.prev_emit, buf.other["prev_emit"], bs.reorder, bs.finished,
                                        bs.result[2:3], block=beam, n_prev=st.n_prev_host)
            buf.swap()

        tokens, lengths, scores, pos = bs.run(logits_fn, after_select, chunk=chunk)
        emit = self._hypothesis_emit(bs, emit_log).to(self.device)
        return tokens, lengths, scores, pos, emit, {"steps": bs.steps}

    @staticmethod
    def _hypothesis_emit(bs, emit_log: torch.Tensor) -> torch.Tensor:
        """the emit positions of the returned hypotheses [Bs, nbest, L] int32 (CPU): the finalised hypotheses ranked as
        simulst_beam_backtrack ranks them (descending fin_score, equal scores in finalisation order), each walked back from
        (fin_step, fin_row) through bp_parent; the row that computed step p of a hypothesis is the PARENT of its step-p entry"""
        n = bs.steps
        fin_step, fin_row, fin_score, fin_count = (x.cpu().tolist() for x in (bs.fin_step, bs.fin_row, bs.fin_score, bs.fin_count))
        parent, log = bs.bp_parent[:n].cpu().tolist(), emit_log[:n].cpu().tolist()
        out = [[[-1] * bs.L for _ in range(bs.nbest)] for _ in range(bs.Bs)]
        for s in range(bs.Bs):
            cnt = min(max(fin_count[s], 0), bs.beam)
            order = sorted(range(cnt), key=lambda k: (-fin_score[s][k], k))[:bs.nbest]
            for rank, k in enumerate(order):
                t, row = min(max(fin_step[s][k], 0), n - 1), min(max(fin_row[s][k], 0), bs.R - 1)
                e = out[s][rank]
                e[t] = log[t][row]
                for p in range(t - 1, -1, -1):
                    row = min(max(parent[p][row], 0), bs.R - 1)
                    e[p] = log[p][row]
        emit = torch.tensor(out, dtype=torch.int32).view(bs.Bs, bs.nbest, bs.L)
        return emit

    # ------------------------------------------------------------------ a whole target in one pass
    def features_teacher_forced(self, tokens: torch.Tensor) -> torch.Tensor:
        """the prediction network over every position of tokens [B, U1] (a decoder input: bos first, pads last) at once ->
        [B, U1, D]: the per-op kernels of features(), with simulst_decoder_self_attention_causal in place of the cached step"""
        ops, cfg, Wd = self.ops, self.cfg, self.w
        B, U1 = tokens.shape
        D, H = cfg.embed_dim, cfg.num_heads
        ensure_positions(Wd, U1 + cfg.padding_idx + 2)
        toks = tokens.to(device=self.device, dtype=torch.int64).contiguous().view(-1)
        pos_row = torch.arange(cfg.padding_idx + 1, cfg.padding_idx + 1 + U1, device=self.device, dtype=torch.int32).repeat(B)
        x = ops.embed_tokens(toks, Wd.E, Wd.pos, pos_row, self.embed_scale)              # [B * U1, D]

        def attend(qkv, l):
            return ops.decoder_self_attention_causal(qkv.view(B, U1, 3 * D), H=H).view(B * U1, D)

        for l, L in enumerate(Wd.layers):
            x = self_attention_block(ops, L, x, attend, l)
            x = feed_forward_block(ops, L, x)
        return ops.layernorm(x, Wd.ln_g, Wd.ln_b).view(B, U1, D)

    def lattice_inputs(self, prev_output_tokens: torch.Tensor):
        """the decoder input of :143-156: column 0 read as bos, a pad column appended, EOS scattered at each row's non-pad count ->
        (input [B, U1] int64 = [bos, y_1 .. y_{n-1}, eos, pad ..], labels [B, U1] int32 = input shifted left, tgt_len [B] int32 = n)"""
        cfg = self.cfg
        prev = prev_output_tokens.to(device=self.device, dtype=torch.int64).clone()
        B = prev.size(0)
        prev[:, 0] = BLANK
        inp = torch.cat([prev, prev.new_full((B, 1), cfg.padding_idx)], 1)
        tgt_len = inp.ne(cfg.padding_idx).sum(1, keepdim=True)
        inp.scatter_(1, tgt_len, cfg.eos)
        labels = torch.cat([inp[:, 1:], inp.new_full((B, 1), cfg.padding_idx)], 1).to(torch.int32).contiguous()
        return inp.contiguous(), labels, tgt_len.view(B).to(torch.int32).contiguous()

    def forward_lattice(self, prev_output_tokens: torch.Tensor, enc_btd: torch.Tensor, enc_len: torch.Tensor, *,
                        T: Optional[int] = None, return_logits: bool = False):
        """TransducerDecoder.forward (:124-163) WITHOUT an incremental state, reduced to what the RNN-T criterion reads:
        prev_output_tokens [B, U] = the target with its EOS moved to the front (pads behind), enc_btd [B, S_in, D], enc_len [B].
        Returns {"lp_blank", "lp_label": fp32 [B, S', U + 1] log-probabilities of the blank and of the row's next token in every
        cell s < src_len'[b], u <= tgt_len[b] (u < tgt_len[b] for the label; zero elsewhere), "src_len", "tgt_len": [B] int32,
        "padding_mask": the pooled padding mask [B, S'], "P" / "G": the joiner's fp32 source and target projections [B, S', D] /
        [B, U + 1, D]}.  The [B, S', U + 1, V] logits are not made (simulst_joiner_lattice);
        return_logits=True adds them as "logits" (fp32, no forced blank) from the tanh rows and simulst_linear -- for parity and
        baselines only, refused above lattice_logits_cap_bytes."""
        ops, V = self.ops, self.cfg.vocab
        B, _, D = enc_btd.shape
        inp, labels, tgt_len = self.lattice_inputs(prev_output_tokens)
        U1 = inp.size(1)
        pooled, src_len = self.downsample(enc_btd.to(device=self.device, dtype=self.dtype), enc_len, T)
        S = pooled.size(1)
        if return_logits and B * S * U1 * V * 4 > self.lattice_logits_cap_bytes:
            raise ValueError(f"forward_lattice(return_logits=True): the [B, S', U + 1, V] logits take {B * S * U1 * V * 4} bytes, "
                             f"above lattice_logits_cap_bytes = {self.lattice_logits_cap_bytes}")
        P = ops.linear(pooled.view(B * S, D), self.w.w_src, self.w.b_src, epilogue=EPI_BIAS_F32OUT).view(B, S, D)
        feats = self.features_teacher_forced(inp)
        G = ops.linear(feats.view(B * U1, D), self.w.w_tgt, None, epilogue=EPI_BIAS_F32OUT).view(B, U1, D)
        lp_blank, lp_label = ops.joiner_lattice(P, G, self.w.out_proj_fm, labels, src_len, tgt_len, V=V, blank=BLANK)
        out = {"lp_blank": lp_blank, "lp_label": lp_label, "src_len": src_len, "tgt_len": tgt_len, "P": P, "G": G,
               "padding_mask": torch.arange(S, device=self.device).unsqueeze(0) >= src_len.unsqueeze(1)}
        if return_logits:
            z = torch.tanh(P.unsqueeze(2) + G.unsqueeze(1)).to(self.dtype).view(B * S * U1, D)
            out["logits"] = ops.linear(z, self.w.out_proj, None, epilogue=EPI_BIAS_F32OUT).view(B, S, U1, V)
        return out

    # ------------------------------------------------------------------ the reference's call shape
    def forward(self, prev_output_tokens: torch.Tensor, encoder_out: Optional[Dict[str, List[torch.Tensor]]] = None,
                incremental_state: Optional[dict] = None, **unused):
        """TransducerDecoder.forward (:124-212) with an incremental state: prev_output_tokens [B, 1 + written] (its first column is
        read as bos), encoder_out["encoder_out"][0] [T, B, C] and its padding mask, incremental_state the CALLER's dict (it owns
        the state).  Returns (logits [B, 1, V] fp32, {"padding_mask": the pooled padding mask [B, S']}).  The written-token count
        is taken from prev_output_tokens: a call that repeats a prefix (a discarded prediction) restarts from the emit position
        that prefix had, no rollback call is needed."""
        if incremental_state is None:
            raise NotImplementedError("TransducerDecoder.forward without an incremental state returns the [B, S, T, V] lattice "
                                      "(models/transducer_model.py:148-156), which is never materialised here: use forward_lattice "
                                      "(log p(blank) / log p(label) per cell) or TransducerModel.score_reference")
        enc = encoder_out["encoder_out"][0]
        T, B = enc.shape[0], enc.shape[1]
        n_written = prev_output_tokens.size(1) - 1
        st = incremental_state.get(self.STATE_KEY)
        if st is None:
            st = self.new_state(B, cap=max(32, n_written + 8))
            incremental_state[self.STATE_KEY] = st
        if n_written + 2 > st.cap:
            st.grow(max(2 * st.cap, n_written + 8))
        if st.enc_rows != T:
            self.set_source(st, enc.to(device=self.device, dtype=self.dtype).transpose(0, 1).contiguous(),
                            source_lengths(encoder_out, B, T), T=T)
        if n_written > len(st.emit_before):
            raise ValueError(f"TransducerDecoder.forward: {n_written} tokens written but only {len(st.emit_before)} steps were taken")
        if n_written < len(st.emit_before):                      # a repeated prefix: back to where its last step started
            st.prev_emit.copy_(st.emit_before[n_written])
            del st.emit_before[n_written:]
        if st.n_prev_host != n_written:
            st.n_prev.fill_(n_written)
            st.n_prev_host = n_written
        st.emit_before.append(st.prev_emit.clone())
        logits = self.step(st, prev_output_tokens[:, -1])
        st.kv_rows = n_written + 1
        S = st.P.size(1)
        padding_mask = torch.arange(S, device=self.device).unsqueeze(0) >= st.src_len.unsqueeze(1)
        return logits.unsqueeze(1), {"padding_mask": padding_mask, "attn": [None], "inner_states": None}

    def reorder_incremental_state(self, incremental_state, new_order):
        """TransducerDecoder.reorder_incremental_state (:241-251): row r of the caller's state becomes row new_order[r] -- the
        prediction network's K/V prefix and prev_emit through simulst_transducer_beam_reorder (block = all rows: any new_order over
        the state's rows), the emit positions forward() keeps for repeated prefixes, and the source rows (the caller reorders its
        encoder output the same way).  A state that has taken no step has nothing to reorder.  new_order lives on the decoder's
        device, where fairseq's generator makes it: the reorder kernel reads it on the handle's stream, and as everywhere in this
        package nothing is copied from the host on the caller's behalf -- a host index is not implemented."""
        if not torch.is_tensor(new_order) or new_order.device.type != self.device.type:
            raise NotImplementedError("reorder_incremental_state with new_order on the host is not implemented: pass it on the "
                                      "decoder's device (the reorder kernel reads it on the handle's stream; no host copies are made)")
        st = None if incremental_state is None else incremental_state.get(self.STATE_KEY)
        if st is None:
            return
        R = st.B
        order = new_order.to(device=self.device, dtype=torch.int32).contiguous().view(-1)
        if order.numel() != R:
            raise ValueError(f"reorder_incremental_state: new_order holds {order.numel()} rows, the state {R} (the state's row count "
                             "is fixed; finished rows stay in the batch)")
        from .beam import ReorderBuffers
        buf = ReorderBuffers.of(st, extra=("prev_emit",))
        result = torch.zeros(1, device=self.device, dtype=torch.int32)
        self.ops.transducer_beam_reorder(buf.desc, buf.src, buf.dst, st.prev_emit, buf.other["prev_emit"], order, None, result,
                                         block=R, n_prev=min(st.kv_rows, st.cap))
        buf.swap()
        idx = order.long()
        st.emit_before = [e.index_select(0, idx) for e in st.emit_before]
        if st.P is not None and st.P.size(0) == R:
            st.P, st.pooled, st.src_len = st.P.index_select(0, idx), st.pooled.index_select(0, idx), st.src_len.index_select(0, idx)
        if int(result.item()) != 0:
            raise ValueError("reorder_incremental_state: new_order names a row outside the state")


class TransducerModel(FairseqModelSurface):
    """models/transducer_model.py:271-300: S2TEmformerModel's encoder with the TransducerDecoder.  An offline model:
    generate_offline (greedy, or beam search with beam / nbest / lenpen) and generate (beam search).  The attention-policy
    agents refuse it (model.refuse_offline_model); its own simultaneous agents are simulst_amd.transducer_agent.TransducerAgent
    and BatchedTransducerStreamingAgent, which write what generate_offline writes."""

    def __init__(self, cfg: ModelConfig, weights: Dict[str, torch.Tensor], device="cuda", dtype=torch.float32,
                 ops: Optional[Ops] = None):
        if cfg.model != "transducer_model":
            raise ValueError(f"TransducerModel builds config.transducer_model_s, not {cfg.model!r}")
        self.cfg = cfg
        self._deferred = None
        self.ops = ops or Ops()
        self.device, self.dtype = torch.device(device), dtype
        self.encoder = S2TEmformerEncoder(cfg, weights, device, dtype, self.ops)
        self.decoder = TransducerDecoder(cfg, weights, device, dtype, self.ops)

    @staticmethod
    def add_args(parser):
        """S2TEmformerModel.add_args + --downsample (:273-287)"""
        FairseqModelSurface.add_args(parser)
        parser.add_argument("--downsample", type=int)

    def generate_offline(self, src_tokens, src_lengths, n_steps=None, mask_eos=False, *, beam=1, lenpen=1.0, nbest=1):
        """the encoder once, then greedy transducer steps.  Returns tokens [B, n] and a dict with "emit" [B, n] (the pooled frame
        each token was emitted at), the encoder output and the state.  T = max(encoder_lengths) is read once per batch: the pooled
        states of a row depend on it (AvgPool1dTBCPad).  With beam > 1 (or nbest / lenpen away from their defaults): beam search,
        generate()'s hypothesis lists, n_steps (when given) the cap of every sentence."""
        if beam != 1 or nbest != 1 or lenpen != 1.0:
            assert not mask_eos, "mask_eos is a greedy-decode option"
            return self.generate(src_tokens, src_lengths, beam=beam, lenpen=lenpen, nbest=nbest, max_len=n_steps)
        enc = self.encoder.forward(src_tokens, src_lengths)
        if n_steps is None:
            n_steps = int(0.1 * src_tokens.size(1) + 10)
        T = int(enc["encoder_lengths"].max().item())
        toks, emit, st = self.decoder.greedy_offline(enc["encoder_out_btd"], enc["encoder_lengths"], n_steps, mask_eos, T=T)
        return toks, {"emit": emit, "encoder": enc, "state": st}

    def generate(self, src_tokens, src_lengths, *, beam=5, lenpen=1.0, nbest=1, max_len_a=0.1, max_len_b=10, max_len=None):
        """SimulSTModel.generate's surface (eval/generate.py --beam / --lenpen / --nbest) over the transducer: sentence s decodes at
        most max_len[s] = min(int(max_len_a T_s + max_len_b), max_target_positions - 1) tokens and EOS, T_s its own frame count
        (max_len: one cap for every sentence instead).  Returns per sentence a list of at most nbest {"tokens" (EOS included),
        "score", "positional_scores", "alignment": the pooled frame each token was emitted at (int32, one per token),
        "attention": None}, best first."""
        from .beam import hypotheses
        enc = self.encoder.forward(src_tokens, src_lengths)
        lens = [int(t) for t in torch.as_tensor(src_lengths).tolist()]
        a, b = (max_len_a, max_len_b) if max_len is None else (0, max_len)
        caps = [self.target_cap(t, a, b) for t in lens]
        T = int(enc["encoder_lengths"].max().item())
        toks, lengths, scores, pos, emit, _ = self.decoder.beam_offline(enc["encoder_out_btd"], enc["encoder_lengths"], caps, beam=beam,
                                                                        lenpen=lenpen, nbest=nbest, T=T)
        hyps = hypotheses(toks, lengths, scores, pos)
        emit, lengths = emit.cpu(), lengths.cpu()
        for s, sent in enumerate(hyps):
            for k, h in enumerate(sent):               # hypotheses() drops only empty trailing slots: index k is slot k
                h["alignment"] = emit[s, k, :int(lengths[s, k])].clone()
        return hyps

    def score_reference(self, src_tokens, src_lengths, targets, *, return_alignments=False):
        """Score given translations under the transducer (the forward value of criterion/rnnt_criterion.py:82-147): the encoder once,
        ONE pass of the prediction network and the joiner lattice over every target (TransducerDecoder.forward_lattice), then
        simulst_rnnt_forward.  targets: one EOS-terminated token list per sentence (n tokens, EOS counted).  Returns per sentence
        {"tokens", "score": ll / n, "nll": -ll with ll the log-likelihood summed over all monotonic alignments, "nll_offline":
        -sum_u lp_label[S_b - 1][u] (the criterion's offline-path term at label smoothing 0), "alignment", "positional_scores"};
        return_alignments fills the last two from the best single alignment: the pooled frame each token is emitted at [n] and the
        tokens' log-probabilities along it [n] (None otherwise)."""
        cfg = self.cfg
        targets = [[int(t) for t in tgt] for tgt in targets]
        B = len(targets)
        assert B == src_tokens.size(0) and all(len(t) >= 1 and t[-1] == cfg.eos for t in targets), "one EOS-terminated target per sentence"
        U = max(len(t) for t in targets)
        assert U + 1 <= cfg.max_target_positions, "target longer than max_target_positions"
        prev = torch.full((B, U), cfg.padding_idx, dtype=torch.int64)
        for b, t in enumerate(targets):
            prev[b, :len(t)] = torch.tensor([cfg.eos] + t[:-1])
        enc = self.encoder.forward(src_tokens, src_lengths)
        T = int(enc["encoder_lengths"].max().item())
        lat = self.decoder.forward_lattice(prev, enc["encoder_out_btd"], enc["encoder_lengths"], T=T)
        lp_blank, lp_label, src_len, tgt_len = lat["lp_blank"], lat["lp_label"], lat["src_len"], lat["tgt_len"]
        if return_alignments:
            ll, _, emit = self.ops.rnnt_forward(lp_blank, lp_label, src_len, tgt_len, want_best=True)
            pos = lp_label.gather(1, emit.clamp_min(0).long().unsqueeze(1)).squeeze(1).cpu()          # [B, U1]: lp_label[b, emit[u], u]
            emit = emit.cpu()
        else:
            ll = self.ops.rnnt_forward(lp_blank, lp_label, src_len, tgt_len)
        last = (src_len.long() - 1).clamp_min(0).view(B, 1, 1).expand(B, 1, lp_label.size(2))
        at_last = lp_label.gather(1, last).squeeze(1).cpu()                                          # [B, U1]: lp_label[b, S_b - 1, u]
        ll = ll.cpu()
        out = []
        for b, t in enumerate(targets):
            n = len(t)
            hyp = {"tokens": torch.tensor(t), "score": ll[b] / n, "nll": -ll[b], "nll_offline": -at_last[b, :n].sum(),
                   "alignment": None, "positional_scores": None}
            if return_alignments:
                hyp["alignment"] = emit[b, :n].clone()
                hyp["positional_scores"] = pos[b, :n].clone()
            out.append(hyp)
        return out


def transducer_model_s_arch(args):
    """models/transducer_model.py:303-310"""
    _default(args, "downsample", 8)
    _default(args, "activation_fn", "gelu")
    s2t_emformer_s(args)


def register():
    """add transducer_model / transducer_model_s to the registries (idempotent)"""
    from .registry import ARCH_REGISTRY, MODEL_REGISTRY, register_model, register_model_architecture
    if "transducer_model" not in MODEL_REGISTRY:
        register_model("transducer_model")(TransducerModel)
    if "transducer_model_s" not in ARCH_REGISTRY:
        register_model_architecture("transducer_model", "transducer_model_s")(transducer_model_s_arch)
