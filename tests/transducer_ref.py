"""fp64 restatement, in plain torch on the CPU, of the transducer's inference path (models/transducer_model.py:28-212):

* ``pool``            AvgPool1dTBCPad (:79-98): y[b, j] = (sum of the valid rows of window j) / n_j with n_j the window clipped to the
                      batch's T, times k / r at a shorter row's last window
* ``TransducerRef``   the prediction network (fairseq's pre-norm TransformerDecoder with no_encoder_attn: self-attention + GELU
                      feed-forward, sinusoidal positions, embed_scale, a final LayerNorm, fed [bos] + hypothesis, :101-122,158-162)
                      and the joiner step (:60-76,163-209)
* ``joiner_logits`` / ``emit_decisions``  the joiner alone, from P, g and W_out: what the scan and emit kernels are held to

Weights are a ``{name: tensor}`` dict under the reference's state-dict names (``decoder.*``).
"""
import math

import torch

F64 = torch.float64
BLANK = 0
BLANK_AT_EOS = -1e4


def pool(x_btd, lens, k, T=None):
    """x [B, S_in, D], lens [B] -> (y [B, ceil(T / k), D] fp64, new lengths [B] int64); T defaults to max(lens)"""
    x = x_btd.to(F64)
    lens = torch.as_tensor(lens).to(torch.int64)
    B, _, D = x.shape
    T = int(lens.max()) if T is None else int(T)
    S = (T + k - 1) // k
    y = torch.zeros(B, S, D, dtype=F64)
    for b in range(B):
        n = int(lens[b])
        for j in range((n + k - 1) // k):
            t0, t1 = j * k, min(j * k + k, T)
            y[b, j] = x[b, t0:min(t1, n)].sum(0) / (t1 - t0)
        if 0 < n < T:
            r = (n - 1) % k + 1
            y[b, (n - 1) // k] *= k / r
    return y, (lens + k - 1) // k


def sinusoidal(n, dim, padding_idx):
    half = dim // 2
    freq = torch.exp(torch.arange(half, dtype=F64) * -(math.log(10000) / (half - 1)))
    ang = torch.arange(n, dtype=F64).unsqueeze(1) * freq.unsqueeze(0)
    tab = torch.cat([torch.sin(ang), torch.cos(ang)], 1)
    if dim % 2 == 1:
        tab = torch.cat([tab, torch.zeros(n, 1, dtype=F64)], 1)
    tab[padding_idx] = 0
    return tab


def layer_norm(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def joiner_logits(P, g, W, round_z=None):
    """P [B, S, D], g [B, D], W [V, D] -> logits [B, S, V] fp64 of W tanh(P + g); round_z: a dtype the tanh is rounded to first"""
    z = torch.tanh(P.to(F64) + g.to(F64).unsqueeze(1))
    if round_z is not None:
        z = z.to(round_z).to(F64)
    return z @ W.to(F64).t()


def emit_decisions(logits, prev_emit, src_len):
    """logits [B, S, V] fp64 -> per row (new_emit, returned row [V], margins): the scan of :170-200.  margins: for every scanned
    position up to the emit |blank - best non-blank| (blank = -1e4 at src_len - 1)."""
    B, S, V = logits.shape
    new_emit, rows, margins = [], [], []
    for b in range(B):
        n = int(src_len[b])
        pe = min(max(int(prev_emit[b]), 0), n - 1)
        ne, m = n - 1, []
        for s in range(pe, n):
            row = logits[b, s].clone()
            if s == n - 1:
                row[BLANK] = BLANK_AT_EOS
            nb = torch.cat([row[:BLANK], row[BLANK + 1:]]).max()
            m.append(float((nb - row[BLANK]).abs()))
            if nb > row[BLANK]:
                ne = s
                break
        row = logits[b, ne].clone()
        if ne == n - 1:
            row[BLANK] = BLANK_AT_EOS
        new_emit.append(ne)
        rows.append(row)
        margins.append(m)
    return torch.tensor(new_emit), torch.stack(rows), margins


def greedy_pick(row, pad, eos, mask_eos):
    lp = row.clone()
    lp[pad] = -float("inf")
    if mask_eos:
        lp[eos] = -float("inf")
    return int(lp.argmax())


def top2_margin(row, pad, eos, mask_eos):
    lp = row.clone()
    lp[pad] = -float("inf")
    if mask_eos:
        lp[eos] = -float("inf")
    t = lp.topk(2).values
    return float(t[0] - t[1])


class TransducerRef:
    def __init__(self, weights, *, heads, downsample, pad=1, eos=2, no_scale_embedding=False, round_to=None):
        """round_to: a dtype the weights are rounded to first (the fp64 reference of a bf16 model runs on the bf16 weights)"""
        self.w = {k: (v.to(round_to) if round_to is not None else v).to(F64) for k, v in weights.items() if k.startswith("decoder.")}
        self.H, self.k, self.pad, self.eos = heads, downsample, pad, eos
        self.D = self.w["decoder.embed_tokens.weight"].shape[1]
        self.V = self.w["decoder.output_projection.weight"].shape[0]
        self.scale = 1.0 if no_scale_embedding else math.sqrt(self.D)
        self.n_layers = 1 + max(int(k.split(".")[2]) for k in self.w if k.startswith("decoder.layers."))
        self.pos = sinusoidal(1024 + pad + 2, self.D, pad)

    def set_source(self, enc_btd, enc_len, T=None):
        self.pooled, self.src_len = pool(enc_btd, enc_len, self.k, T)
        w = self.w
        self.P = self.pooled @ w["decoder.joiner.source_projection.weight"].t() + w["decoder.joiner.source_projection.bias"]
        self.prev_emit = torch.zeros(enc_btd.shape[0], dtype=torch.int64)

    def features(self, hyp):
        """hyp [B, n] written tokens -> features of the newest position of [bos] + hyp, [B, D]"""
        w, H = self.w, self.H
        B = hyp.shape[0]
        toks = torch.cat([torch.full((B, 1), BLANK, dtype=torch.int64), hyp.to(torch.int64)], 1)
        U, D = toks.shape[1], self.D
        d = D // H
        x = self.scale * w["decoder.embed_tokens.weight"][toks] + self.pos[self.pad + 1:self.pad + 1 + U].unsqueeze(0)
        causal = torch.triu(torch.full((U, U), -float("inf"), dtype=F64), 1)
        for l in range(self.n_layers):
            p = f"decoder.layers.{l}"
            y = layer_norm(x, w[p + ".self_attn_layer_norm.weight"], w[p + ".self_attn_layer_norm.bias"])
            q, k, v = (y @ w[f"{p}.self_attn.{n}_proj.weight"].t() + w[f"{p}.self_attn.{n}_proj.bias"] for n in "qkv")
            q = (q * d ** -0.5).view(B, U, H, d).transpose(1, 2)
            k, v = k.view(B, U, H, d).transpose(1, 2), v.view(B, U, H, d).transpose(1, 2)
            a = torch.softmax(q @ k.transpose(-1, -2) + causal, -1) @ v
            a = a.transpose(1, 2).reshape(B, U, D)
            x = x + a @ w[p + ".self_attn.out_proj.weight"].t() + w[p + ".self_attn.out_proj.bias"]
            y = layer_norm(x, w[p + ".final_layer_norm.weight"], w[p + ".final_layer_norm.bias"])
            h = gelu(y @ w[p + ".fc1.weight"].t() + w[p + ".fc1.bias"])
            x = x + h @ w[p + ".fc2.weight"].t() + w[p + ".fc2.bias"]
        x = layer_norm(x, w["decoder.layer_norm.weight"], w["decoder.layer_norm.bias"])
        return x[:, -1]

    def step(self, hyp):
        """one joiner step after the written tokens hyp [B, n] -> (row logits [B, V], new_emit [B], margins per row)"""
        g = self.features(hyp) @ self.w["decoder.joiner.target_projection.weight"].t()
        logits = joiner_logits(self.P, g, self.w["decoder.output_projection.weight"])
        new_emit, rows, margins = emit_decisions(logits, self.prev_emit, self.src_len)
        self.prev_emit = new_emit
        return rows, new_emit, margins

    def run_forced(self, forced):
        """teacher-forced steps over forced [B, n] -> (step_logits [n, B, V], step_emit [n, B], margins [n][B])"""
        out, emits, ms = [], [], []
        for t in range(forced.shape[1]):
            rows, ne, m = self.step(forced[:, :t])
            out.append(rows), emits.append(ne), ms.append(m)
        return torch.stack(out), torch.stack(emits), ms

    def run_greedy(self, n, mask_eos=False):
        """-> (tokens [B, n], emit [B, n], min margin per (step, row): scan decisions and top-1 against top-2 of the row)"""
        B = self.P.shape[0]
        hyp = torch.zeros(B, 0, dtype=torch.int64)
        emits, margins = [], []
        for t in range(n):
            rows, ne, m = self.step(hyp)
            me = mask_eos or t == 0
            tok = torch.tensor([greedy_pick(rows[b], self.pad, self.eos, me) for b in range(B)])
            margins.append([min(m[b] + [top2_margin(rows[b], self.pad, self.eos, me)]) for b in range(B)])
            hyp = torch.cat([hyp, tok.unsqueeze(1)], 1)
            emits.append(ne)
        return hyp, torch.stack(emits, 1), torch.tensor(margins)
