"""Float64 references of the front-end kernels (csrc/fbank.hip, conv_pos_mfma.hip, rowops.hip), each written from the operation's
definition in numpy, with no GPU and no index arithmetic taken from a kernel.  tests/test_hip_front_end.py holds the kernels to them,
tests/test_front_end_ref_cpu.py ties them to the oracle and shows, with the `mut` argument every reference takes, that the cases of
the GPU file can fail.  `mut` names ONE deliberate mistake (the table MUTATIONS); None is the reference.
"""
import math

import numpy as np

WIN, SHIFT, NFFT, SAMPLE_RATE = 400, 160, 512, 16000
EPS32 = float(np.float32(1.1920928955078125e-07))
MUTATIONS = {
    "fbank": ("twiddle_sign", "preemph0_zero", "window_off1", "mel_lo_off1"),
    "conv": ("window_shift1", "hist_reversed", "t_le_len", "w_co_swapped"),
    "layernorm": ("var_dm1",),
    "prenorm": ("sum_div_S", "cnt_no_max"),
    "pack": ("src_seg_S", "no_last_zero"),
    "argmax": ("tie_highest",),
}


# ---- fbank ----------------------------------------------------------------------------------------------------------------------------
def povey_window64():
    i = np.arange(WIN, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / (WIN - 1))) ** 0.85


def mel_weights64(n_mel, low=20.0):
    """[n_mel, 257] triangles on the mel scale 1127 ln(1 + f / 700) between `low` Hz and Nyquist, evaluated at the centres of FFT
    bins 0..255; the Nyquist bin has weight 0"""
    mel = lambda f: 1127.0 * math.log(1.0 + f / 700.0)
    m_lo, m_hi = mel(low), mel(0.5 * SAMPLE_RATE)
    step = (m_hi - m_lo) / (n_mel + 1)
    Wm = np.zeros((n_mel, NFFT // 2 + 1))
    for m in range(n_mel):
        left, centre, right = m_lo + m * step, m_lo + (m + 1) * step, m_lo + (m + 2) * step
        for j in range(NFFT // 2):
            mj = mel(j * SAMPLE_RATE / NFFT)
            Wm[m, j] = max(0.0, min((mj - left) / (centre - left), (right - mj) / (right - centre)))
    return Wm


def dft_matrix64():
    """[257, 400] complex: exp(-2 pi i j n / 512)"""
    j = np.arange(NFFT // 2 + 1, dtype=np.float64)[:, None]
    n = np.arange(WIN, dtype=np.float64)[None, :]
    ang = -2.0 * np.pi * ((j * n) % NFFT) / NFFT
    return np.cos(ang) + 1j * np.sin(ang)


def _fft_wrong_last_stage(y):
    """a float64 radix-2 FFT of the zero-padded frame whose LAST stage uses exp(+i ...) (the `twiddle_sign` mistake).  Flipping
    every stage would give the conjugate spectrum and the same power; one stage does not."""
    def rec(v, top):
        n = v.size
        if n == 1:
            return v.astype(np.complex128)
        ev, od = rec(v[0::2], False), rec(v[1::2], False)
        sign = 1.0 if top else -1.0
        tw = np.exp(sign * 2j * np.pi * np.arange(n // 2) / n)
        return np.concatenate([ev + tw * od, ev - tw * od])
    return rec(np.concatenate([y, np.zeros(NFFT - WIN)]), True)[:NFFT // 2 + 1]


_TABLES = {}


def _tables(n_mel):
    if "dft" not in _TABLES:
        _TABLES["dft"], _TABLES["win"] = dft_matrix64(), povey_window64()
    if n_mel not in _TABLES:
        _TABLES[n_mel] = mel_weights64(n_mel)
    return _TABLES["dft"], _TABLES["win"], _TABLES[n_mel]


def ref_fbank(wave, n_mel, preemph, mut=None):
    """wave [n] float64.  Returns e [F, n_mel] mel energies before floor and log, a [F, n_mel] = sum_j w_mj sqrt(P_j), ynorm [F] the
    windowed frame's 2-norm, wsum [n_mel] = sum_j w_mj."""
    wave = np.asarray(wave, dtype=np.float64)
    n = wave.size
    F = 1 + (n - WIN) // SHIFT if n >= WIN else 0
    dft, win, Wm = _tables(n_mel)
    if mut == "window_off1":
        win = np.concatenate([win[1:], win[-1:]])
    if mut == "mel_lo_off1":
        Wm = np.concatenate([Wm[:, 1:], np.zeros((n_mel, 1))], axis=1)      # the triangle laid one bin too far up
    e, a, yn = np.zeros((F, n_mel)), np.zeros((F, n_mel)), np.zeros(F)
    for f in range(F):
        fr = wave[f * SHIFT:f * SHIFT + WIN]
        fr = fr - fr.sum() / WIN
        prev = np.concatenate([[0.0 if mut == "preemph0_zero" else fr[0]], fr[:-1]])
        y = (fr - preemph * prev) * win
        spec = _fft_wrong_last_stage(y) if mut == "twiddle_sign" else dft @ y
        P = spec.real ** 2 + spec.imag ** 2
        e[f], a[f], yn[f] = Wm @ P, Wm @ np.sqrt(P), math.sqrt(float((y * y).sum()))
    return dict(e=e, a=a, ynorm=yn, wsum=Wm.sum(axis=1))


# ---- conv-pos -------------------------------------------------------------------------------------------------------------------------
_erf = np.frompyfunc(math.erf, 1, 1)                         # math.erf(nan) is nan


def gelu64(v):
    v = np.asarray(v, dtype=np.float64)
    return 0.5 * v * (1.0 + _erf(v / math.sqrt(2.0)).astype(np.float64))


def ref_conv_pos(x, hist, W, bias, lengths, groups, mut=None):
    """x [B, T, D], hist [B, k - 1, D] or None, W [D, cpg, k], bias [D], lengths [B] or None, all float64 (x may hold NaN at
    t >= len).  y = x + gelu_erf(bias + sum_{tau < k, c < cpg} W[g cpg + o][c][tau] * xx[t - (k - 1) + tau][g cpg + c]) with xx = hist
    (or zeros) in front of x; exact 0 at t >= len.  Returns y, pre (the pre-activation) and mag = sum |w||x|, each [B, T, D]; rows at
    t >= len hold 0 in all three."""
    B, T, D = x.shape
    cpg, k = W.shape[1], W.shape[2]
    assert D == groups * cpg
    if mut == "w_co_swapped":
        W = W.reshape(groups, cpg, cpg, k).transpose(0, 2, 1, 3).reshape(D, cpg, k)
    front = np.zeros((B, k - 1, D)) if hist is None else np.asarray(hist, dtype=np.float64)
    if mut == "hist_reversed":
        front = front[:, ::-1]
    xx = np.concatenate([front, x], axis=1)                                  # output frame t sees rows t .. t + k - 1 of xx
    if mut == "window_shift1":
        xx = np.concatenate([np.zeros((B, 1, D)), xx[:, :-1]], axis=1)
    y, pre, mag = np.zeros((B, T, D)), np.zeros((B, T, D)), np.zeros((B, T, D))
    with np.errstate(all="ignore"):
        for g in range(groups):
            sl = slice(g * cpg, (g + 1) * cpg)
            wins = np.lib.stride_tricks.sliding_window_view(xx[:, :, sl], k, axis=1)      # [B, T, c, tau]
            flat = wins.reshape(B * T, cpg * k)                                # row (b, t): every (c, tau) of its window
            w_g = W[sl].reshape(cpg, cpg * k).T                                # [(c, tau), o]
            pre[:, :, sl] = (flat @ w_g).reshape(B, T, cpg)
            mag[:, :, sl] = (np.abs(flat) @ np.abs(w_g)).reshape(B, T, cpg)
        pre += bias
        for b in range(B):
            L = T if lengths is None else int(lengths[b])
            n_t = min(T, L + 1) if mut == "t_le_len" else min(T, L)
            y[b, :n_t] = x[b, :n_t] + gelu64(pre[b, :n_t])
            pre[b, n_t:] = 0.0
            mag[b, n_t:] = 0.0
    return y, pre, mag


# ---- LayerNorm, pre-norm with summaries, segment means ----------------------------------------------------------------------------------
def ref_layernorm(x, gamma, beta, eps=1e-5, mut=None):
    """x [..., D] float64 -> y = z * gamma + beta and z = (x - mean) / sqrt(var + eps), var the mean squared deviation"""
    D = x.shape[-1]
    mu = x.sum(axis=-1, keepdims=True) / D
    d = x - mu
    var = (d * d).sum(axis=-1, keepdims=True) / (D - 1 if mut == "var_dm1" else D)
    z = d / np.sqrt(var + eps)
    return z * gamma + beta, z


def _seg_counts(T, S, L, mut=None):
    """[(t0, count)] per segment: the summary is the mean over the first min(t1, max(L, t0 + 1)) - t0 rows"""
    out = []
    for t0 in range(0, T, S):
        t1 = min(t0 + S, T)
        cnt = min(t1, L if mut == "cnt_no_max" else max(L, t0 + 1)) - t0
        out.append((t0, cnt))
    return out


def ref_prenorm(X, gamma, beta, lengths, T, n_rc, S, mut=None):
    """X [B, n_rc + T, D] float64.  Returns ln [B, n_rc + T, D] (the LayerNorm rows), z (before gamma / beta), summ [B, N, D] (the mean
    of the UNROUNDED LayerNorm rows of each segment's counted rows), cnt [B, N] and mabs [B, N, D] = the mean |ln| over the same
    rows.  With NaN rows at t >= len the summaries of segments with t0 >= len are NaN: nobody reads them."""
    B, D = X.shape[0], X.shape[2]
    with np.errstate(all="ignore"):
        ln, z = ref_layernorm(X, gamma, beta)
    N = -(-T // S)
    summ, mabs, cnt = np.zeros((B, N, D)), np.zeros((B, N, D)), np.zeros((B, N), dtype=np.int64)
    for b in range(B):
        L = T if lengths is None else int(lengths[b])
        for i, (t0, c) in enumerate(_seg_counts(T, S, L, mut)):
            rows = ln[b, n_rc + t0:n_rc + t0 + max(c, 0)]
            div = S if mut == "sum_div_S" else c
            with np.errstate(all="ignore"):
                summ[b, i] = rows.sum(axis=0) / div if div != 0 else np.nan
                mabs[b, i] = np.abs(rows).sum(axis=0) / max(c, 1)
            cnt[b, i] = c
    return ln, z, summ, cnt, mabs


def ref_segment_mean(X, lengths, S, n_out):
    """X [B, T, D] float64 -> out [B, n_out, D], cnt [B, n_out], mabs [B, n_out, D]"""
    B, T, D = X.shape
    out, mabs, cnt = np.zeros((B, n_out, D)), np.zeros((B, n_out, D)), np.zeros((B, n_out), dtype=np.int64)
    for b in range(B):
        L = T if lengths is None else int(lengths[b])
        for i, (t0, c) in enumerate(_seg_counts(T, S, L)[:n_out]):
            with np.errstate(all="ignore"):
                out[b, i] = X[b, t0:t0 + c].sum(axis=0) / c
                mabs[b, i] = np.abs(X[b, t0:t0 + c]).sum(axis=0) / c
            cnt[b, i] = c
    return out, cnt, mabs


# ---- copies and picks -----------------------------------------------------------------------------------------------------------------
def ref_pack_rows(x, S, R, N, mut=None):
    """x [B, T, D] -> [B, N R + T, D]: right-context row r of segment i is utterance frame (i + 1) S + r, zero for the last segment
    and at or beyond T; then the T utterance rows"""
    B, T, D = x.shape
    out = np.zeros((B, N * R + T, D), dtype=x.dtype)
    for b in range(B):
        for i in range(N):
            for r in range(R):
                src = (i * S + r) if mut == "src_seg_S" else ((i + 1) * S + r)
                last = i == N - 1 and mut != "no_last_zero"
                if not last and src < T:
                    out[b, i * R + r] = x[b, src]
        for t in range(T):
            out[b, N * R + t] = x[b, t]
    return out


def ref_embed(tokens, E, pos, pos_row, scale):
    """scale * E[token] + pos[pos_row], float64; mag = |scale * e| + |pos|"""
    B, D = len(tokens), E.shape[1]
    val, mag = np.zeros((B, D)), np.zeros((B, D))
    for b in range(B):
        se, p = scale * E[int(tokens[b])], pos[int(pos_row[b])]
        val[b], mag[b] = se + p, np.abs(se) + np.abs(p)
    return val, mag


def ref_argmax(logits, pad_idx, eos_idx, mask_eos, eos_bias=None, mut=None):
    """logits [B, V] float64.  eos_bias[b] is added to the EOS column, pad and (with mask_eos) EOS count as -inf, the lowest index
    wins a tie, an all -inf row gives 0"""
    B, V = logits.shape
    out = np.zeros(B, dtype=np.int64)
    for b in range(B):
        best, bi = -math.inf, 0
        for c in range(V):
            v = float(logits[b, c])
            if c == eos_idx and eos_bias is not None:
                v += float(eos_bias[b])
            if c == pad_idx or (mask_eos and c == eos_idx):
                v = -math.inf
            if v > best or (mut == "tie_highest" and v == best and v > -math.inf):
                best, bi = v, c
        out[b] = bi
    return out
