"""fp64 reference of the expected-alignment chain (test_hip_alignment_scans.py): utils/monotonic_attention.py:12-197 written from the
formulas as the headers of csrc/scans.hip restate them, in plain torch float64.  Vectorised over rows, sequential over targets, a DIRECT
cumulative product (no log space), `key_len` instead of a mask.  It does not call oracle/monotonic.py.  Gradients come from torch
autograd through `expected_alignment`.  Nothing here touches the device.

Every function takes a named `mutation`: one line of the reference changed into a bug a kernel could have.  The tests use them to
prove that their inputs can see that class of bug."""
import torch

CHUNK = 64          # positions a wavefront scans before it carries a prefix

MUTATIONS_ALIGNMENT = ("drop_sum_carry", "drop_prod_carry", "no_lead", "no_lower_clamp")
MUTATIONS_SOFT = ("keylen_of_row", "soft_drop_fwd_carry", "soft_drop_rev_carry", "chunk_window_off_by_one")
MUTATIONS_MASS = ("keylen_of_row",)


def _chunked(scan, x):
    """`scan` (torch.cumsum / torch.cumprod) over the last dim, restarted at every CHUNK positions: a dropped carry"""
    return torch.cat([scan(c, dim=-1) for c in x.split(CHUNK, dim=-1)], dim=-1)


def _valid(key_len, n_rows, S, rows_per_len=1, mutation=None):
    """[n_rows, S] bool: position < key_len of the row's utterance (row r belongs to key_len[r // rows_per_len])"""
    if key_len is None:
        return torch.ones(n_rows, S, dtype=torch.bool)
    kl = key_len.detach().cpu().to(torch.int64).view(-1)
    r = torch.arange(n_rows)
    idx = r // rows_per_len
    if mutation == "keylen_of_row":
        idx = r.clamp(max=kl.numel() - 1)
    return torch.arange(S).view(1, S) < kl[idx].view(-1, 1)


def expected_alignment(p, key_len=None, eps=1e-6, mutation=None, aux=False):
    """p [BH, U, S], key_len [BH] or None -> alpha [BH, U, S] fp64.
      c_i   = exclusive cumprod over the source of (1 - p_i + eps), with a prepended (1 + eps)
      alpha_i = clamp(p_i c_i cumsum(alpha_{i-1} / clamp(c_i, eps, 1)), 0, 1),   alpha_{-1} = one-hot(0)
    p counts as 0 at positions >= key_len.  aux=True also returns (c, u), u the value before the last clamp."""
    assert mutation is None or mutation in MUTATIONS_ALIGNMENT, mutation
    BH, U, S = p.shape
    p = p.double()
    p = torch.where(_valid(key_len, BH, S).unsqueeze(1), p, torch.zeros((), dtype=torch.float64))
    x = 1.0 - p + eps
    incl = _chunked(torch.cumprod, x) if mutation == "drop_prod_carry" else torch.cumprod(x, dim=-1)
    excl = torch.cat([torch.ones(BH, U, 1, dtype=torch.float64), incl[..., :-1]], dim=-1)
    if mutation == "drop_prod_carry":
        excl = torch.where((torch.arange(S) % CHUNK == 0).view(1, 1, S), torch.ones((), dtype=torch.float64), excl)
    lead = 1.0 if mutation == "no_lead" else 1.0 + eps
    c = lead * excl
    cc = c.clamp(max=1.0) if mutation == "no_lower_clamp" else c.clamp(eps, 1.0)
    prev = torch.zeros(BH, S, dtype=torch.float64)
    prev[:, 0] = 1.0
    rows, us = [], []
    for i in range(U):
        r = prev / cc[:, i]
        R = _chunked(torch.cumsum, r) if mutation == "drop_sum_carry" else torch.cumsum(r, dim=-1)
        u = p[:, i] * c[:, i] * R
        prev = u.clamp(0.0, 1.0)
        rows.append(prev)
        us.append(u)
    alpha = torch.stack(rows, dim=1) if U else p.new_zeros(BH, 0, S)
    if aux:
        return alpha, c, (torch.stack(us, dim=1) if U else alpha)
    return alpha


def alignment_grad(p, key_len, eps, upstream, mutation=None):
    """d sum(alpha * upstream) / d p by autograd through the fp64 reference -> (grad [BH, U, S] fp64, alpha, c, u)"""
    pr = p.detach().double().clone().requires_grad_(True)
    alpha, c, u = expected_alignment(pr, key_len, eps, mutation=mutation, aux=True)
    (alpha * upstream.double()).sum().backward()
    return pr.grad, alpha.detach(), c.detach(), u.detach()


def mass_preservation(alpha, key_len=None, mutation=None):
    """alpha [BH, U, S] -> fp64 copy whose last valid position takes the residual 1 - clamp(sum, 0, 1).  Without key_len the last
    position is REPLACED by the residual of the others; with it, positions >= key_len become 0 and the residual is ADDED."""
    assert mutation is None or mutation in MUTATIONS_MASS, mutation
    BH, U, S = alpha.shape
    a = alpha.detach().cpu().double().clone()
    if key_len is None:
        a[..., -1] = 1.0 - a[..., :-1].sum(-1).clamp(0.0, 1.0)
        return a
    valid = _valid(key_len, BH * U, S, U, mutation).view(BH, U, S)
    a = torch.where(valid, a, torch.zeros((), dtype=torch.float64))
    last = valid.sum(-1, keepdim=True) - 1
    return a.scatter_add(2, last, 1.0 - a.sum(-1, keepdim=True).clamp(0.0, 1.0))


def _window_sum(x, back, fwd):
    """out[j] = sum of x[j - back .. j + fwd], zero outside: one shifted add per offset (no difference of prefix sums, whose
    cancellation would cost the small windows their digits)"""
    S = x.size(-1)
    out = torch.zeros_like(x)
    for o in range(-min(back, S - 1), min(fwd, S - 1) + 1):
        if o <= 0:
            out[..., -o:] += x[..., :S + o]
        else:
            out[..., :S - o] += x[..., o:]
    return out


def expected_soft_attention(alpha, energy, key_len=None, chunk=None, eps=1e-10, mutation=None):
    """alpha, energy [BH, U, S] -> beta fp64.  ex = exp(e - max e) + eps with e = -1e8 at positions >= key_len (alpha = 0 there);
      infinite lookback: beta_j = ex_j sum_{k >= j} alpha_k / (eps + sum_{m <= k} ex_m)
      chunkwise:         beta_j = ex_j sum_{k = j .. j+chunk-1} alpha_k / (eps + sum_{m = k-chunk+1 .. k} ex_m)
    beta is 0 at positions >= key_len and clamped to [0, 1]."""
    assert mutation is None or mutation in MUTATIONS_SOFT, mutation
    BH, U, S = alpha.shape
    valid = _valid(key_len, BH * U, S, U, mutation).view(BH, U, S)
    a = torch.where(valid, alpha.detach().cpu().double(), torch.zeros((), dtype=torch.float64))
    e = torch.where(valid, energy.detach().cpu().double(), torch.full((), -1e8, dtype=torch.float64))
    ex = torch.exp(e - e.max(dim=-1, keepdim=True).values) + eps
    if chunk:
        d = _window_sum(ex, chunk if mutation == "chunk_window_off_by_one" else chunk - 1, 0)
        beta = ex * _window_sum(a / (eps + d), 0, chunk - 1)
    else:
        cs = _chunked(torch.cumsum, ex) if mutation == "soft_drop_fwd_carry" else torch.cumsum(ex, dim=-1)
        inner = (a / (eps + cs)).flip(-1)          # the reverse cumsum walks 64-wide chunks from the END of the source
        rs = _chunked(torch.cumsum, inner) if mutation == "soft_drop_rev_carry" else torch.cumsum(inner, dim=-1)
        beta = ex * rs.flip(-1)
    return torch.where(valid, beta, torch.zeros((), dtype=torch.float64)).clamp(0.0, 1.0)
