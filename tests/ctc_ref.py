"""fp64 references of the CTC-head tests (test_hip_ctc_pick.py, test_hip_ctc_decode.py, test_ctc_report.py): the row pick of
SIMULST_EPI_ROW_PICK computed from the SAME rounded operands the kernel reads, the clear / unclear rule that compares a pick with it,
and the collapse as a plain Python loop.  Nothing here touches the device."""
import torch


def logits64(x, W, bias=None):
    """x [M, K], W [N, K] (already rounded to the operand dtype), bias fp32 [N] or None -> z [M, N] fp64"""
    z = x.detach().cpu().double() @ W.detach().cpu().double().t()
    return z if bias is None else z + bias.detach().cpu().double()


def pick64(z):
    """z [M, N] fp64 -> (pick: lowest column of the maximum, zmax, lse, margin: top-1 minus top-2, inf for N == 1)"""
    zmax, pick = z.max(dim=1)
    pick = (z == zmax.unsqueeze(1)).to(torch.int64).argmax(dim=1)          # the LOWEST maximal column
    lse = torch.logsumexp(z, dim=1)
    if z.size(1) > 1:
        top2 = z.topk(2, dim=1).values
        margin = top2[:, 0] - top2[:, 1]
    else:
        margin = torch.full_like(zmax, float("inf"))
    return pick, zmax, lse, margin


def check_pick(z, pick, e, what=""):
    """The pick rule of the issue: a row is UNCLEAR if its fp64 top-2 margin is <= 2e; there the pick must be a column within 2e of the
    maximum, everywhere else it must be the fp64 pick exactly.  -> boolean mask of the unclear rows."""
    ref, zmax, _, margin = pick64(z)
    pick = pick.detach().cpu().to(torch.int64).view(-1)
    assert pick.numel() == z.size(0) and int(pick.min()) >= 0 and int(pick.max()) < z.size(1), f"{what}: pick out of range"
    unclear = margin <= 2 * e
    wrong = (~unclear) & (pick != ref)
    assert not bool(wrong.any()), f"{what}: {int(wrong.sum())} clear rows differ from fp64, first row {int(wrong.nonzero()[0])}"
    got = z.gather(1, pick.unsqueeze(1)).squeeze(1)
    far = unclear & (got < zmax - 2 * e)
    assert not bool(far.any()), f"{what}: {int(far.sum())} unclear rows picked a column more than 2e below the maximum"
    return unclear


def collapse_loop(path, length, blank):
    """one row: -> (tokens, frames) by the textbook loop"""
    toks, frames, prev = [], [], None
    for t in range(min(int(length), len(path))):
        p = int(path[t])
        if p != blank and (t == 0 or p != prev):
            toks.append(p)
            frames.append(t)
        prev = p
    return toks, frames
