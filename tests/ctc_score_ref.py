"""fp64 reference pieces of the CTC scoring tests (test_hip_ctc_nll.py, test_hip_ctc_score.py): the textbook forward recursion with
the size of its alphas, and the error bound of an fp32 run of it.  Nothing here touches the device."""
import torch


def alpha64(lp, tg, blank):
    """lp [S, V] fp64 log-probabilities, tg list of labels -> (nll, largest finite |alpha|) of the CTC forward recursion"""
    ext = [blank]
    for t in tg:
        ext += [int(t), blank]
    ext = torch.tensor(ext)
    n = ext.numel()
    skip = torch.zeros(n, dtype=torch.bool)
    skip[2:] = ext[2:] != ext[:-2]
    ninf = torch.tensor(float("-inf"), dtype=torch.float64)
    a = torch.full((n,), float("-inf"), dtype=torch.float64)
    a[0] = lp[0, blank]
    if n > 1:
        a[1] = lp[0, ext[1]]
    big = float(a[torch.isfinite(a)].abs().max())
    for t in range(1, lp.size(0)):
        p1 = torch.cat([ninf.view(1), a[:-1]])
        p2 = torch.where(skip, torch.cat([ninf.expand(2), a[:-2]])[:n], ninf)
        a = torch.logsumexp(torch.stack([a, p1, p2]), 0) + lp[t, ext]
        fin = a[torch.isfinite(a)]
        if fin.numel():
            big = max(big, float(fin.abs().max()))
    return -float(torch.logsumexp(a[-2:] if n > 1 else a[-1:], 0)), big


def nll_bound(S, max_alpha):
    """|nll - ref| of an fp32 recursion over S frames: one rounding of the sum and one of the log-add per frame (the form of
    tests/rnnt_ref.ll_bound)"""
    return (S + 1) * 2.0 ** -22 * max(1.0, max_alpha)
