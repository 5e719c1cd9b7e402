"""Reference for the batched edit distance (csrc/edit_distance.hip, simulst_amd/edit_distance.py): the plain dynamic program with the
tie rule of include/simulst_hip.h spelled out, a back-trace, and the counts carried forward with the minimum.

D[i][j] is the distance of the first i reference labels and the first j hypothesis labels.  Among the predecessors that attain the
minimum a cell takes, in this order: the diagonal (a match if the labels are equal, else a substitution), a deletion (D[i-1][j] + 1:
reference label i has no counterpart), an insertion (D[i][j-1] + 1).  Operation codes: 0 match, 1 substitution, 2 deletion, 3 insertion.

`align_plain` is the specification, cell by cell in Python.  `align` is the same recurrence evaluated one anti-diagonal at a time in
numpy (the cells of an anti-diagonal do not depend on each other), for the 1023-label cases of the GPU tests; the CPU tests hold the two
equal.  Both return (counts, ops): counts = (distance, sub, del, ins) from the back-trace, after asserting that the forward-carried
counts say the same; ops is the alignment front to back."""
import functools
import itertools

import numpy as np

MATCH, SUB, DEL, INS = 0, 1, 2, 3


def _backtrace(op, Lr, Lh):
    i, j, ops = Lr, Lh, []
    while i > 0 or j > 0:
        o = int(op[i][j])
        ops.append(o)
        if o <= SUB:
            i, j = i - 1, j - 1
        elif o == DEL:
            i -= 1
        else:
            j -= 1
    ops.reverse()
    return ops


def _finish(dist, carried, ops):
    n = [ops.count(c) for c in (SUB, DEL, INS)]
    assert tuple(n) == tuple(carried), (n, carried)          # back-trace == the counts carried forward
    assert dist == sum(n)
    return (dist, n[0], n[1], n[2]), ops


def align_plain(ref, hyp):
    ref, hyp = list(ref), list(hyp)
    Lr, Lh = len(ref), len(hyp)
    D = [[0] * (Lh + 1) for _ in range(Lr + 1)]
    op = [[MATCH] * (Lh + 1) for _ in range(Lr + 1)]
    cnt = [[(0, 0, 0)] * (Lh + 1) for _ in range(Lr + 1)]
    for j in range(1, Lh + 1):
        D[0][j], op[0][j], cnt[0][j] = j, INS, (0, 0, j)
    for i in range(1, Lr + 1):
        D[i][0], op[i][0], cnt[i][0] = i, DEL, (0, i, 0)
        for j in range(1, Lh + 1):
            eq = ref[i - 1] == hyp[j - 1]
            best, o, src, add = D[i - 1][j - 1] + (0 if eq else 1), (MATCH if eq else SUB), cnt[i - 1][j - 1], (0 if eq else 1, 0, 0)
            if D[i - 1][j] + 1 < best:
                best, o, src, add = D[i - 1][j] + 1, DEL, cnt[i - 1][j], (0, 1, 0)
            if D[i][j - 1] + 1 < best:
                best, o, src, add = D[i][j - 1] + 1, INS, cnt[i][j - 1], (0, 0, 1)
            D[i][j], op[i][j], cnt[i][j] = best, o, tuple(a + b for a, b in zip(src, add))
    return _finish(D[Lr][Lh], cnt[Lr][Lh], _backtrace(op, Lr, Lh))


def align(ref, hyp):
    r, h = np.asarray(list(ref), dtype=np.int64), np.asarray(list(hyp), dtype=np.int64)
    Lr, Lh = len(r), len(h)
    D = np.zeros((Lr + 1, Lh + 1), dtype=np.int64)
    op = np.zeros((Lr + 1, Lh + 1), dtype=np.int8)
    cnt = np.zeros((Lr + 1, Lh + 1, 3), dtype=np.int64)
    D[0, :], D[:, 0] = np.arange(Lh + 1), np.arange(Lr + 1)
    op[0, 1:], op[1:, 0] = INS, DEL
    cnt[0, :, 2], cnt[:, 0, 1] = np.arange(Lh + 1), np.arange(Lr + 1)
    unit = np.eye(3, dtype=np.int64)
    for t in range(2, Lr + Lh + 1):
        i = np.arange(max(1, t - Lh), min(Lr, t - 1) + 1)
        j = t - i
        ne = (r[i - 1] != h[j - 1]).astype(np.int64)
        best, o = D[i - 1, j - 1] + ne, ne.astype(np.int8)             # MATCH = 0, SUB = 1
        c = cnt[i - 1, j - 1] + ne[:, None] * unit[0]
        up = D[i - 1, j] + 1 < best
        best, o = np.where(up, D[i - 1, j] + 1, best), np.where(up, DEL, o)
        c = np.where(up[:, None], cnt[i - 1, j] + unit[1], c)
        left = D[i, j - 1] + 1 < best
        best, o = np.where(left, D[i, j - 1] + 1, best), np.where(left, INS, o)
        c = np.where(left[:, None], cnt[i, j - 1] + unit[2], c)
        D[i, j], op[i, j], cnt[i, j] = best, o, c
    return _finish(int(D[Lr, Lh]), tuple(int(x) for x in cnt[Lr, Lh]), _backtrace(op, Lr, Lh))


def enumerate_alignments(ref, hyp):
    """every monotone alignment of two short strings as a tuple of operation codes (a diagonal step is a match or a substitution by
    the labels it joins): what the distance is the minimum over"""
    ref, hyp = list(ref), list(hyp)

    def rec(i, j):
        if i == len(ref) and j == len(hyp):
            yield ()
            return
        if i < len(ref) and j < len(hyp):
            o = MATCH if ref[i] == hyp[j] else SUB
            for rest in rec(i + 1, j + 1):
                yield (o,) + rest
        if i < len(ref):
            for rest in rec(i + 1, j):
                yield (DEL,) + rest
        if j < len(hyp):
            for rest in rec(i, j + 1):
                yield (INS,) + rest
    return rec(0, 0)


def cost(ops):
    return sum(1 for o in ops if o != MATCH)


@functools.lru_cache(maxsize=None)
def min_cost(ref, hyp):
    """the distance of two short tuples as the minimum over ALL their alignments"""
    return min(cost(a) for a in enumerate_alignments(ref, hyp))


def rule_path(ref, hyp):
    """the rule's alignment WITHOUT a table: from (Lr, Lh) backwards, the distance of every prefix pair by exhaustive enumeration, the
    predecessor chosen in the order diagonal, deletion, insertion among those that attain it"""
    ref, hyp = tuple(ref), tuple(hyp)
    dist = lambda i, j: min_cost(ref[:i], hyp[:j])   # noqa: E731
    i, j, ops = len(ref), len(hyp), []
    while i > 0 or j > 0:
        d = dist(i, j)
        if i > 0 and j > 0 and dist(i - 1, j - 1) + (ref[i - 1] != hyp[j - 1]) == d:
            ops.append(MATCH if ref[i - 1] == hyp[j - 1] else SUB)
            i, j = i - 1, j - 1
        elif i > 0 and dist(i - 1, j) + 1 == d:
            ops.append(DEL)
            i -= 1
        else:
            assert j > 0 and dist(i, j - 1) + 1 == d
            ops.append(INS)
            j -= 1
    ops.reverse()
    return ops


def replay(ref, hyp, ops):
    """walk the two strings by `ops`: True iff both are consumed exactly, every match joins equal labels and every substitution unequal"""
    i = j = 0
    for o in ops:
        if o <= SUB:
            if i >= len(ref) or j >= len(hyp) or (ref[i] == hyp[j]) != (o == MATCH):
                return False
            i, j = i + 1, j + 1
        elif o == DEL:
            i += 1
        elif o == INS:
            j += 1
        else:
            return False
    return i == len(ref) and j == len(hyp)


def all_strings(alphabet, max_len):
    for n in range(max_len + 1):
        yield from itertools.product(range(alphabet), repeat=n)
