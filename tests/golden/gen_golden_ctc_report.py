#!/usr/bin/env python3
"""Record g28_ctc_report.npz by RUNNING THE REFERENCE's calc_recall_precision (criterion/joint_ctc_criterion.py:24-48) and the blank
rate of JointCTCCriterion.forward (:101) on a few small integer cases.

    python tests/golden/gen_golden_ctc_report.py

The module is imported by file path from /root/reference (never copied); fairseq, which it imports for its registries, base classes
and logging helpers only, is replaced for the import by the stand-ins of gen_golden_losses.py (no arithmetic of this path).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden_losses import _mod  # noqa: E402


def load_reference_criterion():
    from dataclasses import dataclass

    @dataclass
    class _Cfg:
        pass

    class _Base:
        def __init__(self, *a, **k):
            pass

    ident = lambda *a, **k: (lambda cls: cls)
    _mod("fairseq", metrics=types.SimpleNamespace(), utils=types.SimpleNamespace())
    _mod("fairseq.logging")
    _mod("fairseq.logging.meters", safe_round=round)
    _mod("fairseq.criterions", register_criterion=ident)
    _mod("fairseq.criterions.label_smoothed_cross_entropy", LabelSmoothedCrossEntropyCriterion=_Base,
         LabelSmoothedCrossEntropyCriterionConfig=_Cfg)
    spec = importlib.util.spec_from_file_location("ref_joint_ctc_criterion", "/root/reference/codebase/criterion/joint_ctc_criterion.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    ref = load_reference_criterion()
    g = torch.Generator().manual_seed(28)
    out = {}
    # (N, S, T, labels, blank, pad): random paths with many blanks and repeats, padded targets; one case with another blank / pad index,
    # one where the path holds the pad index and the target the blank index (the function does not exclude either from the match)
    cases = [(4, 12, 5, 9, 0, 1), (6, 7, 4, 6, 0, 1), (1, 1, 1, 4, 0, 1), (3, 10, 6, 12, 3, 2), (5, 9, 3, 5, 0, 1)]
    for ci, (N, S, T, V, blank, pad) in enumerate(cases):
        path = torch.randint(0, V, (N, S), generator=g)
        path[torch.rand(N, S, generator=g) < 0.4] = blank
        if S > 3:
            path[:, 2] = path[:, 1]                                                     # repeats
        tl = torch.randint(1, T + 1, (N,), generator=g)
        target = torch.randint(0, V, (N, T), generator=g)
        if ci != 4:
            target[target == blank] = (blank + 4) % V if (blank + 4) % V != pad else (blank + 5) % V
        target[torch.arange(T).unsqueeze(0) >= tl.unsqueeze(1)] = pad
        if ci == 0:
            path[0] = blank                                                             # an all-blank row: precision 0 / eps
        recall, precision = ref.calc_recall_precision(path, target, blank_idx=blank, pad_idx=pad)
        blank_rate = path.eq(blank).float().mean(-1).sum()                              # joint_ctc_criterion.py:101 on y_pred = path
        out.update({f"c{ci}.path": path.numpy(), f"c{ci}.target": target.numpy(), f"c{ci}.blank_pad": np.array([blank, pad]),
                    f"c{ci}.out": np.array([float(recall), float(precision), float(blank_rate)], dtype=np.float64)})
        print(ci, float(recall), float(precision), float(blank_rate))
    out["n_cases"] = np.array(len(cases))
    np.savez_compressed(os.path.join(HERE, "g28_ctc_report.npz"), **out)
    print("wrote g28_ctc_report.npz with", len(out), "arrays")


if __name__ == "__main__":
    main()
