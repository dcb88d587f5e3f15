"""Makes tests/golden/qwen2_sample.npz with ``transformers``' four sampling processors (5.15.0 when this was run), in the order the
sampling call builds them: RepetitionPenalty, Temperature, TopK, TopP.

64 logit rows, 32 of V = 384 and 32 of V = 151936, are made by ``qwen2_ref.logits_row`` (integer Philox and exact sums: the tests
remake the same bits) with the histories of ``qwen2_ref.history_row``.  For each row and each setting (penalty, temperature,
top_k, top_p) the survivors (ids in descending order of probability, -1 padded) and their probabilities are stored.  Rows are
the first for which no two of the 65 largest penalised values are equal and no ascending cumulative sum lies within 1e-4 of
1 - top_p, in any setting; both are asserted.

    python tests/golden/make_qwen2_sample_golden.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import qwen2_ref as Q  # noqa: E402

SETTINGS = ((1.05, 0.7, 20, 0.95), (1.05, 0.7, 20, 0.8), (1.0, 1.0, 64, 1.0), (1.3, 0.3, 1, 0.5))
SIZES = (384, 151936)
ROWS_PER_SIZE = 32


def process(x, hist, setting):
    from transformers.generation.logits_process import (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper)
    pen, T, k, p = setting
    ids = torch.tensor([hist], dtype=torch.long)
    s = torch.from_numpy(x)[None].clone()
    for proc in (RepetitionPenaltyLogitsProcessor(pen), TemperatureLogitsWarper(T), TopKLogitsWarper(k), TopPLogitsWarper(p)):
        s = proc(ids, s)
    return s[0]


def row_ok(x, hist):
    """-> per setting (ids, probs), or None when the row breaks a condition."""
    out = []
    for setting in SETTINGS:
        pen, T, k, p = setting
        y = np.sort(Q.penalise(x, hist, pen).astype(np.float64) / T)[::-1][:65]
        if (np.diff(y) == 0).any():
            return None
        s = process(x, hist, setting)
        probs = torch.softmax(s, -1).numpy()
        ids = np.nonzero(np.isfinite(s.numpy()))[0]
        ids = ids[np.argsort(-probs[ids], kind="stable")]
        top = np.sort(Q.penalise(x, hist, pen).astype(np.float64) / T)[::-1][:k]
        q = np.exp(top - top[0])
        cum = np.cumsum((q / q.sum())[::-1])
        if (np.abs(cum - (1 - p)) < 1e-4).any():
            return None
        out.append((ids, probs[ids]))
    return out


def main():
    fx = dict(settings=np.array(SETTINGS, np.float64))
    for V in SIZES:
        rows, k = [], 0
        while len(rows) < ROWS_PER_SIZE:
            x = Q.logits_row(V, k)
            hist = Q.history_row(V, k, x)
            res = row_ok(x, hist)
            if res is not None:
                rows.append((k, hist, res))
            k += 1
        assert len(rows) == ROWS_PER_SIZE
        fx[f"rows_{V}"] = np.array([r[0] for r in rows], np.int32)
        fx[f"hist_{V}"] = np.array([r[1] for r in rows], np.int32)
        for si in range(len(SETTINGS)):
            ids = np.full((ROWS_PER_SIZE, 64), -1, np.int32)
            pr = np.zeros((ROWS_PER_SIZE, 64), np.float32)
            for i, r in enumerate(rows):
                a, b = r[2][si]
                ids[i, :len(a)], pr[i, :len(a)] = a, b
            fx[f"keep_id_{V}_{si}"], fx[f"keep_p_{V}_{si}"] = ids, pr
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "qwen2_sample.npz")
    np.savez_compressed(path, **fx)
    print({V: fx[f"rows_{V}"].tolist()[-3:] for V in SIZES}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
