"""NumPy restatement of f5e_ctc_loss (csrc/ctc.hip, include/f5e_abi.h): log of the sum over all CTC paths, one row per step.
``dtype=np.float32`` does what the kernel does (every operation rounded to fp32, logaddexp = max + log1p(exp(-|d|)) applied
to (stay, s-1) and then s-2, the frame normaliser max + log1p(sum over the other classes of exp(x - max))); ``np.float64``
is the same recurrence in double precision.  Pinned against torch.nn.functional.ctc_loss and the reference's ``CTC.forward``
(tests/golden/ctc_loss.npz) by tests/test_ctc_loss_cpu.py."""
import numpy as np


def tolerance(T, ref):
    """One fp32 rounding at the magnitude of the running value per frame, plus the closing logaddexp and the normaliser."""
    return (4 + T) * 2.0 ** -24 * max(1.0, abs(float(ref)))


def logaddexp(a, b, dtype):
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    m = np.maximum(a, b)
    with np.errstate(invalid="ignore", over="ignore"):
        r = (m + np.log1p(np.exp(-np.abs(a - b)).astype(dtype)).astype(dtype)).astype(dtype)
    return np.where(np.isneginf(m), m, r).astype(dtype)


def frame_lse(scores, dtype):
    """logsumexp of every row, [T, V] -> [T]; 0 for a row of -inf (its log-probabilities stay -inf)."""
    x = np.asarray(scores, dtype)
    arg = x.argmax(-1)
    m = x.max(-1)
    dead = np.isneginf(m)
    with np.errstate(invalid="ignore"):
        e = np.exp((x - m[:, None]).astype(dtype)).astype(dtype)
    e[np.arange(len(x)), arg] = 0
    e[dead] = 0
    rest = e.sum(-1, dtype=dtype)
    return np.where(dead, 0, (np.where(dead, 0, m) + np.log1p(rest).astype(dtype))).astype(dtype)


def has_path(labels, t_len, V):
    labels = np.asarray(labels)
    if t_len < 1 or ((labels < 0) | (labels >= V)).any():
        return False
    return t_len >= len(labels) + int((labels[1:] == labels[:-1]).sum())


def loss_one(scores, labels, blank=0, dtype=np.float32):
    """scores [T, V] (raw logits or log-probabilities, -inf allowed), labels [l] (l >= 0) -> log P(labels | frames)."""
    scores = np.asarray(scores, dtype)
    labels = np.asarray(labels, np.int64)
    T, V = scores.shape
    NEG = dtype(-np.inf)
    if not has_path(labels, T, V):
        return NEG
    ext = np.full(2 * len(labels) + 1, blank, np.int64)
    ext[1::2] = labels
    S = len(ext)
    s_idx = np.arange(S)
    skip = (s_idx & 1).astype(bool) & (s_idx >= 3) & (ext != np.roll(ext, 2))
    lp = (scores[:, ext] - frame_lse(scores, dtype)[:, None]).astype(dtype)
    alpha = np.full(S, NEG, dtype)
    alpha[:2] = lp[0, :2]
    for t in range(1, T):
        one = np.concatenate([[NEG], alpha[:-1]]).astype(dtype)
        two = np.where(skip, np.concatenate([[NEG, NEG], alpha[:-2]])[:S], NEG).astype(dtype)
        alpha = (logaddexp(logaddexp(alpha, one, dtype), two, dtype) + lp[t]).astype(dtype)
    return dtype(logaddexp(alpha[S - 1], alpha[S - 2] if S > 1 else NEG, dtype))


def loss(scores, labels, t_len, l_len, blank=0, dtype=np.float32):
    """Batched form with the kernel's conventions: scores [B, T, V], labels [B, L] -> logp [B]; -inf without a path."""
    scores, labels = np.asarray(scores), np.asarray(labels)
    B, T, V = scores.shape
    L = labels.shape[1]
    out = np.full(B, -np.inf, dtype)
    for b in range(B):
        t, l = int(t_len[b]), int(l_len[b])
        if 0 <= l <= L and 1 <= t <= T:
            out[b] = loss_one(scores[b, :t], labels[b, :l], blank, dtype)
    return out


def torch_logp(scores, labels, t_len, l_len, blank=0):
    """-torch.nn.functional.ctc_loss(reduction="none") on the float64 log_softmax, on the host: THE reference of the tests.
    scores [B, T, V], labels [B, L], lengths [B] -> float64 [B] (-inf where torch says +inf)."""
    import torch
    import torch.nn.functional as F
    x = torch.as_tensor(np.asarray(scores), dtype=torch.float64)
    lp = F.log_softmax(x, dim=-1).transpose(0, 1)
    y = torch.as_tensor(np.asarray(labels), dtype=torch.long)
    out = F.ctc_loss(lp, y, torch.as_tensor(np.asarray(t_len), dtype=torch.long),
                     torch.as_tensor(np.asarray(l_len), dtype=torch.long), blank=blank, reduction="none")
    return -out.numpy()
