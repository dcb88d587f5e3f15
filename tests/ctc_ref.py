"""NumPy restatement of the CTC semantics of csrc/ctc.hip (include/f5e_abi.h: f5e_ctc_align, f5e_ctc_greedy), one row per step.
Pinned against the reference's own ``forced_align`` / ``ctc_greedy_search`` by tests/golden/ctc_align.npz and ctc_asr.npz
(tests/golden/make_ctc_golden.py); the GPU tests use it on shapes the reference's Python loop cannot cover.

``wrap=True`` restates the reference literally, including its negative index at state 0 (``log_alpha[t-1, -1]`` is the LAST
state): the generator uses it to show where the reference's output comes from on scores that are not peaky."""
import numpy as np

NEG = np.float32(-np.inf)


def extend(labels, blank):
    ext = np.full(2 * len(labels) + 1, blank, np.int64)
    ext[1::2] = labels
    return ext


def feasible(labels, t_len, V=None):
    labels = np.asarray(labels)
    if len(labels) < 1 or t_len < 1:
        return False
    if V is not None and ((labels < 0) | (labels >= V)).any():
        return False
    return t_len >= len(labels) + int((labels[1:] == labels[:-1]).sum())


def align_one(scores, labels, blank=0, wrap=False):
    """scores f32 [T, V], labels [l] -> (align [T] classes, states [T], tok_start [l], tok_end [l], score f32).
    The caller checks ``feasible`` first."""
    scores = np.asarray(scores, np.float32)
    labels = np.asarray(labels, np.int64)
    T, l = scores.shape[0], len(labels)
    ext = extend(labels, blank)
    S = len(ext)
    s_idx = np.arange(S)
    skip = (ext != blank) & (s_idx >= 2) & (ext != np.roll(ext, 2))
    alpha = np.full(S, NEG, np.float32)
    alpha[0], alpha[1] = scores[0, ext[0]], scores[0, ext[1]]
    dec = np.zeros((T, S), np.int8)
    for t in range(1, T):
        stay = alpha
        one = np.roll(alpha, 1)
        two = np.roll(alpha, 2)
        if not wrap:
            one = one.copy()
            one[0] = NEG
        two = np.where(skip, two, NEG).astype(np.float32)
        best, d = stay, np.zeros(S, np.int8)
        d = np.where(one > best, 1, d)
        best = np.where(one > best, one, best)
        d = np.where(two > best, 2, d)
        best = np.where(two > best, two, best)
        dec[t] = d
        alpha = (best + scores[t, ext]).astype(np.float32)     # one fp32 add
    end = S - 1 if alpha[S - 1] >= alpha[S - 2] else S - 2
    states = np.zeros(T, np.int64)
    states[T - 1] = end
    for t in range(T - 1, 0, -1):
        states[t - 1] = (states[t] - dec[t, states[t]]) % S      # % S: the wrap of the literal restatement
    start, stop = np.zeros(l, np.int32), np.zeros(l, np.int32)
    for i in range(l):
        on = np.nonzero(states == 2 * i + 1)[0]
        if len(on):
            start[i], stop[i] = on[0], on[-1] + 1
    return ext[states].astype(np.int32), states, start, stop, np.float32(alpha[end])


def align(scores, labels, t_len, l_len, blank=0):
    """Batched form with the kernel's conventions: scores [B, T, V], labels [B, L] -> align [B, T] (-1 past t_len),
    tok_start / tok_end [B, L], score [B]; a sequence without a path gets -1 / 0 / -inf rows."""
    scores, labels = np.asarray(scores, np.float32), np.asarray(labels)
    B, T, V = scores.shape
    L = labels.shape[1]
    al = np.full((B, T), -1, np.int32)
    ts, te = np.zeros((B, L), np.int32), np.zeros((B, L), np.int32)
    sc = np.full(B, NEG, np.float32)
    for b in range(B):
        t, l = int(t_len[b]), int(l_len[b])
        if not (1 <= l <= L and 1 <= t <= T and feasible(labels[b, :l], t, V)):
            continue
        a, _, s0, s1, v = align_one(scores[b, :t], labels[b, :l], blank)
        al[b, :t], ts[b, :l], te[b, :l], sc[b] = a, s0, s1, v
    return al, ts, te, sc


def is_ctc_path(classes, labels, blank=0):
    """classes [T]: does the frame sequence collapse to ``labels`` along ONE pass through blank, y0, blank, y1, ...?"""
    ext = extend(np.asarray(labels), blank)
    s = 0 if classes[0] == ext[0] else 1
    if classes[0] != ext[s]:
        return False
    for c in classes[1:]:
        for step in (0, 1, 2):
            n = s + step
            if n < len(ext) and ext[n] == c and (step < 2 or (ext[n] != blank and ext[n] != ext[s])):
                s = n
                break
        else:
            return False
    return s >= len(ext) - 2


def path_score(logp, classes):
    """Sum of the frame log-probabilities along a path, in fp64."""
    return float(np.asarray(logp, np.float64)[np.arange(len(classes)), classes].sum())


def collapse(ids, blank=0):
    out, before = [], -1
    for i in ids:
        if i != blank and i != before:
            out.append(int(i))
        before = i
    return out


def greedy(scores, t_len, blank=0, pad_id=-1):
    """scores [B, T, V] -> (hyps: list of lists, frame_logp f64 [B, T]).  Frames past t_len take pad_id (>= 0) or are skipped."""
    scores = np.asarray(scores)
    B, T, V = scores.shape
    ids = scores.argmax(-1)
    x = scores.astype(np.float64)
    m = x.max(-1)
    logp = -np.log(np.exp(x - m[..., None]).sum(-1))
    hyps = []
    for b in range(B):
        t = min(max(int(t_len[b]), 0), T)
        row = ids[b, :t].tolist() + ([pad_id] * (T - t) if pad_id >= 0 else [])
        hyps.append(collapse(row, blank))
    return hyps, logp


def planted(T, labels, V, seed, blank=0, boost=4.0):
    """Unit-variance noise plus ``boost`` on the class of a seeded random valid alignment -> raw logits f32 [T, V]."""
    rng = np.random.default_rng(seed)
    labels = np.asarray(labels)
    assert feasible(labels, T)
    ext = extend(labels, blank)
    # forced frames: one per label, one blank between equal neighbours; the slack goes to random states
    need = np.zeros(len(ext), np.int64)
    need[1::2] = 1
    need[2:-1:2] = (labels[1:] == labels[:-1]).astype(np.int64)
    extra = rng.multinomial(T - need.sum(), np.full(len(ext), 1.0 / len(ext)))
    states = np.repeat(np.arange(len(ext)), need + extra)
    logits = rng.standard_normal((T, V)).astype(np.float32)
    logits[np.arange(T), ext[states]] += np.float32(boost)
    return logits


def log_softmax(x):
    x = np.asarray(x, np.float32)
    m = x.max(-1, keepdims=True)
    return (x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))).astype(np.float32)


def speech_edit_recipe(audio, sr, hop, parts, fix):
    """The reference's audio / mask assembly, literally (infer/speech_edit.py:141-160: tensors, F.pad, fix_duration.pop(0)):
    audio [1, n] torch tensor -> (assembled audio, edit_mask [1, n' // hop + 1])."""
    import torch
    import torch.nn.functional as F
    fix = list(fix) if fix is not None else None
    offset = 0
    audio_ = torch.zeros(1, 0)
    edit_mask = torch.zeros(1, 0, dtype=torch.bool)
    for part in parts:
        start, end = part
        part_dur = end - start if fix is None else fix.pop(0)
        part_dur = part_dur * sr
        start = start * sr
        audio_ = torch.cat((audio_, audio[:, round(offset):round(start)], torch.zeros(1, round(part_dur))), dim=-1)
        edit_mask = torch.cat((edit_mask, torch.ones(1, round((start - offset) / hop), dtype=torch.bool),
                               torch.zeros(1, round(part_dur / hop), dtype=torch.bool)), dim=-1)
        offset = end * sr
    audio = torch.cat((audio_, audio[:, round(offset):]), dim=-1)
    edit_mask = F.pad(edit_mask, (0, audio.shape[-1] // hop - edit_mask.shape[-1] + 1), value=True)
    return audio, edit_mask
