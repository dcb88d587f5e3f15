"""NumPy restatement of Whisper's token timestamps as ``transformers`` computes them (generation_whisper.py:
``_extract_token_timestamps`` with the frame count given, ``_median_filter``, ``_dynamic_time_warping``), pinned to
tests/golden/whisper_align.npz by tests/test_whisper_align_cpu.py and used as the reference of the GPU tests.  Every function takes
the dtype it computes in: float64 is the yardstick, float32 is what the rounding of a faithful fp32 evaluation looks like.  It
shares no code with f5e_tts_amd/eval/whisper.py or the kernels.

The rules, for one utterance (tokens[0..n), n0 prompt tokens, M = frames // 2 encoder positions clamped to 1 .. 1500):
  1. row t of an alignment head = the softmax over ALL encoder keys of the query of the token at position n0 + t, cut to M
     columns; t = 0 .. N - 1, N = n - n0 - 1 (n - n0 with include_last)
  2. per head and column: z = (p - mean) / std over the N rows (population std)
  3. median of width w along the columns, reflect padding (rows of M <= w // 2 columns stay as they are)
  4. C = -(mean over the heads)
  5. cost[i][j] = C[i-1][j-1] + (diagonal if it is strictly the smallest, else up if it is strictly the smallest, else left)
  6. backtrace from (N, M); first[t] = the column at which the path enters row t; time = 0.02 first[t]
  7. N = 0: all zero; N = 1: zero (special-cased here, NaN in the reference)."""
import json
import os

import numpy as np

import whisper_ref

HERE = os.path.dirname(os.path.abspath(__file__))


def load_fixture():
    z = np.load(os.path.join(HERE, "golden", "whisper_align.npz"))
    fx = {k: z[k] for k in z.files if not k.startswith("wb/")}
    fx["sd_b"] = {k[3:]: (z[k].astype(np.uint32) << 16).view(np.float32) for k in z.files if k.startswith("wb/")}
    fx["eos_row_b_f32"] = (fx["eos_row_b"].astype(np.uint32) << 16).view(np.float32)
    fx["names"] = json.loads(str(fx["case_names"]))
    fx["words"] = json.loads(str(fx["word_json"]))
    return fx


# ---- rule 1 -----------------------------------------------------------------------------------------------------------------------
def alignment_probs(ref, enc, ids, heads, n0, N, M):
    """The float64 model of tests/whisper_ref.py (``ref``: its Ref) run over the whole prefix: -> [len(heads)][N][M], the
    cross-attention weights of the queries at positions n0 .. n0 + N - 1 for the (layer, head) pairs, softmax over all keys."""
    cfg = ref.cfg
    pre = "model.decoder"
    ids = np.asarray(ids)[:n0 + N]
    H = cfg["decoder_attention_heads"]
    dk = cfg["d_model"] // H
    x = ref.w(pre + ".embed_tokens.weight")[ids] + ref.w(pre + ".embed_positions.weight")[:len(ids)]
    out = {}
    for i in range(cfg["decoder_layers"]):
        lp = f"{pre}.layers.{i}"
        h = ref.ln(x, lp + ".self_attn_layer_norm")
        x = x + ref.attn(h, h, lp + ".self_attn", H, causal=True)
        h = ref.ln(x, lp + ".encoder_attn_layer_norm")
        q = ref.lin(h, lp + ".encoder_attn.q_proj") * dk ** -0.5
        k = ref.lin(enc, lp + ".encoder_attn.k_proj", bias=False)
        for (l, hd) in heads:
            if l == i:
                s = q[:, hd * dk:(hd + 1) * dk] @ k[:, hd * dk:(hd + 1) * dk].T
                s = np.exp(s - s.max(-1, keepdims=True))
                out[(l, hd)] = (s / s.sum(-1, keepdims=True))[n0:n0 + N, :M]
        x = x + ref.attn(h, enc, lp + ".encoder_attn", H)
        h = ref.ln(x, lp + ".final_layer_norm")
        x = x + ref.lin(whisper_ref.gelu(ref.lin(h, lp + ".fc1")), lp + ".fc2")
    return np.stack([out[(l, hd)] for l, hd in heads])


def softmax_rows(q, k, scale, dtype=np.float64):
    """q [dk], k [Tk][dk] -> softmax over all Tk keys."""
    s = (k.astype(dtype) @ q.astype(dtype)) * dtype(scale)
    e = np.exp(s - s.max())
    return e / e.sum()


# ---- rules 2-4 ----------------------------------------------------------------------------------------------------------------------
def median_filter(z, width):
    """z [..., M]: the median of ``width`` neighbours along the last axis, reflect padding; unchanged when M <= width // 2."""
    pad = width // 2
    if z.shape[-1] <= pad:
        return z
    zp = np.pad(z, [(0, 0)] * (z.ndim - 1) + [(pad, pad)], mode="reflect")
    win = np.stack([zp[..., k:k + z.shape[-1]] for k in range(width)], -1)
    return np.sort(win, -1)[..., pad]


def cost_matrix(probs, width=7, dtype=np.float64):
    """probs [heads][N][M] -> C [N][M] in ``dtype``."""
    p = np.asarray(probs).astype(dtype)
    N = p.shape[1]
    mean = (p.sum(1, keepdims=True, dtype=dtype) / dtype(N)).astype(dtype)
    std = np.sqrt(((p - mean) ** 2).sum(1, keepdims=True, dtype=dtype) / dtype(N)).astype(dtype)
    z = ((p - mean) / std).astype(dtype)
    z = median_filter(z, width)
    return (-(z.sum(0, dtype=dtype) / dtype(p.shape[0]))).astype(dtype)


# ---- rules 5-6 ----------------------------------------------------------------------------------------------------------------------
def dtw_first_loop(C):
    """The recursion written cell by cell in the dtype of C (the sum of two values of a dtype, rounded to it) and the backtrace;
    -> first int [N]."""
    C = np.asarray(C)
    dt = C.dtype.type
    N, M = C.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype=C.dtype)
    cost[0, 0] = 0
    move = np.full((N + 1, M + 1), 2, np.int8)
    for i in range(1, N + 1):
        for j in range(1, M + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = dt(C[i - 1, j - 1] + c)
            move[i, j] = t
    return backtrace(move, N, M)


def backtrace(move, N, M):
    first = np.full(N, -1, np.int64)
    i, j = N, M
    while i > 0 or j > 0:
        t = 2 if i == 0 else 1 if j == 0 else int(move[i, j])
        if i > 0 and t != 2:
            first[i - 1] = j - 1                                  # the path leaves row i: the column at which it entered it
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return first


def dtw_first(C):
    """The same recursion evaluated one anti-diagonal i + j at a time (its cells do not depend on each other), which NumPy can do
    as array operations: what the large cases of the GPU tests use.  tests/test_whisper_align_cpu.py checks it against
    ``dtw_first_loop``."""
    C = np.asarray(C)
    N, M = C.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype=C.dtype)
    cost[0, 0] = 0
    move = np.full((N + 1, M + 1), 2, np.int8)
    for d in range(2, N + M + 1):
        i = np.arange(max(1, d - M), min(N, d - 1) + 1)
        j = d - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        diag = (c0 < c1) & (c0 < c2)
        up = ~diag & (c1 < c0) & (c1 < c2)
        t = np.where(diag, 0, np.where(up, 1, 2)).astype(np.int8)
        c = np.where(diag, c0, np.where(up, c1, c2))
        cost[i, j] = (C[i - 1, j - 1] + c).astype(C.dtype)
        move[i, j] = t
    return backtrace(move, N, M)


# ---- the whole thing ------------------------------------------------------------------------------------------------------------------
def token_frames(probs, n, n0, width=7, dtype=np.float64, include_last=False):
    """probs [heads][N][M] of one utterance -> int [n]: zeros for the prompt, first[t] at position n0 + t, and (without
    include_last) the last position repeating the one before it."""
    N = n - n0 - (0 if include_last else 1)
    out = np.zeros(n, np.int64)
    if N <= 0:
        return out
    probs = np.asarray(probs)
    assert probs.shape[1] == N, (probs.shape, N)
    first = np.zeros(N, np.int64) if N == 1 else dtw_first(cost_matrix(probs, width, dtype))
    out[n0:n0 + N] = first
    if not include_last:
        out[n - 1] = out[n - 2]
    return out
