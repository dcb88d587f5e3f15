"""A restatement of the Qwen2 path (csrc/llm.hip, infer/qwen2.py) in NumPy, float64 unless the arithmetic is pinned
to fp32 bits: the rotary table and the rotation (two fp32 products and one fp32 addition per element), which the kernels must
reproduce bit for bit, and the pick's walk over the survivors.  The CPU tests hold it against the ``transformers`` fixtures, the
GPU tests hold the kernels against it."""
import numpy as np
import torch

import whisper_sample_ref as SR

F32 = np.float32


# ---- fp32-pinned parts -----------------------------------------------------------------------------------------------------------
def rotary_table(dk, theta, n):
    """cos, sin f32 [n, dk / 2] as Qwen2RotaryEmbedding computes them (torch fp32 on the host)."""
    inv = 1.0 / (theta ** (torch.arange(0, dk, 2, dtype=torch.int64).float() / dk))
    f = torch.arange(n, dtype=torch.int64).float()[:, None] * inv[None, :]
    return f.cos().numpy(), f.sin().numpy()


def rope(x, cos, sin, pos):
    """x f32 [..., n, dk] at positions pos [n] (clamped below at 0) -> the rotated rows, fp32 bits of
    x * cos + rotate_half(x) * sin."""
    x = np.asarray(x, F32)
    half = x.shape[-1] // 2
    pos = np.maximum(np.asarray(pos), 0)
    c, s = cos[pos].astype(F32), sin[pos].astype(F32)
    a, b = x[..., :half], x[..., half:]
    return np.concatenate([(a * c).astype(F32) - (b * s).astype(F32), (b * c).astype(F32) + (a * s).astype(F32)], -1).astype(F32)


# ---- float64 parts ---------------------------------------------------------------------------------------------------------------
def rmsnorm(x, w, eps):
    x = np.asarray(x, np.float64)
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * np.asarray(w, np.float64)


def swiglu(gu):
    gu = np.asarray(gu, np.float64)
    I = gu.shape[-1] // 2
    g, u = gu[..., :I], gu[..., I:]
    return g / (1.0 + np.exp(-g)) * u


def gqa_append(qkv, kc, vc, begin, cos, sin, p0, U, H, Hkv, dk, scale):
    """What f5e_gqa_rope_append_f32 computes: qkv f32 [R * U, (H + 2 Hkv) dk]; kc / vc f32 [R, P, Hkv dk] are UPDATED in slots
    p0 .. p0+U-1 (rotated keys in fp32 bits, values as they are) -> out float64 [R * U, H dk].  begin [R] ints or None."""
    R = kc.shape[0]
    G = H // Hkv
    qkv = np.asarray(qkv, F32).reshape(R, U, -1)
    out = np.zeros((R, U, H * dk))
    for r in range(R):
        lo = 0 if begin is None else min(max(int(begin[r]), 0), p0 + U)
        pos = np.arange(p0, p0 + U) - lo
        q = rope(qkv[r, :, :H * dk].reshape(U, H, dk).transpose(1, 0, 2), cos, sin, pos)              # [H, U, dk]
        k = rope(qkv[r, :, H * dk:(H + Hkv) * dk].reshape(U, Hkv, dk).transpose(1, 0, 2), cos, sin, pos)
        kc[r, p0:p0 + U] = k.transpose(1, 0, 2).reshape(U, Hkv * dk)
        vc[r, p0:p0 + U] = qkv[r, :, (H + Hkv) * dk:]
        for u in range(U):
            j1 = p0 + u
            if j1 < lo:
                continue
            K = kc[r, lo:j1 + 1].reshape(-1, Hkv, dk).astype(np.float64)
            Vv = vc[r, lo:j1 + 1].reshape(-1, Hkv, dk).astype(np.float64)
            for h in range(H):
                s = K[:, h // G] @ q[h, u].astype(np.float64) * scale
                w = np.exp(s - s.max())
                out[r, u, h * dk:(h + 1) * dk] = (w / w.sum()) @ Vv[:, h // G]
    return out.reshape(R * U, H * dk)


class Model:
    """The float64 model on a fixture's state dict (fp32 arrays under transformers' names)."""

    def __init__(self, sd, cfg):
        self.sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
        self.cfg = cfg
        self.cos, self.sin = rotary_table(cfg["head_dim"], cfg["rope_theta"], cfg.get("positions", 128))

    def new_caches(self, R, P):
        c = self.cfg
        return [(np.zeros((R, P, c["kv_heads"] * c["head_dim"]), F32), np.zeros((R, P, c["kv_heads"] * c["head_dim"]), F32))
                for _ in range(c["layers"])]

    def append(self, caches, ids, begin, p0, hidden=None):
        """ids [R, U] at positions p0 .. -> logits float64 [R, V] of the last position."""
        c, sd = self.cfg, self.sd
        H, Hkv, dk = c["heads"], c["kv_heads"], c["head_dim"]
        ids = np.asarray(ids)
        R, U = ids.shape
        x = sd["model.embed_tokens.weight"][ids.reshape(-1)]
        for i in range(c["layers"]):
            p = f"model.layers.{i}."
            if hidden is not None:
                hidden.append(x.reshape(R, U, -1).copy())
            xn = rmsnorm(x, sd[p + "input_layernorm.weight"], c["eps"])
            qkv = np.concatenate([xn @ sd[p + f"self_attn.{n}_proj.weight"].T + sd[p + f"self_attn.{n}_proj.bias"] for n in "qkv"], 1)
            ao = gqa_append(qkv.astype(F32), caches[i][0], caches[i][1], begin, self.cos, self.sin, p0, U, H, Hkv, dk, dk ** -0.5)
            x = x + ao @ sd[p + "self_attn.o_proj.weight"].T
            xn = rmsnorm(x, sd[p + "post_attention_layernorm.weight"], c["eps"])
            gu = np.concatenate([xn @ sd[p + "mlp.gate_proj.weight"].T, xn @ sd[p + "mlp.up_proj.weight"].T], 1)
            x = x + swiglu(gu) @ sd[p + "mlp.down_proj.weight"].T
        if hidden is not None:
            hidden.append(x.reshape(R, U, -1).copy())
        xl = rmsnorm(x.reshape(R, U, -1)[:, -1], sd["model.norm.weight"], c["eps"])
        head = sd["model.embed_tokens.weight"] if c["tied"] else sd["lm_head.weight"]
        return xl @ head.T

    def greedy(self, ids, begin, n_new, penalty):
        """-> (tokens [R, n_new], caches, the table of all ids): the arg max of the penalised logits, step by step."""
        ids = np.asarray(ids)
        R, U = ids.shape
        caches = self.new_caches(R, U + n_new)
        table = np.concatenate([ids, np.zeros((R, n_new), ids.dtype)], 1)
        logits = self.append(caches, ids, begin, 0)
        for t in range(n_new):
            for r in range(R):
                table[r, U + t] = int(np.argmax(penalise(logits[r], table[r, int(begin[r]):U + t], penalty)))
            if t + 1 < n_new:
                logits = self.append(caches, table[:, U + t:U + t + 1], begin, U + t)
        return table[:, U:], caches, table


# ---- the pick --------------------------------------------------------------------------------------------------------------------
def penalise(x, hist, penalty):
    x = np.array(x, copy=True)
    seen = np.unique(np.asarray(hist, np.int64))
    seen = seen[(seen >= 0) & (seen < x.shape[0])]
    x[seen] = np.where(x[seen] < 0, x[seen] * x.dtype.type(penalty), x[seen] / x.dtype.type(penalty))
    return x


def survivors(x, hist, penalty, temperature, top_k, top_p):
    """The pick's survivors of one fp32 logits row: (ids, e) in descending order, e = exp(y - y_max) in fp32; the renormalised
    probabilities are e / e.sum().  Exactly top_k survive the top-k filter, the lower id first on equal values."""
    y = penalise(np.asarray(x, F32), hist, penalty)
    y = (y / F32(temperature)).astype(F32)
    order = np.lexsort((np.arange(y.shape[0]), -y.astype(np.float64)))[:top_k]
    ys = y[order]
    e = np.exp((ys - ys[0]).astype(F32)).astype(F32)
    S = F32(0)
    for v in e[::-1]:
        S = F32(S + v)
    keep, cum, cut = top_k, F32(0), F32(F32(1) - F32(top_p))
    for i in range(top_k - 1, 0, -1):
        cum = F32(cum + F32(e[i] / S))
        if cum <= cut:
            keep = i
        else:
            break
    return order[:keep], e[:keep]


def draw_u(seed, row_key, serial, p):
    w = SR.philox4x32_10((0, p, serial, row_key), (seed & SR.MASK, (seed >> 32) & SR.MASK))
    return float(SR.uniform(w[0]))


def draw(e, u):
    """The first survivor whose sequential fp32 cumulative sum reaches u * total -> (index, the relative distance of u * total
    to the nearest cumulative boundary)."""
    total = F32(0)
    for v in e:
        total = F32(total + v)
    target = F32(F32(u) * total)
    c, pick = F32(0), len(e) - 1
    for i, v in enumerate(e):
        c = F32(c + v)
        if c >= target:
            pick = i
            break
    full = np.cumsum(np.asarray(e, np.float64))
    margin = float(np.min(np.abs(full - float(u) * full[-1])) / full[-1])
    return pick, margin


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
def load_fixture():
    """tests/golden/qwen2.npz -> (arrays, the state dict as fp32 arrays, the restatement's configuration)."""
    import json
    import os
    fx = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qwen2.npz")))
    sd = {k[2:]: (v.astype(np.uint32) << np.uint32(16)).view(F32) for k, v in fx.items() if k.startswith("w/")}
    hf = json.loads(str(fx["cfg"]))
    cfg = dict(heads=hf["num_attention_heads"], kv_heads=hf["num_key_value_heads"],
               head_dim=hf["hidden_size"] // hf["num_attention_heads"], layers=hf["num_hidden_layers"], eps=hf["rms_norm_eps"],
               rope_theta=hf["rope_theta"], tied=hf["tie_word_embeddings"], positions=128, hf=hf)
    return fx, sd, cfg


def logits_row(V, k):
    """Row k of the pick tests' logits, f32 [V]: 4 (u1 + u2 + u3 - 1.5) from three Philox words per class (exact dyadic sums, so
    every platform makes the same bits)."""
    blocks = np.arange(V, dtype=np.uint64)
    w = SR.philox4x32_10((blocks, k, 7, 11), (0x51ED270B, 0x2545F491))
    u = sum((x >> np.uint64(8)).astype(np.float64) for x in w[:3]) * 2.0 ** -24
    return (4.0 * (u - 1.5)).astype(F32)


def history_row(V, k, x, n=12):
    """The token history of row k: the three largest classes of x, a class repeated, and others drawn from Philox."""
    w = SR.philox4x32_10((np.arange(n, dtype=np.uint64), k, 3, 5), (0x9E3779B9, 0x7F4A7C15))
    rnd = [int(v) % V for v in w[0]]
    top = np.argsort(-x.astype(np.float64), kind="stable")[:3].tolist()
    return top + rnd + rnd[:2]
