"""Float64 NumPy restatement of Whisper as ``transformers`` computes it (feature extractor, encoder, decoder, greedy loop with the two
suppress rules), pinned to tests/golden/whisper.npz by tests/test_whisper_cpu.py and used as the reference of the GPU tests.  It
shares no code with f5e_tts_amd/eval/whisper.py except the host constants it is handed (window, filterbank)."""
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_FFT, HOP = 400, 160


# ---- the fixture -----------------------------------------------------------------------------------------------------------------
def load_fixture():
    z = np.load(os.path.join(HERE, "golden", "whisper.npz"))
    fx = {k: z[k] for k in z.files if not k.startswith("w/")}
    fx["sd"] = {k[2:]: (z[k].astype(np.uint32) << 16).view(np.float32) for k in z.files if k.startswith("w/")}
    fx["config"] = json.loads(str(fx["config_json"]))
    fx["generation_config"] = json.loads(str(fx["generation_config_json"]))
    fx["wave_f32"] = fx["wave"].astype(np.float32) / 32768.0
    fx["eos_row_f32"] = (fx["eos_row"].astype(np.uint32) << 16).view(np.float32)
    return fx


# ---- front-end -------------------------------------------------------------------------------------------------------------------
def hann(n=N_FFT, dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)).astype(dtype)


def slaney_filters(n_mels, n_fft=N_FFT, sr=16000):
    """[n_fft / 2 + 1][n_mels], Slaney scale and area normalisation."""
    def h2m(f):
        return 3.0 * f / 200.0 if f < 1000.0 else 15.0 + math.log(f / 1000.0) * 27.0 / math.log(6.4)

    def m2h(m):
        return 200.0 * m / 3.0 if m < 15.0 else 1000.0 * math.exp(math.log(6.4) / 27.0 * (m - 15.0))
    edges = np.array([m2h(m) for m in np.linspace(h2m(0.0), h2m(sr / 2.0), n_mels + 2)])
    freqs = np.linspace(0.0, sr // 2, n_fft // 2 + 1)
    fb = np.zeros((n_fft // 2 + 1, n_mels))
    for m in range(n_mels):
        lo, ce, hi = edges[m], edges[m + 1], edges[m + 2]
        up, down = (freqs - lo) / (ce - lo), (hi - freqs) / (hi - ce)
        fb[:, m] = np.maximum(0.0, np.minimum(up, down)) * 2.0 / (hi - lo)
    return fb


def power_frames(wav, length, T, dtype=np.float64):
    """[T][201] power spectrum of the frames the extractor keeps: the row cut / zero-padded to hop * T samples, samples at or
    beyond ``length`` zero, centred frames with reflect padding, periodic Hann.  ``dtype`` float32 evaluates the same formulas
    with a float32 direct DFT (the cross-check of the GPU test's bound).  Also returns sum |x w| per frame."""
    N = HOP * T
    row = np.zeros(N, dtype=np.float64)
    n = min(int(length), len(wav), N)
    row[:n] = np.asarray(wav[:n], dtype=np.float64)
    padded = np.pad(row, (N_FFT // 2, N_FFT // 2), mode="reflect")
    idx = np.arange(T)[:, None] * HOP + np.arange(N_FFT)[None, :]
    frames = (padded[idx].astype(dtype) * hann(dtype=dtype)[None, :]).astype(dtype)
    k = np.arange(N_FFT // 2 + 1)
    ang = 2.0 * np.pi * ((k[:, None] * np.arange(N_FFT)[None, :]) % N_FFT) / N_FFT
    c, s = np.cos(ang).astype(dtype), np.sin(ang).astype(dtype)
    if dtype == np.float32:                      # sequential float32 accumulation, as a direct DFT does
        re = np.zeros((T, len(k)), np.float32)
        im = np.zeros((T, len(k)), np.float32)
        for n_ in range(N_FFT):
            re += frames[:, n_:n_ + 1] * c[None, :, n_]
            im += frames[:, n_:n_ + 1] * s[None, :, n_]
    else:
        re, im = frames @ c.T, frames @ s.T
    return (re * re + im * im).astype(dtype), np.abs(frames).sum(1)


def log_mel(wav, length, T, fb, dtype=np.float64):
    """[T][n_mels]: the extractor's features, channels-last."""
    p, _ = power_frames(wav, length, T, dtype)
    mel = (p @ fb.astype(dtype)).astype(dtype)
    x = np.log10(np.maximum(mel, dtype(1e-10))).astype(dtype)
    x = np.maximum(x, x.max() - dtype(8.0))
    return ((x + dtype(4.0)) / dtype(4.0)).astype(dtype)


# ---- model -------------------------------------------------------------------------------------------------------------------------
def mm(a, b):
    """a @ b in float64 through torch's threaded GEMM (numpy's is several times slower at the full-width shapes)."""
    import torch
    return torch.matmul(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)),
                        torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64))).numpy()


def gelu(x):
    import torch
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x / math.sqrt(2.0)))).numpy())


def layer_norm(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


class Ref:
    def __init__(self, sd, cfg):
        self.sd = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
        self.cfg = cfg

    def w(self, name):
        return self.sd[name]

    def lin(self, x, pre, bias=True):
        y = mm(x, self.w(pre + ".weight").T)
        return y + self.w(pre + ".bias") if bias else y

    def ln(self, x, pre):
        return layer_norm(x, self.w(pre + ".weight"), self.w(pre + ".bias"))

    def attn(self, xq, xkv, pre, H, causal=False):
        D = xq.shape[-1]
        dk = D // H
        q = self.lin(xq, pre + ".q_proj") * dk ** -0.5
        k, v = self.lin(xkv, pre + ".k_proj", bias=False), self.lin(xkv, pre + ".v_proj")
        out = np.zeros_like(q)
        for h in range(H):
            sl = slice(h * dk, (h + 1) * dk)
            s = mm(q[:, sl], k[:, sl].T)
            if causal:
                s = np.where(np.tril(np.ones_like(s)) > 0, s, -np.inf)
            s = np.exp(s - s.max(-1, keepdims=True))
            out[:, sl] = mm(s / s.sum(-1, keepdims=True), v[:, sl])
        return self.lin(out, pre + ".out_proj")

    def conv(self, x, pre, stride):
        """x [T][Cin] -> [T / stride][Cout], kernel 3, padding 1."""
        w, b = self.w(pre + ".weight"), self.w(pre + ".bias")
        xp = np.pad(x, ((1, 1), (0, 0)))
        T = x.shape[0]
        y = sum(mm(xp[j:j + T], w[:, :, j].T) for j in range(3)) + b
        return y[::stride]

    def encoder(self, feats):
        """feats [T][n_mels] -> [T / 2][D]."""
        pre = "model.encoder"
        x = gelu(self.conv(feats, pre + ".conv1", 1))
        x = gelu(self.conv(x, pre + ".conv2", 2)) + self.w(pre + ".embed_positions.weight")
        for i in range(self.cfg["encoder_layers"]):
            lp = f"{pre}.layers.{i}"
            h = self.ln(x, lp + ".self_attn_layer_norm")
            x = x + self.attn(h, h, lp + ".self_attn", self.cfg["encoder_attention_heads"])
            h = self.ln(x, lp + ".final_layer_norm")
            x = x + self.lin(gelu(self.lin(h, lp + ".fc1")), lp + ".fc2")
        return self.ln(x, pre + ".layer_norm")

    def decoder_logits(self, enc, ids):
        """enc [Tp][D], ids [U] -> logits [U][V] (no cache: the whole prefix at once)."""
        pre = "model.decoder"
        ids = np.asarray(ids)
        H = self.cfg["decoder_attention_heads"]
        x = self.w(pre + ".embed_tokens.weight")[ids] + self.w(pre + ".embed_positions.weight")[:len(ids)]
        for i in range(self.cfg["decoder_layers"]):
            lp = f"{pre}.layers.{i}"
            h = self.ln(x, lp + ".self_attn_layer_norm")
            x = x + self.attn(h, h, lp + ".self_attn", H, causal=True)
            h = self.ln(x, lp + ".encoder_attn_layer_norm")
            x = x + self.attn(h, enc, lp + ".encoder_attn", H)
            h = self.ln(x, lp + ".final_layer_norm")
            x = x + self.lin(gelu(self.lin(h, lp + ".fc1")), lp + ".fc2")
        return mm(self.ln(x, pre + ".layer_norm"), self.w(pre + ".embed_tokens.weight").T)

    def greedy(self, enc, prompt, suppress, begin_suppress, eos, max_len):
        ids = list(prompt)
        while len(ids) < max_len:
            lg = self.decoder_logits(enc, ids)[-1].copy()
            lg[list(suppress)] = -np.inf
            if len(ids) == len(prompt):
                lg[list(begin_suppress)] = -np.inf
            ids.append(int(np.argmax(lg)))
            if ids[-1] == eos:
                break
        return ids


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
