"""BigVGAN-v2 mel vocoder on libf5e_hip.so (``--vocoder_name bigvgan``, reference infer/utils_infer.py:125-138,488-491).

The reference loads the third-party ``bigvgan`` package, which is not in the tree; this is a restatement of the published
BigVGAN-v2 generator (``resblock "1"``, anti-aliased SnakeBeta), the contract the kernels implement:

- ``conv_pre``: Conv1d(num_mels -> C0, k7, pad 3), C0 = ``upsample_initial_channel``.
- stage i (``upsample_rates`` u_i, ``upsample_kernel_sizes`` k_i): ``ups[i][0]`` ConvTranspose1d(C -> C/2, k_i, stride u_i,
  pad (k_i - u_i)/2); then the mean of ``len(resblock_kernel_sizes)`` AMPBlock1(C/2, k, dilations) outputs, each
  ``for m: t = A_2m(x); t = convs1[m](t) (dilation d_m, pad (k d_m - d_m)/2); t = A_2m+1(t); t = convs2[m](t); x = x + t``.
- ``activation_post`` (Activation1d), ``conv_post`` Conv1d(C -> 1, k7, pad 3, bias iff ``use_bias_at_final``), then
  ``tanh`` if ``use_tanh_at_final`` else ``clamp(-1, 1)``.  Output ``[B, 1, prod(u) * T]``.
- Activation1d: 2x upsample (replicate-pad 5, 2 * conv_transpose1d(stride 2, 12-tap filter), crop [15:-15]), SnakeBeta
  ``u + sin^2(alpha u) / (beta + 1e-9)`` (alpha = exp(alpha), beta = exp(beta) if ``snake_logscale``; plain snake uses
  beta = alpha), 2x downsample (replicate-pad (5, 6), stride-2 conv1d).  Filter: kaiser-windowed sinc, cutoff 0.25,
  half-width 0.3, 12 taps, normalised to sum 1 -- or the checkpoint's ``upsample.filter`` / ``downsample.lowpass.filter``.
- Weight norm is folded at load: ``w = g v / ||v||`` with the norm over every dim but 0 (``weight_g`` / ``weight_v`` or
  ``parametrizations.weight.original0`` / ``original1``; plain ``weight`` is accepted as already folded).

Precision: conv operands are bf16 (MFMA, fp32 accumulation); the residual stream, the stage sums, the activations' inputs
and conv_post are fp32.  Arithmetic is "parity unpinned" against the package (no golden vectors exist); tests compare
with an fp32 restatement (DESIGN.md "BigVGAN").  Layout: channels-last [B][L][C] throughout."""
from __future__ import annotations

import json
import math
import os
from typing import Dict, Optional

import torch
from torch import nn

from . import _C, ops

F32, BF = torch.float32, torch.bfloat16

DEFAULT_CONFIG = dict(num_mels=100, upsample_initial_channel=1536, upsample_rates=[4, 4, 2, 2, 2, 2],
                      upsample_kernel_sizes=[8, 8, 4, 4, 4, 4], resblock="1", resblock_kernel_sizes=[3, 7, 11],
                      resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], activation="snakebeta",
                      snake_logscale=True, use_tanh_at_final=False, use_bias_at_final=False, sampling_rate=24000)


def kaiser_sinc_filter1d(cutoff: float = 0.25, half_width: float = 0.3, kernel_size: int = 12) -> torch.Tensor:
    """The anti-alias low-pass of Activation1d (even kernel_size), built in float64 -> float32 [kernel_size]."""
    half = kernel_size // 2
    A = 2.285 * (half - 1) * math.pi * (4 * half_width) + 7.95
    if A > 50.0:
        beta = 0.1102 * (A - 8.7)
    elif A >= 21.0:
        beta = 0.5842 * (A - 21) ** 0.4 + 0.07886 * (A - 21.0)
    else:
        beta = 0.0
    window = torch.kaiser_window(kernel_size, periodic=False, beta=beta, dtype=torch.float64)
    time = torch.arange(-half, half, dtype=torch.float64) + 0.5
    f = 2 * cutoff * window * torch.sinc(2 * cutoff * time)
    return (f / f.sum()).to(F32)


def fold_weight_norm(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """torch weight_norm(dim=0): g v / ||v|| with the norm over every dim but 0 (per input channel for ConvTranspose1d)."""
    v = v.to(F32)
    norm = v.flatten(1).norm(dim=1).view(-1, *([1] * (v.ndim - 1)))
    return g.to(F32) * v / norm


def _check_config(h: dict) -> dict:
    cfg = dict(DEFAULT_CONFIG)
    cfg.update(h)
    if str(cfg["resblock"]) != "1":
        raise _C.F5EError(f"BigVGAN resblock {cfg['resblock']!r} is not built (only AMPBlock1, resblock \"1\")")
    if cfg["activation"] not in ("snake", "snakebeta"):
        raise _C.F5EError(f"unknown BigVGAN activation {cfg['activation']!r} (snake / snakebeta)")
    if len(cfg["upsample_rates"]) != len(cfg["upsample_kernel_sizes"]):
        raise _C.F5EError("upsample_rates / upsample_kernel_sizes differ in length")
    for u, k in zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"]):
        if (k - u) % 2 or k < u or k > 3 * u:
            raise _C.F5EError(f"ConvTranspose1d(k={k}, stride={u}) needs k - u even and u <= k <= 3u")
    if len(cfg["resblock_dilation_sizes"]) != len(cfg["resblock_kernel_sizes"]):
        raise _C.F5EError("resblock_dilation_sizes / resblock_kernel_sizes differ in length")
    c_last = cfg["upsample_initial_channel"] >> len(cfg["upsample_rates"])
    if c_last < 1 or c_last % 4 or cfg["upsample_initial_channel"] % (1 << len(cfg["upsample_rates"])) or cfg["num_mels"] % 4:
        raise _C.F5EError("the conv kernel needs every channel count (and num_mels) to be a multiple of 4")
    return cfg


def _conv_names(cfg: dict):
    """(canonical conv prefix, has_bias) of every weight-normed conv, and activation prefixes, in network order."""
    convs = [("conv_pre", True)]
    acts = []
    nk = len(cfg["resblock_kernel_sizes"])
    for i in range(len(cfg["upsample_rates"])):
        convs.append((f"ups.{i}.0", True))
        for j, dil in enumerate(cfg["resblock_dilation_sizes"]):
            r = i * nk + j
            for m in range(len(dil)):
                convs += [(f"resblocks.{r}.convs1.{m}", True), (f"resblocks.{r}.convs2.{m}", True)]
            acts += [f"resblocks.{r}.activations.{n}" for n in range(2 * len(dil))]
    acts.append("activation_post")
    convs.append(("conv_post", bool(cfg["use_bias_at_final"])))
    return convs, acts


def fold_state(state: Dict[str, torch.Tensor], cfg: dict) -> Dict[str, torch.Tensor]:
    """Generator state dict (either weight-norm key form) -> {canonical name: fp32 tensor}; missing or extra keys raise."""
    cfg = _check_config(cfg)
    src = dict(state)
    out: Dict[str, torch.Tensor] = {}
    missing = []

    def take(k):
        if k not in src:
            missing.append(k)
            return None
        return src.pop(k)

    convs, acts = _conv_names(cfg)
    for p, has_bias in convs:
        if f"{p}.weight_g" in src or f"{p}.weight_v" in src:
            g, v = take(f"{p}.weight_g"), take(f"{p}.weight_v")
            w = fold_weight_norm(g, v) if g is not None and v is not None else None
        elif f"{p}.parametrizations.weight.original0" in src or f"{p}.parametrizations.weight.original1" in src:
            g, v = take(f"{p}.parametrizations.weight.original0"), take(f"{p}.parametrizations.weight.original1")
            w = fold_weight_norm(g, v) if g is not None and v is not None else None
        else:
            w = take(f"{p}.weight")
            w = w.to(F32) if w is not None else None
        if w is not None:
            out[f"{p}.weight"] = w
        if has_bias:
            b = take(f"{p}.bias")
            if b is not None:
                out[f"{p}.bias"] = b.to(F32)
    for p in acts:
        a = take(f"{p}.act.alpha")
        if a is not None:
            out[f"{p}.act.alpha"] = a.to(F32).flatten()
        if cfg["activation"] == "snakebeta":
            b = take(f"{p}.act.beta")
            if b is not None:
                out[f"{p}.act.beta"] = b.to(F32).flatten()
        for fk in ("upsample.filter", "downsample.lowpass.filter"):   # optional buffers
            if f"{p}.{fk}" in src:
                out[f"{p}.{fk}"] = src.pop(f"{p}.{fk}").to(F32).flatten()
    if missing or src:
        raise _C.F5EError(f"BigVGAN state dict mismatch: missing {sorted(missing)[:8]}{'...' if len(missing) > 8 else ''}, "
                          f"unexpected {sorted(src)[:8]}{'...' if len(src) > 8 else ''}")
    return out


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """Conv1d weight [N][Cin][k] -> bf16 [roundup(N, 64)][k][roundup(Cin, 32)] (f5e_bigvgan_conv), zero-padded."""
    N, Cin, k = w.shape
    n_pad, c_pad = (N + 63) // 64 * 64, (Cin + 31) // 32 * 32
    p = torch.zeros(n_pad, k, c_pad, dtype=F32, device=w.device)
    p[:N, :, :Cin] = w.to(F32).permute(0, 2, 1)
    return p.reshape(n_pad, k * c_pad).to(BF).contiguous()


def transposed_as_conv3(w: torch.Tensor, b: torch.Tensor, u: int):
    """ConvTranspose1d(stride u, k, pad (k - u)/2) weight [Cin][Cout][k] -> the equivalent polyphase 3-tap Conv1d weight
    [u * Cout][Cin][3] (pad 1) and bias [u * Cout]: output row q, column r Cout + co is sample q u + r, channel co, i.e. the
    [L][u Cout] result is the [L u][Cout] output.  Phase r, tap j reads input q - 1 + j through kernel index
    r + p + (1 - j) u (the taps whose index falls outside [0, k) are zero)."""
    Cin, Cout, k = w.shape
    p = (k - u) // 2
    w3 = torch.zeros(u, Cout, Cin, 3, dtype=w.dtype, device=w.device)
    for r in range(u):
        for j in range(3):
            kk = r + p + (1 - j) * u
            if 0 <= kk < k:
                w3[r, :, :, j] = w[:, :, kk].t()
    return w3.reshape(u * Cout, Cin, 3), b.to(w.dtype).repeat(u)


class BigVGAN(nn.Module):
    """Folded fp32 weights (buffers) + the HIP decode.  ``BigVGAN(cfg, folded)``; see ``load_bigvgan``."""

    def __init__(self, cfg: dict, folded: Dict[str, torch.Tensor]):
        super().__init__()
        self.h = _check_config(cfg)
        self._names = {}
        for k, v in folded.items():
            bn = k.replace(".", "__")
            self._names[k] = bn
            self.register_buffer(bn, v.detach().to(F32).contiguous())
        self._packed = None

    def w(self, name: str) -> Optional[torch.Tensor]:
        bn = self._names.get(name)
        return getattr(self, bn) if bn is not None else None

    def _act(self, p: str, dv):
        a = self.w(f"{p}.act.alpha")
        b = self.w(f"{p}.act.beta") if self.h["activation"] == "snakebeta" else a
        if self.h["snake_logscale"]:
            a, b = torch.exp(a), torch.exp(b)
        inv_b = 1.0 / (b + 1e-9)
        default = kaiser_sinc_filter1d()
        fu = self.w(f"{p}.upsample.filter")
        fd = self.w(f"{p}.downsample.lowpass.filter")
        fu = default if fu is None else fu
        fd = default if fd is None else fd
        f = lambda t: t.detach().to(dv, F32).contiguous()  # noqa: E731
        return dict(alpha=f(a), inv_beta=f(inv_b), f_up=f(fu), f_dn=f(fd))

    def _pack(self, dv):
        sig = tuple((t.data_ptr(), t._version) for t in self.buffers()) + (str(dv),)
        if self._packed is not None and self._packed[0] == sig:
            return self._packed[1]
        h = self.h
        f = lambda t: t.detach().to(dv, F32).contiguous()  # noqa: E731
        W = self.w
        P = dict(pre=dict(w=pack_conv_weight(W("conv_pre.weight").to(dv)), b=f(W("conv_pre.bias"))), stages=[])
        nk = len(h["resblock_kernel_sizes"])
        for i, u in enumerate(h["upsample_rates"]):
            w3, b3 = transposed_as_conv3(W(f"ups.{i}.0.weight").to(dv), W(f"ups.{i}.0.bias").to(dv), u)
            blocks = []
            for j, (k, dils) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
                r = i * nk + j
                layers = []
                for m, d in enumerate(dils):
                    layers.append(dict(
                        d=d, w1=pack_conv_weight(W(f"resblocks.{r}.convs1.{m}.weight").to(dv)),
                        b1=f(W(f"resblocks.{r}.convs1.{m}.bias")),
                        w2=pack_conv_weight(W(f"resblocks.{r}.convs2.{m}.weight").to(dv)),
                        b2=f(W(f"resblocks.{r}.convs2.{m}.bias")),
                        a1=self._act(f"resblocks.{r}.activations.{2 * m}", dv),
                        a2=self._act(f"resblocks.{r}.activations.{2 * m + 1}", dv)))
                blocks.append(dict(k=k, layers=layers))
            P["stages"].append(dict(u=u, w=pack_conv_weight(w3), b=f(b3), blocks=blocks))
        pw = W("conv_post.weight")
        pb = W("conv_post.bias")
        P["post"] = dict(w=f(pw[0].t()), b=f(pb) if pb is not None else None, act=self._act("activation_post", dv))
        self._packed = (sig, P)
        return P

    @torch.no_grad()
    def decode(self, mel: torch.Tensor) -> torch.Tensor:
        """mel [b, num_mels, t] on the GPU -> wav [b, 1, prod(upsample_rates) * t] fp32."""
        ops.require_device()
        if mel.ndim != 3 or mel.shape[1] != self.h["num_mels"]:
            raise _C.F5EError(f"BigVGAN.decode expects [b, {self.h['num_mels']}, t] (got {tuple(mel.shape)})")
        dv = mel.device
        P = self._pack(dv)
        B, n_mels, T = mel.shape
        C0 = self.h["upsample_initial_channel"]
        sizes = [C0 * T]
        L, C = T, C0
        for u in self.h["upsample_rates"]:
            L, C = L * u, C // 2
            sizes.append(L * C)
        n = B * max(sizes)
        # workspace from the caching allocator on the caller's stream (graph-capturable, re-entrant per stream)
        S, X0, XB, TT = (torch.empty(n, device=dv) for _ in range(4))
        A = torch.empty(n, device=dv, dtype=BF)
        x = mel.to(F32).transpose(1, 2).contiguous()
        xb = torch.empty(B, T, n_mels, device=dv, dtype=BF)
        ops.cast_bf16(x, xb)

        def v(buf, L_, C_):
            return buf[:B * L_ * C_].view(B, L_, C_)

        ops.bigvgan_conv(xb, P["pre"]["w"], P["pre"]["b"], C0, 7, 1, 3, out=v(S, T, C0))
        L, C = T, C0
        for st in P["stages"]:
            u, Co = st["u"], C // 2
            ops.cast_bf16(v(S, L, C), v(A, L, C))
            ops.bigvgan_conv(v(A, L, C), st["w"], st["b"], u * Co, 3, 1, 1, out=v(X0, L, u * Co))
            L, C = L * u, Co
            nb = len(st["blocks"])
            for j, blk in enumerate(st["blocks"]):
                k = blk["k"]
                for m, ly in enumerate(blk["layers"]):
                    cur = v(X0 if m == 0 else XB, L, C)
                    a = ly["a1"]
                    ops.bigvgan_act(cur, v(A, L, C), a["alpha"], a["inv_beta"], a["f_up"], a["f_dn"])
                    ops.bigvgan_conv(v(A, L, C), ly["w1"], ly["b1"], C, k, ly["d"], (k * ly["d"] - ly["d"]) // 2,
                                     out=v(TT, L, C))
                    a = ly["a2"]
                    ops.bigvgan_act(v(TT, L, C), v(A, L, C), a["alpha"], a["inv_beta"], a["f_up"], a["f_dn"])
                    if m + 1 < len(blk["layers"]):
                        ops.bigvgan_conv(v(A, L, C), ly["w2"], ly["b2"], C, k, 1, (k - 1) // 2, resid=cur,
                                         out=v(XB, L, C))
                    else:   # last layer of the block: x + t goes straight into the stage mean
                        ops.bigvgan_conv(v(A, L, C), ly["w2"], ly["b2"], C, k, 1, (k - 1) // 2, resid=cur,
                                         sum_=v(S, L, C), sum_scale=1.0 / nb, sum_init=(j == 0))
        a = P["post"]["act"]
        ops.bigvgan_act(v(S, L, C), v(TT, L, C), a["alpha"], a["inv_beta"], a["f_up"], a["f_dn"])
        wav = torch.empty(B, 1, L, device=dv)
        ops.bigvgan_post(v(TT, L, C), P["post"]["w"], P["post"]["b"], wav.view(B, L), bool(self.h["use_tanh_at_final"]))
        return wav

    def forward(self, mel):
        return self.decode(mel)


def load_bigvgan(local_path: Optional[str], device="cpu") -> BigVGAN:
    """``config.json`` + ``bigvgan_generator.pt`` ({"generator": state_dict}) from a local BigVGAN-v2 directory (the
    reference's is_local branch, infer/utils_infer.py:125-138).  There is no network: a missing directory is an error."""
    if not local_path or not os.path.isdir(local_path):
        raise FileNotFoundError(f"local BigVGAN checkpoint directory not found: {local_path!r} (no network access)")
    with open(os.path.join(local_path, "config.json"), "r") as f:
        cfg = json.load(f)
    ckpt = torch.load(os.path.join(local_path, "bigvgan_generator.pt"), map_location="cpu", weights_only=True)
    state = ckpt["generator"] if isinstance(ckpt, dict) and "generator" in ckpt else ckpt
    return BigVGAN(cfg, fold_state(state, cfg)).eval().to(device)
