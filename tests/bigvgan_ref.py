"""fp32 restatement of the BigVGAN-v2 generator (channels-first torch ops, the published module structure) that the
BigVGAN tests compare the HIP path with.  Test code only: the product never imports it.  ``bf16=True`` rounds the conv
operands to bf16 exactly where the kernels do (conv inputs and weights; conv_post stays fp32)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from f5e_tts_amd.vocoder_bigvgan import DEFAULT_CONFIG, kaiser_sinc_filter1d


def _r(t, bf16):
    return t.to(torch.bfloat16).float() if bf16 else t


def activation1d(x, alpha, beta, f_up, f_dn, logscale=True):
    """Activation1d(SnakeBeta): x [B, C, L] fp32; alpha / beta the raw per-channel parameters."""
    C = x.shape[1]
    a = torch.exp(alpha) if logscale else alpha
    b = torch.exp(beta) if logscale else beta
    xp = F.pad(x, (5, 5), mode="replicate")
    up = 2 * F.conv_transpose1d(xp, f_up.view(1, 1, -1).expand(C, 1, -1), stride=2, groups=C)
    up = up[..., 15:-15]
    s = up + (1.0 / (b + 1e-9)).view(1, -1, 1) * torch.sin(up * a.view(1, -1, 1)) ** 2
    sp = F.pad(s, (5, 6), mode="replicate")
    return F.conv1d(sp, f_dn.view(1, 1, -1).expand(C, 1, -1), stride=2, groups=C)


def act_params(W, cfg, p):
    alpha = W[f"{p}.act.alpha"]
    beta = W[f"{p}.act.beta"] if cfg["activation"] == "snakebeta" else alpha
    f = kaiser_sinc_filter1d()
    return alpha, beta, W.get(f"{p}.upsample.filter", f), W.get(f"{p}.downsample.lowpass.filter", f)


def generator(W, cfg, mel, bf16=False):
    """W: folded fp32 weights (vocoder_bigvgan.fold_state); mel [B, num_mels, T] -> wav [B, 1, 256 T]."""
    h = dict(DEFAULT_CONFIG)
    h.update(cfg)
    ls = h["snake_logscale"]
    x = F.conv1d(_r(mel.float(), bf16), _r(W["conv_pre.weight"], bf16), W["conv_pre.bias"], padding=3)
    nk = len(h["resblock_kernel_sizes"])
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        x = F.conv_transpose1d(_r(x, bf16), _r(W[f"ups.{i}.0.weight"], bf16), W[f"ups.{i}.0.bias"], stride=u,
                               padding=(k - u) // 2)
        xs = None
        for j, (kr, dils) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            r = i * nk + j
            xj = x
            for m, d in enumerate(dils):
                t = activation1d(xj, *act_params(W, h, f"resblocks.{r}.activations.{2 * m}"), logscale=ls)
                t = F.conv1d(_r(t, bf16), _r(W[f"resblocks.{r}.convs1.{m}.weight"], bf16),
                             W[f"resblocks.{r}.convs1.{m}.bias"], dilation=d, padding=(kr * d - d) // 2)
                t = activation1d(t, *act_params(W, h, f"resblocks.{r}.activations.{2 * m + 1}"), logscale=ls)
                t = F.conv1d(_r(t, bf16), _r(W[f"resblocks.{r}.convs2.{m}.weight"], bf16),
                             W[f"resblocks.{r}.convs2.{m}.bias"], padding=(kr - 1) // 2)
                xj = xj + t
            xs = xj if xs is None else xs + xj
        x = xs / nk
    x = activation1d(x, *act_params(W, h, "activation_post"), logscale=ls)
    x = F.conv1d(x, W["conv_post.weight"], W.get("conv_post.bias"), padding=3)
    return torch.tanh(x) if h["use_tanh_at_final"] else torch.clamp(x, -1.0, 1.0)
