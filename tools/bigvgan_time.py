"""BigVGAN decode timing (device events after warm-up) at the C2 shape (B = 1, 281 frames) and the C3 shape (B = 32,
938 frames), with synthetic weights (tools/synth.py).  Prints one JSON line per shape: ms per decode, mel-frames/s, and
the conv FLOP over the decode time as a fraction of the 2.5 PFLOP/s bf16 dense peak.  ``--yardstick`` adds the same
network as torch-ROCm ``F.conv1d`` in bf16 and fp32 (a yardstick only, never a product path).

    timeout -k 10 600 python tools/bigvgan_time.py [--shapes c2,c3] [--iters 10] [--yardstick]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16 = 2.5e15
SHAPES = {"c2": (1, 281), "c3": (32, 938)}


def conv_flop(cfg, B, T):
    """2 * MACs of every convolution (no padding, no activation work)."""
    C, L = cfg["upsample_initial_channel"], T
    f = 2 * B * L * cfg["num_mels"] * C * 7
    for u, k in zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"]):
        f += 2 * B * L * C * (C // 2) * k
        C, L = C // 2, L * u
        for kr, dils in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]):
            f += 2 * len(dils) * 2 * B * L * C * C * kr
    return f + 2 * B * L * C * 7


def _act_torch(x, p):
    C = x.shape[1]
    fu = p["fu"].to(x.dtype).view(1, 1, -1).expand(C, 1, -1)
    fd = p["fd"].to(x.dtype).view(1, 1, -1).expand(C, 1, -1)
    up = 2 * F.conv_transpose1d(F.pad(x, (5, 5), mode="replicate"), fu, stride=2, groups=C)[..., 15:-15]
    s = up + p["ib"].to(x.dtype).view(1, -1, 1) * torch.sin(up * p["a"].to(x.dtype).view(1, -1, 1)) ** 2
    return F.conv1d(F.pad(s, (5, 6), mode="replicate"), fd, stride=2, groups=C)


def torch_yardstick(W, cfg, mel, dtype):
    from f5e_tts_amd.vocoder_bigvgan import kaiser_sinc_filter1d
    g = lambda k: W[k].to(mel.device, dtype)  # noqa: E731
    filt = kaiser_sinc_filter1d().to(mel.device)

    def act(p):
        a, b = torch.exp(W[f"{p}.act.alpha"]), torch.exp(W[f"{p}.act.beta"])
        return dict(a=a.to(mel.device), ib=(1.0 / (b + 1e-9)).to(mel.device), fu=filt, fd=filt)

    x = F.conv1d(mel.to(dtype), g("conv_pre.weight"), g("conv_pre.bias"), padding=3)
    nk = len(cfg["resblock_kernel_sizes"])
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        x = F.conv_transpose1d(x, g(f"ups.{i}.0.weight"), g(f"ups.{i}.0.bias"), stride=u, padding=(k - u) // 2)
        xs = None
        for j, (kr, dils) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            r, xj = i * nk + j, x
            for m, d in enumerate(dils):
                t = _act_torch(xj, act(f"resblocks.{r}.activations.{2 * m}"))
                t = F.conv1d(t, g(f"resblocks.{r}.convs1.{m}.weight"), g(f"resblocks.{r}.convs1.{m}.bias"), dilation=d,
                             padding=(kr * d - d) // 2)
                t = _act_torch(t, act(f"resblocks.{r}.activations.{2 * m + 1}"))
                t = F.conv1d(t, g(f"resblocks.{r}.convs2.{m}.weight"), g(f"resblocks.{r}.convs2.{m}.bias"),
                             padding=(kr - 1) // 2)
                xj = xj + t
            xs = xj if xs is None else xs + xj
        x = xs / nk
    x = _act_torch(x, act("activation_post"))
    return torch.clamp(F.conv1d(x, g("conv_post.weight"), padding=3), -1.0, 1.0)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--yardstick", action="store_true")
    args = ap.parse_args()
    from f5e_tts_amd import ops
    from f5e_tts_amd.vocoder_bigvgan import BigVGAN, fold_state
    from tools import synth as SY

    ops.require_device()
    torch.cuda.set_device(0)
    cfg = SY.bigvgan_config()
    W = fold_state(SY.init_bigvgan_state(cfg), cfg)
    voc = BigVGAN(cfg, W).cuda().eval()
    for name in args.shapes.split(","):
        B, T = SHAPES[name]
        mel = SY.synthetic_mel(T, batch=B).cuda()
        flop = conv_flop(cfg, B, T)
        iters = args.iters if B == 1 else max(2, args.iters // 4)
        ms = timed(lambda: voc.decode(mel), args.warmup, iters)
        res = dict(tool="bigvgan_time", shape=name, B=B, frames=T, ms=round(ms, 3),
                   mel_frames_per_s=round(B * T / ms * 1e3, 1), conv_tflop=round(flop / 1e12, 3),
                   frac_bf16_peak=round(flop / (ms * 1e-3) / PEAK_BF16, 4))
        if args.yardstick:
            with torch.no_grad():
                for dt, tag in ((torch.bfloat16, "torch_bf16_ms"), (torch.float32, "torch_fp32_ms")):
                    res[tag] = round(timed(lambda: torch_yardstick(W, cfg, mel, dt), 1, max(2, iters // 2)), 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
