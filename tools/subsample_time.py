#!/usr/bin/env python3
"""Yardstick for the 4x subsampling front (f5e_conv2d_sub_f32, csrc/subsample.hip): the second convolution of
Conv2dSubsampling4 -- Conv2d(256, 256, 3, 2) on the [B, T1, 39, 256] channels-last output of the first one (idim 80) -- at
10 s and 20 s of features (T = 1000 / 2000), batch 1 and 32, two arms:

  (a) the implicit GEMM: ``ops.conv2d_sub`` (no workspace);
  (b) the explicit one: the [M, K] = [B T2 19, 2304] patch matrix gathered into a scratch buffer (torch ``unfold`` +
      ``copy_``, built HERE only: the product has no such path) and ``ops.gemm_f32`` with the same weights and ReLU.

Per shape: microseconds (HIP events around 5 calls after a warm one), achieved fp32 TFLOP/s at 2 M 256 K FLOP, the scratch
bytes of (b), the largest difference between the arms, and the whole front (``ConformerEngine._subsample``: im2col, Toeplitz
GEMM, this convolution, the Linear, xscale) for scale.  No threshold: these are figures.
GPU box only:  python tools/subsample_time.py [--out profiles/subsample_time.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from f5e_tts_amd import ops  # noqa: E402
from tools.mas_time import time_eager  # noqa: E402
from tools.src_hash import csrc_sha256  # noqa: E402

C, IDIM, KS, STRIDE = 256, 80, 3, 2


def main():
    from f5e_tts_amd.ppg.ppg_model import ConformerPPG
    ops.require_device()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    torch.manual_seed(13)
    m = ConformerPPG(IDIM, 218, C, 4, 2048, 1, 15, global_cmvn=(torch.zeros(IDIM), torch.ones(IDIM)), ctc=True,
                     input_layer="conv2d4").cuda().eval()
    eng = m.engine()
    w, bias, _ = eng.sub_convs[0]
    w2d = w.view(C, -1)
    K = w2d.shape[1]
    lines = [f"# python tools/subsample_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# Conv2d({C}, {C}, {KS}, {STRIDE}) of the 4x front, idim {IDIM}, K = {K}; us per call, HIP events, 5 calls after a warm one"]
    gen = torch.Generator().manual_seed(14)
    for secs, B in ((10, 1), (20, 1), (10, 32), (20, 32)):
        T = 100 * secs
        T1, F1 = (T - 3) // 2 + 1, (IDIM - 3) // 2 + 1
        x = torch.randn(B, T1, F1, C, generator=gen).cuda()
        T2, F2 = (T1 - KS) // STRIDE + 1, (F1 - KS) // STRIDE + 1
        M = B * T2 * F2
        out_a = torch.empty(B, T2, F2, C, device="cuda")
        ms_a, _ = time_eager(lambda: ops.conv2d_sub(x, w, bias, STRIDE, out=out_a))
        scratch = torch.empty(B, T2, F2, KS, KS, C, device="cuda")
        patches = x.unfold(1, KS, STRIDE).unfold(2, KS, STRIDE).permute(0, 1, 2, 4, 5, 3)        # a view: [B, T2, F2, kt, kf, C]
        out_b = torch.empty(M, C, device="cuda")
        ms_g, _ = time_eager(lambda: scratch.copy_(patches))
        ms_m, _ = time_eager(lambda: ops.gemm_f32(scratch.view(M, K), w2d, bias, out=out_b, act=ops.ACT_RELU))
        diff = float((out_a.view(M, C) - out_b).abs().max())
        feats = torch.randn(B, T, IDIM, generator=gen).cuda()
        ms_f, _ = time_eager(lambda: eng._subsample(feats))
        flop = 2.0 * M * C * K
        lines.append(f"B={B:2d} {secs:2d} s (M={M:6d})  |  (a) implicit {ms_a * 1e3:9.1f} us {flop / ms_a / 1e9:6.2f} TFLOP/s, 0 B scratch"
                     f"  |  (b) gather {ms_g * 1e3:9.1f} us + gemm_f32 {ms_m * 1e3:9.1f} us = {(ms_g + ms_m) * 1e3:9.1f} us "
                     f"({flop / ms_m / 1e9:6.2f} TFLOP/s in the GEMM), scratch {scratch.numel() * 4} B  |  max |a - b| {diff:.2e}"
                     f"  |  whole front {ms_f * 1e3:9.1f} us")
        print(lines[-1], flush=True)
        del x, scratch, patches, out_a, out_b, feats
    if out_path:
        with open(os.path.join(ROOT, out_path) if not os.path.isabs(out_path) else out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
