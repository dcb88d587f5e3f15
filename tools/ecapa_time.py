#!/usr/bin/env python3
"""Yardstick for the ECAPA-TDNN speaker encoder (csrc/ecapa.hip, f5e_tts_amd/eval/ecapa_tdnn.py).
(a) a full-size forward (feat_dim 1024, 25 layers, channels 512, emb 256; synthetic weights) at T = 250 and 500 frames (5 and
    10 s of audio), B = 1 and a ragged B = 2 (lengths T and 0.6 T): ms per forward replayed from a graph (workspace and output
    given, so nothing is allocated), ms per forward launched eagerly from Python (wall clock, the launches' host cost
    included), against the restated module (tests/ecapa_ref.py) run eagerly on torch-ROCm, and the relative L2 between them.
(b) the Res2 chain of one block (w = 64, dilation 3): the single launch of f5e_res2_dconv against seven launches of one step
    each (the same kernel and arithmetic, no halo recomputed).
(c) f5e_layer_mix_inorm at L = 25, F = 1024, T = 500 (51 MB of hidden states): ms and achieved GB/s (bytes read + written over
    time) with every launch of the graph reading ANOTHER 51 MB buffer (10 buffers, 512 MB: more than the 256 MiB memory-side
    cache holds, so the reads come from HBM), and with one buffer read again and again (cache resident), against the 6.3 TB/s
    the HBM of an MI355X achieves (8 TB/s peak).
Kernels: 10 launches per graph (f5e_graph_*), HIP events around 5 replays.  Eager: HIP events around 5 calls.
GPU box only:  python tools/ecapa_time.py [--out profiles/ecapa_time.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from f5e_tts_amd import ops  # noqa: E402
from f5e_tts_amd.eval.ecapa_tdnn import ECAPA_TDNN_SMALL  # noqa: E402
from tools.mas_time import LAUNCHES, REPLAYS, time_eager, time_graph  # noqa: E402
from tools.src_hash import csrc_sha256  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ecapa_ref as ER  # noqa: E402

I32 = torch.int32
HBM_ACHIEVABLE_TBS = 6.3


def forward_lines():
    cfg = ER.make_cfg(1024, 512, 256, False, 25)
    sd = ER.synth_state_dict(cfg, 4101)
    model = ECAPA_TDNN_SMALL(1024)
    model.load_state_dict(sd)
    model.cuda()
    sd_dev = {k: v.cuda() for k, v in sd.items()}
    side, out = torch.cuda.Stream(), []
    for T in (250, 500):
        for lengths in ([T], [T, int(0.6 * T)]):
            B = len(lengths)
            hs = ER.synth_hidden_states(4102 + T, 25, B, T, 1024).cuda()
            ln = torch.tensor(lengths, dtype=I32).cuda()
            ws = torch.empty(model.workspace_bytes(B, T), dtype=torch.uint8, device="cuda")
            emb = torch.empty(B, 256, device="cuda")
            graph_ms = time_graph(lambda: model(hs, ln, workspace=ws, out=emb), side)
            eager_ms, got = time_eager(lambda: model(hs, ln, workspace=ws, out=emb))
            torch_ms, want = time_eager(lambda: ER.forward(sd_dev, cfg, hs, ln)["emb"])
            err = ER.rel_l2(got.cpu(), want.cpu())
            out.append(f"forward B={B} T={T} lengths {lengths} ({hs.numel() * 4 / 1e6:.1f} MB of hidden states): graph replay "
                       f"{graph_ms:7.3f} ms, eager launches {eager_ms:7.3f} ms  |  restated module, eager torch-ROCm "
                       f"{torch_ms:7.3f} ms = {torch_ms / graph_ms:5.1f} x the replay, {torch_ms / eager_ms:5.1f} x the eager "
                       f"launches;  relative L2 of the embeddings {err:.1e}")
            print(out[-1], flush=True)
    return out


def res2_lines():
    side, out, w, d = torch.cuda.Stream(), [], 64, 3
    wt = ER.hash_tensor(5, 1, (7, w, 3 * w), -0.125, 0.125).cuda()
    bias, scale, shift = (ER.hash_tensor(5, k, (7, w), lo, hi).cuda() for k, lo, hi in ((2, -0.1, 0.1), (3, 0.5, 1.5), (4, -0.3, 0.3)))
    for B, T in ((1, 250), (1, 500), (2, 500)):
        x = ER.hash_tensor(6, T, (B, T, 8 * w), -1.0, 1.0).cuda()
        y1, y7 = torch.empty_like(x), torch.empty_like(x)
        one = time_graph(lambda: ops.res2_dconv(x, y1, wt, bias, scale, shift, None, d), side)

        def seven():
            for i in range(7):
                ops.res2_dconv(x, y7, wt, bias, scale, shift, None, d, i, 1)
        sev = time_graph(seven, side)
        torch.cuda.synchronize()
        out.append(f"res2 chain w={w} d={d} B={B} T={T}: one launch {one:7.4f} ms  |  seven launches of one step {sev:7.4f} ms "
                   f"= {sev / one:4.2f} x;  same bits: {bool(torch.equal(y1, y7))}")
        print(out[-1], flush=True)
    return out


def layer_mix_lines():
    side, Lm, T, Fd = torch.cuda.Stream(), 25, 500, 1024
    fw = ER.hash_tensor(7, 1, (Lm,), -1.0, 1.0).cuda()
    bufs = [torch.randn(Lm, 1, T, Fd, device="cuda") for _ in range(LAUNCHES)]
    x, mask = torch.empty(1, T, Fd, device="cuda"), torch.empty(1, T, device="cuda")
    nbytes = (Lm + 3) * T * Fd * 4          # hidden states read once; x written, then read and rewritten by the norm
    turn = [0]

    def rotating():
        ops.layer_mix_inorm(bufs[turn[0] % LAUNCHES], fw, None, x, mask)
        turn[0] += 1
    turn[0] = 1                              # time_graph warms with one call, then captures LAUNCHES: one per buffer
    cold = time_graph(rotating, side)
    warm = time_graph(lambda: ops.layer_mix_inorm(bufs[0], fw, None, x, mask), side)
    line = (f"layer mix + instance norm L={Lm} F={Fd} T={T} ({Lm * T * Fd * 4 / 1e6:.1f} MB read once, {nbytes / 1e6:.1f} MB moved): "
            f"from HBM (10 buffers in turn) {cold:7.4f} ms = {nbytes / cold / 1e6:6.0f} GB/s = "
            f"{100 * nbytes / cold / 1e9 / HBM_ACHIEVABLE_TBS:4.1f} % of {HBM_ACHIEVABLE_TBS} TB/s  |  one buffer again and again "
            f"(cache resident) {warm:7.4f} ms = {nbytes / warm / 1e6:6.0f} GB/s")
    print(line, flush=True)
    return [line]


def main():
    ops.require_device()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = [f"# python tools/ecapa_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# graph: ms per forward / launch, {LAUNCHES} per graph, HIP events over {REPLAYS} replays; eager: HIP events over 5 calls"]
    lines += forward_lines()
    lines += res2_lines()
    lines += layer_mix_lines()
    if out_path:
        with open(os.path.join(ROOT, out_path) if not os.path.isabs(out_path) else out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
