#!/usr/bin/env python3
"""Yardstick for Paraformer (csrc/paraformer.hip, f5e_tts_amd/eval/paraformer.py) at the full-size configuration
(paraformer-large: 50 encoder layers at 512, 16 decoder layers, V = 8404; seeded synthetic weights), B = 1 at 5 s and 10 s of
16 kHz audio:
(a) ms per ``generate`` launched eagerly from Python (workspace given; wall clock, it contains the one read-back of the token
    counts), and ms per front-end + encoder + predictor (``encode_predict``) eager and replayed from a graph;
(b) the CIF kernels alone (f5e_cif_alpha_f32 + f5e_cif_fire_f32, 3 launches) against copying alpha and h to the host, running the
    sequential loop there (NumPy, vectorised over the channels) and copying the frames back.
Eager: HIP events around 5 calls after a warm one.  Graph: 10 launches per graph (f5e_graph_*), HIP events around 5 replays.
GPU box only:  python tools/paraformer_time.py [--out profiles/paraformer_time.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from f5e_tts_amd import ops  # noqa: E402
from f5e_tts_amd.eval import paraformer as P  # noqa: E402
from tools.mas_time import LAUNCHES, REPLAYS, time_eager, time_graph, wall  # noqa: E402
from tools.src_hash import csrc_sha256  # noqa: E402


def host_cif(alpha_dev, h_dev):
    """The sequential loop on the host: device -> host copies, the loop in fp32, the frames copied back."""
    alpha, h = alpha_dev.cpu().numpy()[0], h_dev.cpu().numpy()[0]
    h = np.concatenate([h, np.zeros((1, h.shape[1]), np.float32)])
    integrate, frame, out = np.float32(0), np.zeros(h.shape[1], np.float32), []
    for t in range(alpha.shape[0]):
        comp = np.float32(1) - integrate
        integrate = integrate + alpha[t]
        fire = integrate >= np.float32(1)
        if fire:
            integrate = integrate - np.float32(1)
        cur = comp if fire else alpha[t]
        frame = frame + cur * h[t]
        if fire:
            out.append(frame)
            frame = (alpha[t] - cur) * h[t]
    return torch.from_numpy(np.stack(out) if out else np.zeros((0, h.shape[1]), np.float32)).cuda()


def main():
    ops.require_device()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = [f"# python tools/paraformer_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# paraformer-large sizes, seeded synthetic weights, B = 1; generate: wall ms, best of 5 after a warm call; eager: HIP "
             f"events over 5 calls after a warm one; graph: {LAUNCHES} per graph, HIP events over {REPLAYS} replays"]
    cfg = P.ParaformerConfig()
    model = P.Paraformer(cfg)
    model.load_funasr_state(P.seeded_state_dict(cfg, 4244))
    model = model.cuda().eval()
    side = torch.cuda.Stream()
    for seconds in (5, 10):
        S = 16000 * seconds
        g = torch.Generator().manual_seed(seconds)
        wav = (0.1 * torch.randn(1, S, generator=g) + 0.2 * torch.sin(torch.arange(S) * (2 * np.pi * 180 / 16000))).cuda()
        lens = torch.tensor([S], dtype=torch.int32).cuda()
        T, Tp = model.frames_of(S)
        ws = torch.empty(model.workspace_bytes(1, S), dtype=torch.uint8, device="cuda")
        tokens, n_tok, _ = model.generate(wav, lens, workspace=ws)
        gen_ms = min(wall(lambda: model.generate(wav, lens, workspace=ws))[0] for _ in range(5))
        front = lambda: model.encode_predict(wav, lens, workspace=ws)   # noqa: E731
        eager_ms, (_, frames, enc, embeds, n, alpha) = time_eager(front)
        graph_ms = time_graph(front, side)
        # the CIF kernels alone on the buffers the pass has just filled, against the host loop
        logit = torch.logit(alpha[:, :Tp].clamp(1e-6, 1 - 1e-6)).contiguous()
        a2, n2, cnt = torch.empty_like(alpha), torch.empty_like(n), torch.empty_like(n)
        out = torch.empty_like(embeds)
        scratch = torch.empty(ops.cif_fire_scratch(1, Tp, Tp + 1), device="cuda")
        cif_ms, _ = time_eager(lambda: (ops.cif_alpha(logit, frames, a2, n2, cfg.smooth_factor, cfg.noise_threshold, cfg.tail_threshold),
                                        ops.cif_fire(a2, enc.view(Tp, -1), frames, out, cnt, scratch, n_limit=n2)))
        host_ms = min(wall(lambda: host_cif(a2, enc))[0] for _ in range(3))
        same = torch.equal(host_cif(a2, enc)[: int(n2)], out[0, : int(n2)])
        for line in (
                f"generate B=1 {seconds} s (T' = {Tp}, {int(n)} tokens, {int(n_tok)} ids kept, workspace {ws.numel() / 1e6:.0f} MB): eager {gen_ms:8.3f} ms wall",
                f"  {seconds} s  front-end + encoder + predictor: eager {eager_ms:8.3f} ms, graph replay {graph_ms:8.3f} ms",
                f"  {seconds} s  f5e_cif_alpha_f32 + f5e_cif_fire_f32 (3 launches) {cif_ms:8.3f} ms;  alpha and h to the host, the loop there, "
                f"frames back {host_ms:8.3f} ms = {host_ms / cif_ms:6.1f} x; frames bit-identical: {same}"):
            lines.append(line)
            print(line, flush=True)
    if out_path:
        with open(os.path.join(ROOT, out_path) if not os.path.isabs(out_path) else out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
