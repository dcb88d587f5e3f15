#!/usr/bin/env python3
"""Yardstick for the UTMOS predictor (csrc/utmos.hip, f5e_tts_amd/eval/utmos.py) at utmos22_strong's sizes (wav2vec2-base,
BiLSTM 2 x 512, seeded synthetic weights), B = 1 at 5 s and 10 s of 16 kHz audio:
(a) ms per ``predict`` launched eagerly from Python (workspace and output given, nothing allocated) and replayed from a graph;
(b) f5e_lstm_f32 alone on the same buffers: ms, its share of the eager ``predict`` and us per time step (one launch each);
    f5e_w2v_conv0_gn (two launches) and f5e_score_mean alone as well;
(c) the same ``nn.LSTM`` run eagerly in fp32 on torch-ROCm over the same input -- a yardstick only, never on the product path --
    and the relative L2 between the two outputs.
Eager: HIP events around 5 calls after a warm one.  Graph: 10 launches per graph (f5e_graph_*), HIP events around 5 replays.
GPU box only:  python tools/utmos_time.py [--out profiles/utmos_time.txt]"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from f5e_tts_amd import ops  # noqa: E402
from f5e_tts_amd.eval.utmos import UTMOS22Strong  # noqa: E402
from tools.mas_time import LAUNCHES, REPLAYS, time_eager, time_graph  # noqa: E402
from tools.src_hash import csrc_sha256  # noqa: E402


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    ops.require_device()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = [f"# python tools/utmos_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# utmos22_strong sizes, synthetic weights, B = 1; eager: HIP events over 5 calls after a warm one; graph: ms per predict, "
             f"{LAUNCHES} per graph, HIP events over {REPLAYS} replays"]
    torch.manual_seed(4243)
    model = UTMOS22Strong().cuda()
    side = torch.cuda.Stream()
    for seconds in (5, 10):
        S = 16000 * seconds
        wav = (0.1 * torch.randn(1, S, generator=torch.Generator().manual_seed(seconds))).cuda()
        T = model.wav2vec2.frame_count(S)
        ws = torch.empty(model.workspace_bytes(1, S), dtype=torch.uint8, device="cuda")
        out = torch.empty(1, device="cuda")
        run = lambda: model.predict(wav, out=out, workspace=ws)   # noqa: E731
        eager_ms, _ = time_eager(run)
        graph_ms = time_graph(run, side)
        # the head's kernels alone, on the buffers predict has just filled
        hd, (plan, _total) = model._fold(), model._plan(1, S)
        f32 = ws.view(torch.float32)
        buf = lambda n: f32[plan[n][0]:plan[n][0] + math.prod(plan[n][1])].view(plan[n][1])   # noqa: E731
        hid, xg, lstm, cell, p1 = buf("hid"), buf("xg"), buf("lstm"), buf("cell"), buf("p1")
        lstm_ms, _ = time_eager(lambda: ops.lstm_f32(xg, hd["w_hh"], None, lstm, cell))
        both_ms, _ = time_eager(lambda: (ops.gemm_f32(hid.view(T, -1), hd["w_ih"], hd["b_ih"], out=xg),
                                         ops.lstm_f32(xg, hd["w_hh"], None, lstm, cell)))
        score_ms, _ = time_eager(lambda: ops.score_mean(p1, hd["w2"], hd["b2"], None, out, 1, scale=2.0, offset=3.0))
        C = model.wav2vec2.cfg.conv_dim[0]
        fd = model.wav2vec2._fold()
        c0out = torch.empty(1, (S - 10) // 5 + 1, C, device="cuda")
        part = torch.empty(ops.w2v_conv0_gn_partials(1, S, C), device="cuda")
        conv0_ms, _ = time_eager(lambda: ops.w2v_conv0_gn(wav, fd["conv"][0]["w"], None, fd["gn_g"], fd["gn_b"], None, c0out, part))
        # the yardstick: the same nn.LSTM on torch-ROCm over the same input
        x = torch.cat([hid, model.domain_emb.expand(1, T, -1), model.judge_emb.expand(1, T, -1)], -1)
        with torch.no_grad():
            torch_ms, (want, _) = time_eager(lambda: model.blstm(x))
        ops.lstm_f32(xg, hd["w_hh"], None, lstm, cell)
        err = rel_l2(lstm, want)
        for line in (
                f"predict B=1 {seconds} s (T = {T}, workspace {ws.numel() / 1e6:.0f} MB): eager {eager_ms:8.3f} ms, graph replay {graph_ms:8.3f} ms",
                f"  {seconds} s  f5e_lstm_f32 alone (T launches)   {lstm_ms:8.3f} ms = {100 * lstm_ms / eager_ms:5.1f} % of the eager predict, "
                f"{1e3 * lstm_ms / T:6.2f} us per step",
                f"  {seconds} s  nn.LSTM eager on torch-ROCm     {torch_ms:8.3f} ms = {torch_ms / both_ms:5.2f} x the input-projection GEMM + f5e_lstm_f32 "
                f"({both_ms:8.3f} ms); relative L2 of the two outputs {err:.1e}",
                f"  {seconds} s  f5e_w2v_conv0_gn alone (2 launches) {conv0_ms:8.3f} ms;  f5e_score_mean alone {score_ms:8.3f} ms"):
            lines.append(line)
            print(line, flush=True)
    if out_path:
        with open(os.path.join(ROOT, out_path) if not os.path.isabs(out_path) else out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
