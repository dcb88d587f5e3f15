#!/usr/bin/env python3
"""Yardstick for the WavLM upstream (csrc/wavlm.hip, f5e_relbias_attn_f32, f5e_tts_amd/eval/wavlm.py) at the full-size
configuration (WavLM-large, seeded synthetic weights), a ragged B = 2 (lengths S and 0.6 S) at 5 s and 10 s of 16 kHz audio:
(a) ms per ``extract`` replayed from a graph (workspace and output given, nothing allocated) and launched eagerly from Python;
(b) the share of each kernel class: every op of one eager ``extract`` between its own pair of HIP events (the GEMMs split by
    their N and K), summed by class over 3 runs after a warm one;
(c) the GB/s of f5e_wavlm_conv0 (samples read + frames written over its time in (b));
(d) the restated module (tests/wavlm_ref.py) run eagerly in fp32 on torch-ROCm -- a yardstick only, never on the product path --
    and the relative L2 between the two.
Graph: 10 launches per graph (f5e_graph_*), HIP events around 5 replays.  Eager: HIP events around 5 calls.
GPU box only:  python tools/wavlm_time.py [--out profiles/wavlm_time.txt] [--no-torch]"""
import os
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from f5e_tts_amd import ops  # noqa: E402
from f5e_tts_amd.eval.wavlm import WavLM  # noqa: E402
from tools.mas_time import LAUNCHES, REPLAYS, time_eager, time_graph  # noqa: E402
from tools.src_hash import csrc_sha256  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import wavlm_ref as WR  # noqa: E402

I32 = torch.int32
OPS = ("wav_norm", "wavlm_conv0", "gemm_f32", "layernorm_gelu", "layernorm", "wavlm_posconv", "wavlm_gate", "relbias_attn")


def class_times(run, runs=3):
    """ms per run of every op class: each ops.* call of ``run`` between two HIP events."""
    real, marks = {n: getattr(ops, n) for n in OPS}, []

    def timed(name):
        def call(*a, **kw):
            label = name
            if name == "gemm_f32":
                label = f"gemm_f32 N={a[1].shape[0]} K={a[0].shape[1]}"
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = real[name](*a, **kw)
            e1.record()
            marks.append((label, e0, e1))
            return out
        return call
    run()
    torch.cuda.synchronize()
    try:
        for n in OPS:
            setattr(ops, n, timed(n))
        for _ in range(runs):
            run()
        torch.cuda.synchronize()
    finally:
        for n in OPS:
            setattr(ops, n, real[n])
    total = defaultdict(float)
    for label, e0, e1 in marks:
        total[label] += e0.elapsed_time(e1) / runs
    return dict(total)


def main():
    ops.require_device()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    with_torch = "--no-torch" not in sys.argv
    lines = [f"# python tools/wavlm_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# WavLM-large, synthetic weights, ragged B = 2; graph: ms per extract, {LAUNCHES} per graph, HIP events over {REPLAYS} "
             f"replays; eager: HIP events over 5 calls; classes: one HIP event pair per op, mean of 3 eager runs"]
    torch.manual_seed(4242)
    model = WavLM()
    sd_dev = {k: v.detach().cuda() for k, v in model.state_dict().items()} if with_torch else None
    model.cuda()
    side = torch.cuda.Stream()
    for seconds in (5, 10):
        S = 16000 * seconds
        lens = [S, int(0.6 * S)]
        wav = 0.1 * torch.randn(2, S, generator=torch.Generator().manual_seed(seconds))
        wav, ln = wav.cuda(), torch.tensor(lens, dtype=I32).cuda()
        T = model.frame_count(S)
        ws = torch.empty(model.workspace_bytes(2, S), dtype=torch.uint8, device="cuda")
        hs = torch.empty(25, 2, T, 1024, device="cuda")
        run = lambda: model.extract(wav, ln, out=hs, workspace=ws)[0]   # noqa: E731
        graph_ms = time_graph(run, side)
        eager_ms, got = time_eager(run)
        line = (f"extract B=2 {seconds} s lengths {lens} (T = {T}, workspace {ws.numel() / 1e6:.0f} MB): graph replay {graph_ms:8.3f} ms, "
                f"eager launches {eager_ms:8.3f} ms")
        if with_torch:
            torch_ms, (want, frames) = time_eager(lambda: WR.forward(sd_dev, model.cfg, wav, lens), reps=2)
            err = max(WR.rel_l2(got[:, b, :frames[b]].cpu(), want[:, b, :frames[b]].cpu()) for b in range(2))
            line += (f"  |  restated module, eager torch-ROCm {torch_ms:8.3f} ms = {torch_ms / graph_ms:5.2f} x the replay;  relative L2 of "
                     f"the hidden states {err:.1e}")
        lines.append(line)
        print(line, flush=True)
        cls = class_times(run)
        tot = sum(cls.values())
        for label, ms in sorted(cls.items(), key=lambda kv: -kv[1]):
            extra = ""
            if label == "wavlm_conv0":
                nbytes = 2 * S * 4 + 2 * ((S - 10) // 5 + 1) * 512 * 4
                extra = f"  ({nbytes / 1e6:.0f} MB moved: {nbytes / ms / 1e6:.0f} GB/s)"
            lines.append(f"  {seconds} s  {label:28s} {ms:8.3f} ms  {100 * ms / tot:5.1f} %{extra}")
            print(lines[-1], flush=True)
    if out_path:
        with open(os.path.join(ROOT, out_path) if not os.path.isabs(out_path) else out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
