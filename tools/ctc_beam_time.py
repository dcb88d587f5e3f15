#!/usr/bin/env python3
"""Yardstick for f5e_ctc_beam (csrc/ctc_beam.hip) and the rescoring pass of ``ConformerPPG.attention_rescoring``.

Beam search: ms per launch at (B, T, V, K) = (1, 250, 218, 10), (16, 750, 218, 10) and (1, 1500, 5000, 10) against the
copy-to-host route: D2H of the [B, T, V] scores plus the NumPy restatement of the reference's loop (tests/ctc_beam_ref.py,
fp64; the reference's own loop adds an .item() per symbol on top).  The restatement is timed on ONE sequence and multiplied
by B; the copy is also timed alone, it bounds that route from below whatever the host program is.
Kernel: 10 launches per graph (f5e_graph_*), HIP events around 5 replays (the method of tools/ctc_time.py).

Rescoring: one decoder pass over N = 10 hypotheses of 30 tokens against 250 encoder frames (D = 256, 4 heads, 6 blocks, 2048
units, V = 218), as built (the memory's keys / values projected once, the N hypotheses' queries in one source-attention
launch) against the reference's layout (the encoder output repeated N times, one item per hypothesis).  Eager launches, HIP
events around 5 passes.
GPU box only:  python tools/ctc_beam_time.py [--out profiles/ctc_beam_time.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from f5e_tts_amd import ops  # noqa: E402
from tools.mas_time import LAUNCHES, REPLAYS, time_eager, time_graph, wall  # noqa: E402
from tools.src_hash import csrc_sha256  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctc_beam_ref  # noqa: E402
import ctc_ref  # noqa: E402

I32 = torch.int32


def beam_lines(side):
    lines = []
    for B, T, V, K in ((1, 250, 218, 10), (16, 750, 218, 10), (1, 1500, 5000, 10)):
        rng = np.random.default_rng(21)
        host = np.stack([ctc_ref.planted(T, rng.integers(1, V, size=T // 5), V, 22 + b, boost=8.0) * np.float32(2.0)
                         for b in range(B)])
        scores = torch.from_numpy(host).cuda()
        t_len = torch.full((B,), T, dtype=I32, device="cuda")
        hyp = torch.empty(B, K, T, dtype=I32, device="cuda")
        n, sc = torch.empty(B, K, dtype=I32, device="cuda"), torch.empty(B, K, device="cuda")
        ws = torch.empty(ops.ctc_beam_workspace_bytes(B, T, K), dtype=torch.uint8, device="cuda")
        ms = time_graph(lambda: ops.ctc_beam_search(scores, t_len, K, 0, hyp=hyp, hyp_len=n, score=sc, workspace=ws), side)
        d2h_ms, on_host = wall(lambda: scores.cpu().numpy())
        np_ms, (want, delta) = wall(lambda: ctc_beam_ref.search(on_host[0], K))
        got = [tuple(hyp[0, k, :int(n[0, k])].tolist()) for k in range(K)]
        lines.append(f"B={B} T={T} V={V} K={K} ({B * T * V * 4 / 1e6:.1f} MB of scores)  f5e_ctc_beam {ms:8.4f} ms  |  host route: "
                     f"D2H {d2h_ms:8.3f} ms + NumPy search {np_ms:9.1f} ms x {B}; the copy alone = {d2h_ms / ms:6.1f} x the kernel;"
                     f"  best hypothesis equal: {got[0] == want[0][0]}, whole list: {got == [h for h, _ in want]}"
                     f" (margin delta {delta:.1e})")
        print(lines[-1], flush=True)
    return lines


def rescoring_lines():
    from f5e_tts_amd.ppg.ppg_model import ConformerPPG
    N, U1, T2, V = 10, 31, 250, 218
    torch.manual_seed(5)
    m = ConformerPPG(vocab_size=V, num_blocks=1, ctc=True, decoder="transformer").cuda().eval()
    eng = m.engine()
    g = torch.Generator().manual_seed(6)
    mem = torch.randn(1, T2, eng.dim, generator=g).cuda()
    ys = torch.randint(0, V, (N, U1), generator=g).to(I32).cuda()
    lens = torch.full((N,), U1, dtype=I32, device="cuda")
    rep = mem.repeat(N, 1, 1).contiguous()
    shared_ms, a = time_eager(lambda: eng.decode("left", mem, None, ys, lens, N))
    repeated_ms, b = time_eager(lambda: eng.decode("left", rep, None, ys, lens, 1))
    err = float((a - b).abs().max())
    line = (f"rescoring pass N={N} U+1={U1} T'={T2} D={eng.dim} 6 blocks V={V}: keys / values once per utterance "
            f"{shared_ms:8.3f} ms  |  encoder output repeated N times {repeated_ms:8.3f} ms  ({repeated_ms / shared_ms:4.2f} x);"
            f"  max |difference| of the logits {err:.1e}")
    print(line, flush=True)
    return [line]


def main():
    ops.require_device()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = [f"# python tools/ctc_beam_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# kernel: ms per launch, {LAUNCHES}-launch graph, HIP events over {REPLAYS} replays; host route: wall ms of one pass"]
    lines += beam_lines(torch.cuda.Stream())
    lines += rescoring_lines()
    if out_path:
        with open(os.path.join(ROOT, out_path) if not os.path.isabs(out_path) else out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
