#!/usr/bin/env python3
"""Yardstick for f5e_ctc_align and f5e_ctc_greedy (csrc/ctc.hip): ms per launch at a 30 s utterance (T = 1500 encoder
frames, L = 300 labels, V = 5000 classes; B = 1 and B = 16) and at the speech-edit clip (T = 300, L = 60), against the host
route: copy the [T, V] scores to the host and run the row-vectorised NumPy restatement there (tests/ctc_ref.py; the
reference's own forced_align is a Python double loop that takes 0.23 s for 120 frames x 41 states and is not timed).  The
copy is also timed alone: it bounds that route from below whatever the host program is.
Kernel: 10 launches per graph (f5e_graph_*), HIP events around 5 replays.  Host route: wall clock of one pass (synchronised).
GPU box only:  python tools/ctc_time.py [--out profiles/ctc_time.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from f5e_tts_amd import ops  # noqa: E402
from tools.mas_time import LAUNCHES, REPLAYS, time_graph, wall  # noqa: E402
from tools.src_hash import csrc_sha256  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctc_ref  # noqa: E402

I32 = torch.int32


def main():
    ops.require_device()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = [f"# python tools/ctc_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# kernels: ms per launch, {LAUNCHES}-launch graph, HIP events over {REPLAYS} replays; host route: wall ms of one pass"]
    side = torch.cuda.Stream()
    for name, B, T, L, V in (("30 s utterance", 1, 1500, 300, 5000), ("30 s utterance", 16, 1500, 300, 5000),
                             ("speech-edit clip", 1, 300, 60, 5000)):
        rng = np.random.default_rng(11)
        labels = rng.integers(1, V, size=(B, L)).astype(np.int32)
        host = rng.standard_normal((B, T, V)).astype(np.float32)
        for b in range(B):
            host[b] = ctc_ref.planted(T, labels[b], V, 12 + b)
        scores = torch.from_numpy(host).cuda()
        lab = torch.from_numpy(labels).cuda()
        t_len = torch.full((B,), T, dtype=I32, device="cuda")
        l_len = torch.full((B,), L, dtype=I32, device="cuda")
        al = torch.empty(B, T, dtype=I32, device="cuda")
        ts, te = torch.empty(B, L, dtype=I32, device="cuda"), torch.empty(B, L, dtype=I32, device="cuda")
        sc = torch.empty(B, device="cuda")
        ws = torch.empty(ops.ctc_align_workspace_bytes(B, T, L), dtype=torch.uint8, device="cuda")
        hyp, hyp_len = torch.empty(B, T, dtype=I32, device="cuda"), torch.empty(B, dtype=I32, device="cuda")
        logp = torch.empty(B, T, device="cuda")
        align_ms = time_graph(lambda: ops.ctc_align(scores, lab, t_len, l_len, 0, align=al, tok_start=ts, tok_end=te,
                                                    score=sc, workspace=ws), side)
        greedy_ms = time_graph(lambda: ops.ctc_greedy(scores, t_len, 0, V - 1, hyp=hyp, hyp_len=hyp_len, frame_logp=logp), side)
        d2h_ms, on_host = wall(lambda: scores.cpu().numpy())
        dp_ms, want = wall(lambda: ctc_ref.align(on_host, labels, [T] * B, [L] * B))
        gr_ms, hyps = wall(lambda: ctc_ref.greedy(on_host, [T] * B, 0, V - 1)[0])
        same = bool(np.array_equal(al.cpu().numpy(), want[0])) and \
            all(hyp[b, :int(hyp_len[b])].tolist() == hyps[b] for b in range(B))
        lines.append(f"{name}: B={B} T={T} L={L} V={V} ({B * T * V * 4 / 1e6:.1f} MB of scores)  f5e_ctc_align {align_ms:8.4f} ms"
                     f"  f5e_ctc_greedy {greedy_ms:8.4f} ms  |  host route: D2H {d2h_ms:8.3f} ms + NumPy align {dp_ms:9.2f} ms"
                     f" (greedy {gr_ms:8.2f} ms); the copy alone = {d2h_ms / align_ms:6.1f} x the align kernel;"
                     f"  results equal: {same}")
        print(lines[-1], flush=True)
    if out_path:
        with open(os.path.join(ROOT, out_path) if not os.path.isabs(out_path) else out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
