#!/usr/bin/env python3
"""Yardstick for f5e_mas_path (csrc/mas.hip): ms per launch at the C5 utterance (t_y 250 frames x t_x 60 tokens, B = 1) and
at the largest matrix the ABI admits (4096 x 4096, B = 8; with t_x = 3000, a wide band, and with t_x = t_y), against the
route a user of the reference takes: copy the matrix to the host, run the dynamic program there, copy the dense path back.
The host program here is the row-vectorised NumPy restatement of tests/mas_ref.py (numba, which the reference uses, is not
a dependency of this package); the two copies are also timed alone, since they bound that route from below whatever the
host program is.
Kernel: 10 launches per graph (f5e_graph_*), HIP events around 5 replays.  Host route: wall clock of one pass (synchronised).
GPU box only:  python tools/mas_time.py [--out profiles/mas_time.txt]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from f5e_tts_amd import ops  # noqa: E402
from tools.src_hash import csrc_sha256  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import mas_ref  # noqa: E402

I32 = torch.int32
LAUNCHES, REPLAYS = 10, 5


def time_graph(launch, stream):
    """ms per launch: LAUNCHES launches captured once through the project's f5e_graph_* (ops.Graph) on a side stream, HIP
    events around REPLAYS replays on that stream."""
    launch()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        g = ops.Graph()
        g.begin()
        try:
            for _ in range(LAUNCHES):
                launch()
        finally:
            g.end()
        g.launch()
        stream.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(REPLAYS):
            g.launch()
        t1.record(stream)
        t1.synchronize()
        g.destroy()
    return t0.elapsed_time(t1) / (REPLAYS * LAUNCHES)


def time_eager(fn, reps=5):
    """ms per call of an eager torch expression, HIP events around `reps` calls after one warm call."""
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        out = fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps, out


def host_dp(logp, t_y, t_x):
    """The search on the host: the row-vectorised NumPy restatement the tests use (tests/mas_ref.py) -> dense path f32."""
    tok, _ = mas_ref.mas_index(logp, t_y, t_x)
    return mas_ref.dense(tok, logp.shape[2]).astype(np.float32)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ops.require_device()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = [f"# python tools/mas_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# kernel: ms per launch, {LAUNCHES}-launch graph, HIP events over {REPLAYS} replays; host route: wall ms of one pass"]
    side = torch.cuda.Stream()
    # the largest matrix the ABI admits, once with a wide band (t_x = 3000: 7.8 M band cells per sequence, close to the
    # maximum of t_x (t_y - t_x + 1) at t_x = 2048) and once as the issue's shape reads (t_x = t_y: the band is the diagonal)
    for name, B, Ty, Tx, ty, tx in (("C5 utterance", 1, 250, 60, 250, 60),
                                    ("4096 x 4096, wide band (t_x = 3000)", 8, 4096, 4096, 4096, 3000),
                                    ("4096 x 4096, t_x = t_y (diagonal band)", 8, 4096, 4096, 4096, 4096)):
        logp = torch.randn(B, Ty, Tx, generator=torch.Generator().manual_seed(7)).cuda() * 3.0 - 4.0
        t_y = torch.full((B,), ty, dtype=I32, device="cuda")
        t_x = torch.full((B,), tx, dtype=I32, device="cuda")
        tok = torch.empty(B, Ty, dtype=I32, device="cuda")
        dur = torch.empty(B, Tx, dtype=I32, device="cuda")
        ws = torch.empty(ops.mas_workspace_bytes(B, Ty, Tx), dtype=torch.uint8, device="cuda")
        kernel_ms = time_graph(lambda: ops.mas_path(logp, t_y, t_x, tok, dur, workspace=ws), side)
        # the dense path a caller of the reference gets, expanded on the device from the indices
        dense_ms, dense = time_eager(lambda: (tok.unsqueeze(-1) == torch.arange(Tx, device="cuda", dtype=I32)).float())
        d2h_ms, host = wall(lambda: logp.cpu().numpy())
        dp_ms, path = wall(lambda: host_dp(host, [ty] * B, [tx] * B))
        h2d_ms, back = wall(lambda: torch.from_numpy(path).cuda())
        same = bool(torch.equal(back, dense))
        mb = B * Ty * Tx * 4 / 1e6
        lines.append(f"{name}: B={B} Ty={Ty} Tx={Tx} t_y={ty} t_x={tx} ({mb:.1f} MB matrix)  f5e_mas_path {kernel_ms:9.4f} ms"
                     f"  (+ dense expansion {dense_ms:8.3f} ms, eager torch, mean of 5)  |  host route: D2H {d2h_ms:9.3f}"
                     f" + NumPy DP {dp_ms:10.2f}"
                     f" + H2D {h2d_ms:9.3f} ms; copies alone {d2h_ms + h2d_ms:9.3f} ms = {(d2h_ms + h2d_ms) / kernel_ms:7.1f} x the"
                     f" kernel;  paths equal: {same}")
        print(lines[-1], flush=True)
        del logp, dense, back
    if out_path:
        with open(os.path.join(ROOT, out_path) if not os.path.isabs(out_path) else out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
