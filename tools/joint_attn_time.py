#!/usr/bin/env python3
"""Yardstick: us per launch of f5e_joint_attn (MMDiT: N audio + Nt text keys and queries) against f5e_flash_attn over the
same total number of keys and queries (one sequence of N + Nt), S = 1 x 16 heads, the library's own split pick, 22
launches per graph on rotating buffers, HIP events around 20 replays.
GPU box only:  python tools/joint_attn_time.py [N,Nt ...]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from f5e_tts_amd import ops  # noqa: E402

BF = torch.bfloat16
LAUNCHES, REPLAYS = 22, 20


def time_graph(launch):
    launch(0)
    launch(1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(LAUNCHES):
            launch(i)
    g.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(REPLAYS):
        g.replay()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / (REPLAYS * LAUNCHES)


def pad64(n):
    return (n + 63) // 64 * 64


def bufs(S, H, n, sets=6):
    return [[(torch.randn(S, H, pad64(n), 64, device="cuda") * 0.18).to(BF) for _ in range(3)] for _ in range(sets)]


def main():
    ops.require_device()
    cases = [(938, 200), (469, 100), (938, 13), (1876, 200)]
    if len(sys.argv) > 1:   # "N,Nt N,Nt ..."
        cases = [tuple(int(x) for x in a.split(",")) for a in sys.argv[1:]]
    S, H = 1, 16
    for N, Nt in cases:
        bx, bc, bf = bufs(S, H, N), bufs(S, H, Nt), bufs(S, H, N + Nt)
        ox = torch.empty(S * N, H * 64, device="cuda", dtype=BF)
        oc = torch.empty(S * Nt, H * 64, device="cuda", dtype=BF)
        of = torch.empty(S * (N + Nt), H * 64, device="cuda", dtype=BF)
        joint = time_graph(lambda i: ops.joint_attn(*bx[i % 6], *bc[i % 6], ox, oc, N, Nt))
        joint_x = time_graph(lambda i: ops.joint_attn(*bx[i % 6], *bc[i % 6], ox, None, N, Nt))
        flash = time_graph(lambda i: ops.flash_attn(*bf[i % 6], of, N + Nt))
        print(f"S={S} H={H} N={N:5d} Nt={Nt:4d}  joint {joint:7.2f}  joint (no text queries) {joint_x:7.2f}  "
              f"flash over {N + Nt:5d} {flash:7.2f}  us per launch  (joint / flash {joint / flash:5.3f})", flush=True)


if __name__ == "__main__":
    sys.exit(main())
