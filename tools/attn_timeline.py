"""In-kernel timeline of the batch-1 attention launch (4 KV splits) inside a chain of dependent launches replayed from a
hipGraph, the way it runs inside one DiT evaluation.   usage: python tools/attn_timeline.py [S H N] [--out FILE]

Needs the TOOLS build (make -C f5e-tts_amd/csrc tools-lib; F5E_HIP_LIB=f5e-tts_amd/libf5e_hip_tools.so): its stamped kernel
instantiations write per workgroup and wave the shader clock at the first instruction, at entry (past the prefetch branch), Q landed, first / second tile landed, at and past the
merge barrier and after the last store (f5e_debug_attn_trace).  F5E_ATTN_VARIANT=4 keeps the general attn_fwd_kernel<4> loop
at every size (the kernel before the batch-1 variant).  The stamped build's fences forbid overlaps the real kernel has: read
its shares, not its length; the per-launch time printed first is the UNSTAMPED kernel in the same chain."""
import ctypes
import importlib
import os
import sys

import torch

sys.path.insert(0, ".")
ops = importlib.import_module("f5e-tts_amd.ops")
_C = importlib.import_module("f5e-tts_amd._C")
from tools.src_hash import csrc_sha256  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
S, H, N = (int(v) for v in args[:3]) if len(args) >= 3 else (2, 16, 469)
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
BF = torch.bfloat16
CHAIN = 22
n_pad = (N + 63) // 64 * 64
gen = torch.Generator().manual_seed(7)
q, k, vt = (torch.randn(S, H, n_pad, 64, generator=gen).mul(0.3).to(BF).cuda() for _ in range(3))
lens = torch.full((S,), N, dtype=torch.int32).cuda()
o = torch.empty(S * N, H * 64, device="cuda", dtype=BF)


def chain():
    for _ in range(CHAIN):
        ops.flash_attn(q, k, vt, o, N, kv_len=lens, waves=4)


def graph_of_chain(st):
    gr = ops.Graph()
    gr.begin()
    try:
        chain()
    finally:
        gr.end()
    return gr


lines = [f"# python tools/attn_timeline.py {S} {H} {N} on one MI355X; F5E_ATTN_VARIANT={os.environ.get('F5E_ATTN_VARIANT', '')!r}; "
         f"csrc_sha256 {csrc_sha256()}"]
st = torch.cuda.Stream()
with torch.cuda.stream(st):
    chain()
    st.synchronize()
    gr = graph_of_chain(st)
    for _ in range(3):
        gr.launch()
    st.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(9):
        e0.record(st)
        gr.launch()
        e1.record(st)
        st.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / CHAIN)
    ts.sort()
    gr.destroy()
    lines.append(f"unstamped kernel, {CHAIN} dependent launches in a graph: median {ts[len(ts) // 2]:.2f} us per launch "
                 f"(min {ts[0]:.2f}, max {ts[-1]:.2f}; launch gap included)")

    qtiles = (N + 31) // 32
    nwg = qtiles * H * S
    buf = torch.zeros(nwg * 4 * 8, dtype=torch.int64, device="cuda")
    hook = _C.lib().f5e_debug_attn_trace      # TOOLS build only
    hook.argtypes, hook.restype = [ctypes.c_void_p], None
    hook(ctypes.c_void_p(buf.data_ptr()))
    gr = graph_of_chain(st)                   # the kernel arguments carry the trace pointer: the chain's last launch stays
    hook(ctypes.c_void_p(0))
    for _ in range(3):
        gr.launch()
    st.synchronize()
    gr.destroy()

t = buf.view(nwg, 4, 8).cpu().double()
names = ["entry", "Q landed", "tile 1 landed", "tile 2 landed", "at merge barrier", "past merge barrier", "last store issued"]
rel = t[:, :, :7] - t[:, :, :1]
wg_span = (t[:, :, 1:7].amax(dim=(1, 2)) - t[:, :, 0].amin(dim=1))
lines.append(f"stamped kernel, last launch of the chain, {nwg} workgroups x 4 waves; shader-clock cycles from each wave's entry "
             f"(median | 10 % | 90 %), 0 = not stamped on this path")
for i, nm in enumerate(names):
    if i == 0:
        continue
    row = [f"{nm:>20}: all waves"]
    for w in (None, 0, 1, 2, 3):
        x = (rel[:, :, i] if w is None else rel[:, w, i]).reshape(-1)
        x = x[x > 0]
        if x.numel() == 0:
            row.append("      -")
            continue
        qs = torch.quantile(x, torch.tensor([0.5, 0.1, 0.9], dtype=torch.double))
        cell = f"{qs[0]:6.0f} | {qs[1]:6.0f} | {qs[2]:6.0f}"
        row.append(cell if w is None else f"w{w} {qs[0]:6.0f}")
    lines.append("  ".join(row))
head = (t[:, :, 0] - t[:, :, 7]).reshape(-1)   # [7]: the wave's first instruction; [0]: past the prefetch branch (needs n_main)
hq = torch.quantile(head, torch.tensor([0.5, 0.1, 0.9], dtype=torch.double))
lines.append(f"wave's first instruction -> entry stamp (what the launch head waits for before its first load can go out): "
             f"{hq[0]:.0f} | {hq[1]:.0f} | {hq[2]:.0f} cycles")
entry_spread = t[:, :, 0].amax(dim=1) - t[:, :, 0].amin(dim=1)
lines.append(f"workgroup span (first wave's entry -> last stamp of any wave): median {wg_span.median():.0f} cycles, "
             f"90 % {torch.quantile(wg_span, 0.9):.0f}; entry spread inside a workgroup: median {entry_spread.median():.0f}")
print("\n".join(lines))
if out_path:
    open(out_path, "w").write("\n".join(lines) + "\n")
