"""Times Whisper's word-timestamp kernels (csrc/whisper_align.hip) at the whisper-large-v3 shape -- 20 heads of 64, 1500 keys, the
checkpoint's 10 alignment heads (one per layer, so one f5e_cross_attn_probs_f32 launch of one head each) -- with synthetic weights
(tools/synth.py), one 30 s utterance, random tokens fed through the cached step:
  * us per f5e_cross_attn_probs_f32 launch (one row, one head, all 1500 columns kept);
  * ms of f5e_dtw_cost_f32 + f5e_dtw_path, and of each alone, at N = 32 and 128 rows with M = 500 and 1500 columns, on the
    probabilities the model produced;
  * the same on the copy-to-host route of the reference: the device-to-host copy of the selected heads' weights, then NumPy
    (normalise, median filter, mean) and the cell-by-cell Python loop of the dynamic time warping, restated here.  The two routes
    must give the same path: checked.
Device events around work on one stream after a warm-up (the host route: wall clock around a synchronised copy); every figure is
the median of ``--repeats`` measurements with their smallest and largest.  Nothing is gated on these figures.

    python tools/whisper_align_time.py [--repeats 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.src_hash import csrc_sha256  # noqa: E402

F32, I32 = torch.float32, torch.int32
# generation_config.alignment_heads of openai/whisper-large-v3
LARGE_V3_HEADS = ((7, 0), (10, 17), (12, 18), (13, 12), (16, 1), (17, 14), (19, 11), (21, 4), (24, 1), (25, 6))


def events_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def spread(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values))


def host_route(probs_dev, N, M, width):
    """The reference's route, restated: weights to the host, NumPy for the cost matrix, a Python double loop for the warping.
    -> (first, seconds of the copy, seconds of the arithmetic)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    w = probs_dev[0, :, :N, :M].cpu()
    t1 = time.perf_counter()
    w = w.numpy()
    z = (w - w.mean(1, keepdims=True)) / w.std(1, keepdims=True)
    pad = width // 2
    zp = np.pad(z, ((0, 0), (0, 0), (pad, pad)), mode="reflect")
    z = np.sort(np.stack([zp[..., k:k + M] for k in range(width)], -1), -1)[..., pad]
    C = -z.mean(0).astype(np.float64)
    cost = np.ones((N + 1, M + 1), dtype=np.float32) * np.inf
    trace = -np.ones((N + 1, M + 1), dtype=np.float32)
    cost[0, 0] = 0
    for j in range(1, M + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = C[i - 1, j - 1] + c
            trace[i, j] = t
    first = np.full(N, -1)
    i, j = N, M
    while i > 0 and j > 0:
        t = trace[i, j]
        if t != 2:
            first[i - 1] = j - 1
        i, j = (i - 1, j - 1) if t == 0 else (i - 1, j) if t == 1 else (i, j - 1)
    return first, t1 - t0, time.perf_counter() - t1


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from f5e_tts_amd import ops
    from f5e_tts_amd.eval import whisper as W
    from tools import synth as SY
    ops.require_device()
    lines = [f"# python tools/whisper_align_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# whisper-large-v3 shape, 10 alignment heads, one 30 s utterance, synthetic weights, random tokens, fp32, eager launches; "
             f"median / min / max of {args.repeats} repeats"]
    with torch.no_grad():
        cfg = W.WhisperConfig(**SY.whisper_config_fields("large-v3"), alignment_heads=LARGE_V3_HEADS)
        with torch.device("cuda"):
            model = W.Whisper(cfg)
        shapes = {k: v.shape for k, v in model.state_dict().items()}
        model.load_state_dict(SY.init_whisper_state(shapes, 99, 4.0, device="cuda"), strict=False)
        kv = model.encode(SY.synthetic_ref_wave(3000, seed=5, hop=160).cuda())
        D, H = cfg.d_model, cfg.decoder_attention_heads
        q = torch.randn(1, D, device="cuda")
        out = torch.zeros(1, 1, 1500, device="cuda")
        head = torch.tensor([3], dtype=I32, device="cuda")

        def probs_launches(reps=500):
            for _ in range(reps):
                ops.cross_attn_probs_f32(q, kv[0][0], head, H, (D // H) ** -0.5, out)
        probs_launches(10)
        torch.cuda.synchronize()
        lines.append(json.dumps(dict(cross_attn_probs_us=spread([1e3 * events_ms(probs_launches) / 500 for _ in range(args.repeats)]))))
        print(lines[-1], flush=True)
        prompt = model.prompt_ids("en")
        n0, g = len(prompt), torch.Generator().manual_seed(11)
        for N in (32, 128):
            ids = torch.cat([torch.tensor(prompt), torch.randint(0, 50000, (N + 1,), generator=g)]).to(I32).cuda()[None]
            for M in (500, 1500):
                probs, n_rows, m_len = model.alignment_probs(kv, ids, [n0 + N + 1], 2 * M, n0)
                ws = torch.empty(ops.dtw_workspace_bytes(1, N, probs.shape[3]) // 4, dtype=I32, device="cuda")
                cost = ops.dtw_cost_f32(probs, n_rows, m_len, cfg.median_filter_width)
                first = ops.dtw_path(cost, n_rows, m_len, workspace=ws)

                def both():
                    ops.dtw_path(ops.dtw_cost_f32(probs, n_rows, m_len, cfg.median_filter_width, out=cost), n_rows, m_len, first=first,
                                 workspace=ws)
                both()
                torch.cuda.synchronize()
                rec = dict(N=N, M=M,
                           device_cost_and_path_ms=spread([events_ms(both) for _ in range(args.repeats)]),
                           device_cost_ms=spread([events_ms(lambda: ops.dtw_cost_f32(probs, n_rows, m_len, cfg.median_filter_width,
                                                                                      out=cost)) for _ in range(args.repeats)]),
                           device_path_ms=spread([events_ms(lambda: ops.dtw_path(cost, n_rows, m_len, first=first, workspace=ws))
                                                  for _ in range(args.repeats)]))
                host = [host_route(probs, N, M, cfg.median_filter_width) for _ in range(args.repeats)]
                rec["host_copy_ms"] = spread([1e3 * h[1] for h in host])
                rec["host_numpy_and_loop_ms"] = spread([1e3 * h[2] for h in host])
                rec["paths_equal"] = bool(np.array_equal(host[0][0], first[0, :N].cpu().numpy()))
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
