"""Times Whisper's 16-bit weight modes (``Whisper(weights="fp16" | "bf16")``) against fp32 at the large-v3 and
large-v3-turbo decoder shapes, synthetic weights, B = 1 and B = 4 rows:

  * per launch: ``ops.gemm_f32_w16_skinny`` beside ``ops.gemm_f32_skinny`` on the step's GEMM shapes (q|k|v, the three D x D
    projections, FF1, FF2) and the logits GEMM.  Inside a decode step every weight comes from HBM (the decoder is far larger
    than the 256 MiB Infinity Cache), so a launch here never meets the matrix it read last: each arm cycles over copies of W
    that total at least ``--cold_mb`` megabytes in ITS OWN type.  One measurement = one pass over all copies, replayed from
    a hipGraph (an eager loop of launches this short measures the host's enqueue rate), between two device events, ended by a
    synchronise; us per launch = that time over the number of copies.  The arms (f32, fp16, bf16)
    are alternated; the record keeps the median, the smallest and the largest of ``--repeats`` measurements after a warm-up
    pass of each, the bytes of W per launch, and the GB/s they amount to;
  * per decode step, in each weight mode: ms per token of the eager step, the captured step and the captured step with
    ``step_gemm="skinny"`` (``tools/whisper_step_time.py``'s arms and method: 64 greedy picks behind a prompt of 4, arms
    alternated within a mode; the modes one after another, each on a model built from the same seed), and
    ``Whisper.device_bytes()`` of that model (one encoder layer: the decoder is what is timed);
  * per weight mode, the large-v3 ENCODER (32 layers, one decoder layer): ms of ``encode_features`` + ``cross_kv`` on one
    30-second window of random features, median of ``--repeats`` after a warm-up, the modes one after another.  In a 16-bit
    mode these GEMMs run on the register-staged tile instead of ``f5e_gemm_f32``'s LDS-DMA kernel.

Clocks: whatever the device runs at under this load, not pinned; read the spread.  Nothing is gated on these figures.

    python tools/whisper_w16_time.py [--repeats 7] [--tokens 64] [--cold_mb 600] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.src_hash import csrc_sha256  # noqa: E402
from tools.whisper_beam_time import events_ms, spread  # noqa: E402
from tools.whisper_step_time import time_shape  # noqa: E402

F32 = torch.float32
MODES = (("f32", F32), ("fp16", torch.float16), ("bf16", torch.bfloat16))


def size_of(dt):
    return torch.finfo(dt).bits // 8


def time_launches(name, B, repeats, cold_mb):
    """us per launch of the skinny GEMM in each weight type on the decoder's shapes, W cold."""
    from f5e_tts_amd import ops
    from tools import synth as SY
    f = SY.whisper_config_fields(name)
    D, FF, V = f["d_model"], f["decoder_ffn_dim"], f["vocab_size"]
    g = torch.Generator(device="cuda").manual_seed(5)
    side = torch.cuda.Stream()
    out = []
    for label, N, K, act in (("qkv", 3 * D, D, 0), ("out / xq / xout", D, D, 0), ("ff1", FF, D, ops.ACT_GELU_ERF), ("ff2", D, FF, 0),
                             ("logits", V, D, 0)):
        a = torch.randn(B, K, generator=g, device="cuda")
        bias = torch.randn(N, generator=g, device="cuda")
        y = torch.empty(B, N, device="cuda")
        arms, copies, graphs = {}, {}, []
        scratch = torch.empty(max(ops.gemm_f32_skinny_workspace(N, K), 16) // 4, device="cuda")
        for mode, dt in MODES:
            n = max(2, -(-cold_mb * 1000000 // (N * K * size_of(dt))))
            ws = [(torch.randn(N, K, generator=g, device="cuda") * K ** -0.5).to(dt) for _ in range(n)]
            fn = ops.gemm_f32_skinny if dt == F32 else ops.gemm_f32_w16_skinny
            copies[mode] = n

            def run(ws=ws, fn=fn):
                for w in ws:
                    fn(a, w, bias, out=y, act=act, workspace=scratch)
            run()                                          # warm-up, eager
            # the pass as ONE hipGraph (a linear chain captured on a side stream): an eager loop of launches this short
            # measures the host's enqueue rate (about 20 us per call through the wrapper), not the kernels
            graph = ops.Graph()
            with torch.cuda.stream(side):
                graph.begin()
                try:
                    run()
                finally:
                    graph.end()
            graphs.append(graph)
            arms[mode] = graph.launch
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
        us = {mode: [] for mode in arms}
        for _ in range(repeats):
            for mode, fn in arms.items():
                us[mode].append(events_ms(fn) * 1e3 / copies[mode])
        rec = dict(model=name, rows=B, shape=label, N=N, K=K, copies=copies, us_per_launch={m: spread(v) for m, v in us.items()},
                   w_bytes={m: N * K * size_of(dt) for m, dt in MODES})
        rec["w_gb_per_s"] = {m: rec["w_bytes"][m] / rec["us_per_launch"][m]["median"] * 1e-3 for m in us}
        rec["speedup_over_f32"] = {m: rec["us_per_launch"]["f32"]["median"] / rec["us_per_launch"][m]["median"] for m in us if m != "f32"}
        out.append(rec)
        torch.cuda.synchronize()
        del arms, ws, graphs
        torch.cuda.empty_cache()
    return out


def time_encoder(name, repeats):
    """ms per window of the encoder and the cross K/V projections in each weight mode."""
    from f5e_tts_amd.eval import whisper as W
    from tools import synth as SY
    out = []
    for mode, _ in MODES:
        cfg = W.WhisperConfig(**SY.whisper_config_fields(name, decoder_layers=1))
        with torch.device("cuda"):
            model = W.Whisper(cfg, weights=mode)
        shapes = {k: v.shape for k, v in model.state_dict().items()}
        model.load_state_dict(SY.init_whisper_state(shapes, 99, 4.0, device="cuda"), strict=False)
        g = torch.Generator(device="cuda").manual_seed(3)
        feats = torch.randn(1, 2 * cfg.max_source_positions, cfg.num_mel_bins, generator=g, device="cuda")

        def run():
            model.cross_kv(model.encode_features(feats))
        run()
        torch.cuda.synchronize()
        ms = [events_ms(run) for _ in range(repeats)]
        out.append(dict(model=name, weights=mode, encoder_layers=cfg.encoder_layers, rows=1, encode_ms=spread(ms),
                        device_bytes=model.device_bytes()))
        del model, feats
        torch.cuda.empty_cache()
    for rec in out:
        rec["speedup_over_f32"] = out[0]["encode_ms"]["median"] / rec["encode_ms"]["median"]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--models", default="large-v3,large-v3-turbo")
    ap.add_argument("--rows", default="1,4")
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cold_mb", type=int, default=600)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from f5e_tts_amd import ops
    ops.require_device()
    lines = [f"# python tools/whisper_w16_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# synthetic weights; clocks not pinned; median / min / max of {args.repeats} measurements between device events, arms "
             f"alternated; launches: W cold (copies of W totalling >= {args.cold_mb} MB per arm); steps: {args.tokens} greedy picks "
             "behind a prompt of 4"]

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    with torch.no_grad():
        for name in args.models.split(","):
            for B in (int(b) for b in args.rows.split(",")):
                for rec in time_launches(name, B, args.repeats, args.cold_mb):
                    emit(rec)
        for name in args.models.split(","):
            for B in (int(b) for b in args.rows.split(",")):
                base = None
                for mode, _ in MODES:
                    rec = time_shape(name, B, args.tokens, args.repeats, weights=mode,
                                     inspect=lambda m, mode=mode: dict(weights=mode, device_bytes=m.device_bytes()))
                    med = {arm: v["median"] for arm, v in rec["ms_per_token"].items()}
                    base = med if base is None else base
                    rec["speedup_over_f32"] = {arm: base[arm] / med[arm] for arm in med}
                    emit(rec)
        for rec in time_encoder("large-v3", args.repeats):
            emit(rec)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
