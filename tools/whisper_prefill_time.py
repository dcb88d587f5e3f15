"""Times Whisper's one-pass decoder prefill (``generate_from_kv(prefill=True)``: f5e_whisper_embed, f5e_attn_prefill_f32, f5e_mha_f32
with U queries per row, GEMMs over R * U rows) against the way the same prompt was fed before it (``prefill=False``: one cached
step per prompt token, the yardstick): ms from the first launch to the first picked token, for the decoders of large-v3-turbo and
large-v3 (random weights, random cross keys / values of 1500 positions), R = 1 and 8 rows, prompts of 4, 32 and 226 tokens (the
length of a fully conditioned window's prompt at the real models: <|startofprev|>, max_target_positions // 2 - 1 previous tokens
and the forced ones).  The two are ALTERNATED in one process (steps, prefill, steps,
prefill, ...), ``--runs`` runs each; a run is the median of ``--repeats`` measurements between device events after a warm-up of
both, and the record keeps every run's median with the smallest and largest measurement.  Both end in the same single pick, so
the difference is the prompt's.  Nothing is gated on these figures.

    python tools/whisper_prefill_time.py [--runs 3] [--repeats 5] [--out FILE]
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

F32 = torch.float32


def run_model(name, rows, prompts, runs, repeats):
    from f5e_tts_amd.eval import whisper as W
    from tools import synth as SY
    cfg = W.WhisperConfig(**SY.whisper_config_fields(name, encoder_layers=1))         # the decoder is what is timed
    with torch.device("cuda"):
        model = W.Whisper(cfg)
    shapes = {k: v.shape for k, v in model.state_dict().items()}
    model.load_state_dict(SY.init_whisper_state(shapes, 99, 4.0, device="cuda"), strict=False)
    g = torch.Generator(device="cuda").manual_seed(7)
    D, Tp = cfg.d_model, cfg.max_source_positions
    out = []
    for R in rows:
        kv = []
        for _ in range(cfg.decoder_layers):
            buf = torch.randn(R, Tp, 2 * D, generator=g, device="cuda")
            kv.append((buf[..., :D], buf[..., D:]))
        for n0 in prompts:
            ids = torch.randint(0, 50000, (R, n0), generator=g, device="cuda").tolist()
            for row in ids:
                row[-3:] = [cfg.decoder_start_token_id, 50259, 50360]

            def steps():
                return model.generate_from_kv(kv, ids, max_new_tokens=1)

            def prefill():
                return model.generate_from_kv(kv, ids, max_new_tokens=1, prefill=True)
            a, b = steps()[0], prefill()[0]                                              # warm-up of both, and the same pick
            torch.cuda.synchronize()
            rec = dict(model=name, decoder_layers=cfg.decoder_layers, rows=R, prompt_tokens=n0, same_pick=bool(torch.equal(a, b)),
                       steps_ms=[], prefill_ms=[])
            for _ in range(runs):
                for key, fn in (("steps_ms", steps), ("prefill_ms", prefill)):
                    rec[key].append(spread([events_ms(fn) for _ in range(repeats)]))
            out.append(rec)
            print(json.dumps(rec), flush=True)
        del kv
    del model
    torch.cuda.empty_cache()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--models", default="large-v3-turbo,large-v3")
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--prompts", default="4,32,226")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from f5e_tts_amd import ops
    ops.require_device()
    lines = [f"# python tools/whisper_prefill_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# fp32, eager launches, synthetic weights and cross keys / values; ms from the first launch to the first picked token; "
             f"{args.runs} alternated runs, each the median / min / max of {args.repeats} repeats"]
    with torch.no_grad():
        for name in [m for m in args.models.split(",") if m]:
            for rec in run_model(name, [int(r) for r in args.rows.split(",")], [int(p) for p in args.prompts.split(",")], args.runs,
                                 args.repeats):
                lines.append(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
