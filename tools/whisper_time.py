"""Times one 30 s utterance through eval/whisper.py at the whisper-large-v3 and -large-v3-turbo shapes with synthetic weights
(tools/synth.py): front-end, encoder (+ the cross keys / values of every decoder layer), and the per-token decode -- with
f5e_cross_attn_decode_f32, and with f5e_mha_f32 at Tq = 1 in its place (same numbers up to summation order: checked here).
Also the two attention kernels alone on one layer's shape.  Device events around work on one stream; every shape is warmed up
first.  Nothing is gated on these figures.

    python tools/whisper_time.py [--models large-v3,large-v3-turbo] [--tokens 32] [--out FILE]
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


def timed(fn, reps):
    """Mean milliseconds of ``fn()`` over ``reps`` calls between two device events (after one warm-up call)."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def mha_in_place_of_cross(ops):
    """A drop-in for ops.cross_attn_decode_f32 (one row per utterance) on f5e_mha_f32 with Tq = 1."""
    def run(q, k, v, heads, scale, rows_per_utt=1, kv_len=None, out=None):
        B, Tk, D = k.shape
        assert rows_per_utt == 1 and kv_len is None
        return ops.mha_f32(q, k.as_strided((B * Tk, D), (k.stride(1), 1)), v.as_strided((B * Tk, D), (v.stride(1), 1)), heads, scale,
                           B=B, out=out)
    return run


def decode_ms(model, kv, prompt, n_tokens):
    """Mean milliseconds per decoder step (all layers + logits + pick) over ``n_tokens`` steps after the prompt."""
    from f5e_tts_amd import ops
    dev = kv[0][0].device
    B = kv[0][0].shape[0]
    U = len(prompt) + n_tokens
    st = model._dec_state(B, U, dev)
    fd = model._fold()
    tokens = torch.full((B, U), model.cfg.eos_token_id, dtype=torch.int32, device=dev)
    tokens[:, :len(prompt)] = torch.tensor(prompt, dtype=torch.int32, device=dev)
    last = tokens[:, 0].clone()
    done, alive = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)

    def steps(lo, hi):
        for p in range(lo, hi):
            logits = model._dec_step(st, kv, last, p, True)
            done.zero_()                                      # keep every step a full step, whatever the synthetic model picks
            ops.greedy_pick(logits, tokens, last, done, alive, p, model.cfg.eos_token_id, suppress=fd["suppress"],
                            begin_suppress=fd["begin_suppress"], first_step=False)
    steps(0, len(prompt))                                    # warm-up: the prompt positions
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    steps(len(prompt), U - 1)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / (U - 1 - len(prompt)), tokens


def run_model(name, n_tokens):
    from f5e_tts_amd import ops
    from f5e_tts_amd.eval import whisper as W
    from tools import synth as SY
    cfg = W.WhisperConfig(**SY.whisper_config_fields(name))
    with torch.device("cuda"):
        model = W.Whisper(cfg)
    shapes = {k: v.shape for k, v in model.state_dict().items()}
    model.load_state_dict(SY.init_whisper_state(shapes, 99, 4.0, device="cuda"), strict=False)
    wav = SY.synthetic_ref_wave(3000, seed=5, hop=160).cuda()           # 30 s
    rec = dict(model=name, encoder_layers=cfg.encoder_layers, decoder_layers=cfg.decoder_layers, seconds=wav.shape[1] / 16000.0)
    rec["front_end_ms"] = timed(lambda: model.features(wav), 20)
    feats = model.features(wav)
    rec["encoder_ms"] = timed(lambda: model.encode_features(feats), 3)
    enc = model.encode_features(feats)
    rec["cross_kv_ms"] = timed(lambda: model.cross_kv(enc), 3)
    kv = model.cross_kv(enc)
    prompt = model.prompt_ids("en")
    real = ops.cross_attn_decode_f32
    rec["decode_ms_per_token"], tok_a = decode_ms(model, kv, prompt, n_tokens)
    ops.cross_attn_decode_f32 = mha_in_place_of_cross(ops)
    try:
        rec["decode_ms_per_token_mha_tq1"], tok_b = decode_ms(model, kv, prompt, n_tokens)
    finally:
        ops.cross_attn_decode_f32 = real
    rec["tokens_equal"] = bool(torch.equal(tok_a, tok_b))
    # the two kernels alone on one layer's shape
    D, H = cfg.d_model, cfg.decoder_attention_heads
    q = torch.randn(1, D, device="cuda")
    K, V = kv[0]
    rec["cross_attn_kernel_us"] = 1e3 * timed(lambda: ops.cross_attn_decode_f32(q, K, V, H, (D // H) ** -0.5), 500)
    mha = mha_in_place_of_cross(ops)
    rec["mha_tq1_kernel_us"] = 1e3 * timed(lambda: mha(q, K, V, H, (D // H) ** -0.5), 500)
    a, b = ops.cross_attn_decode_f32(q, K, V, H, (D // H) ** -0.5), mha(q, K, V, H, (D // H) ** -0.5)
    rec["kernels_rel_l2"] = float((a - b).norm() / b.norm())
    del model, kv
    torch.cuda.empty_cache()
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--models", default="large-v3,large-v3-turbo")
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from f5e_tts_amd import ops
    ops.require_device()
    recs = []
    with torch.no_grad():
        for name in args.models.split(","):
            recs.append(run_model(name, args.tokens))
            print(json.dumps(recs[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
