"""Times Whisper's assisted generation (``generate_from_kv(assistant=)``) at the large-v3 decoder's shape with a
turbo-shaped (4-layer) draft, synthetic weights and random cross keys / values of 1500 positions, R = 1 row:

  * ms per ROUND at U = 2, 4, 8 drafted tokens, split into the draft's U cached steps with their picks, the verify pass
    (``decoder_append`` with the logits of all U + 1 positions; also with f5e_gemm_f32 in place of f5e_gemm_f32_skinny, which is
    what the pass would cost without the new GEMM) and the verify pass plus f5e_whisper_verify / f5e_whisper_accept;
  * the yardstick, measured in the same run: the cached step of the path without an assistant on the same shapes (``_dec_step``
    with logits, and the greedy pick);
  * from these the break-even number of tokens per round (round / step): a round has to keep more than that many tokens to win;
    and the bound at full acceptance (U + 1 tokens per round), which is what a draft equal to the target reaches.  Synthetic
    weights cannot give a real acceptance rate: the real rate is unmeasured;
  * f5e_gemm_f32_skinny beside f5e_gemm_f32 at M = 1, 6, 16 rows on the decoder's five weight shapes (us per launch).

The arms are ALTERNATED in one process, ``--runs`` runs each; a run is the median of ``--repeats`` measurements between device
events after a warm-up of all, and the record keeps every run's median with the smallest and largest measurement
(tools/whisper_prefill_time.py's protocol).  Nothing is gated on these figures.

    python tools/whisper_assist_time.py [--runs 3] [--repeats 5] [--out FILE]
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

F32, I32 = torch.float32, torch.int32
SHAPES = (("qkv", 3840, 1280), ("out / xq / xout", 1280, 1280), ("ff1", 5120, 1280), ("ff2", 1280, 5120), ("vocabulary", 51866, 1280))


def build(name, seed):
    from f5e_tts_amd.eval import whisper as W
    from tools import synth as SY
    cfg = W.WhisperConfig(**SY.whisper_config_fields(name, encoder_layers=1))         # the decoders are what is timed
    with torch.device("cuda"):
        model = W.Whisper(cfg)
    shapes = {k: v.shape for k, v in model.state_dict().items()}
    model.load_state_dict(SY.init_whisper_state(shapes, seed, 4.0, device="cuda"), strict=False)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    kv = []
    for _ in range(cfg.decoder_layers):
        buf = torch.randn(1, cfg.max_source_positions, 2 * cfg.d_model, generator=g, device="cuda")
        kv.append((buf[..., :cfg.d_model], buf[..., cfg.d_model:]))
    return model, kv


def time_rounds(us, runs, repeats, p=64):
    """The pieces of a round at position ``p`` (64 cached positions behind it), and the yardstick."""
    from f5e_tts_amd import ops
    target, kv = build("large-v3", 99)
    draft, dkv = build("large-v3-turbo", 98)
    cfg, fd = target.cfg, target._fold()
    eos, V, Umax = cfg.eos_token_id, cfg.vocab_size, cfg.max_target_positions
    st, dst = target._dec_state(1, Umax, "cuda"), draft._dec_state(1, Umax, "cuda")
    tokens = torch.randint(0, 50000, (1, Umax), device="cuda", dtype=I32)
    last, done, alive, adv = (torch.zeros(1, dtype=I32, device="cuda") for _ in range(4))
    sup = dict(suppress=fd["suppress"], begin_suppress=fd["begin_suppress"])

    def step():                                            # the path without an assistant: one cached step and its pick
        logits = target._dec_step(st, kv, last, p, True)
        ops.greedy_pick(logits, tokens, last, done, alive, p, eos, **sup)
        done.zero_()

    out = []
    for U in us:
        cand, logp = torch.empty(1, U + 1, dtype=I32, device="cuda"), torch.empty(1, U + 1, dtype=F32, device="cuda")
        hist = tokens.clone()

        def drafts():
            for k in range(U):
                logits = draft._dec_step(dst, dkv, last, p + k, True)
                ops.greedy_pick(logits, hist, last, done, alive, p + k, eos, **sup)
            done.zero_()

        def verify():
            return target.decoder_append(st, kv, hist[:, p:p + U + 1], p)

        def verify_gemm_f32():                             # the same pass on the GEMM the prefill uses
            from f5e_tts_amd.eval.whisper import Whisper
            keep = Whisper.__dict__["_append_gemm"]
            Whisper._append_gemm = staticmethod(lambda M, N, K: ops.gemm_f32)
            try:
                return target.decoder_append(st, kv, hist[:, p:p + U + 1], p)
            finally:
                Whisper._append_gemm = keep

        def verify_accept():
            logits = verify()
            ops.whisper_verify(logits.view(U + 1, V), hist, cand, logp, p, 4, eos, None, **sup)
            ops.whisper_accept(cand, logp, hist, tokens, last, done, alive, None, adv, p, eos)
            done.zero_()

        def whole():
            drafts()
            verify_accept()
            return adv.tolist()                            # the round's one synchronisation

        arms = (("step_ms", step), ("draft_steps_ms", drafts), ("verify_pass_ms", verify), ("verify_pass_gemm_f32_ms", verify_gemm_f32),
                ("verify_accept_ms", verify_accept), ("round_ms", whole))
        for _, fn in arms:                                 # warm-up of all
            fn()
        torch.cuda.synchronize()
        rec = dict(target="large-v3", draft="large-v3-turbo", rows=1, position=p, drafted=U, **{k: [] for k, _ in arms})
        for _ in range(runs):
            for key, fn in arms:
                rec[key].append(spread([events_ms(fn) for _ in range(repeats)]))
        med = {k: sorted(r["median"] for r in rec[k])[len(rec[k]) // 2] for k, _ in arms}
        rec["break_even_tokens_per_round"] = med["round_ms"] / med["step_ms"]
        rec["full_acceptance_ms_per_token"] = med["round_ms"] / (U + 1)
        rec["full_acceptance_speedup_bound"] = med["step_ms"] * (U + 1) / med["round_ms"]
        out.append(rec)
        print(json.dumps(rec), flush=True)
    del target, draft, kv, dkv, st, dst
    torch.cuda.empty_cache()
    return out


def time_gemms(runs, repeats, inner=20):
    """us per launch of the two GEMMs on the decoder's weight shapes (``inner`` launches between the events)."""
    from f5e_tts_amd import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    out = []
    for name, N, K in SHAPES:
        w = torch.randn(N, K, generator=g, device="cuda") * K ** -0.5
        bias = torch.randn(N, generator=g, device="cuda")
        for M in (1, 6, 16):
            a = torch.randn(M, K, generator=g, device="cuda")
            y0, y1 = torch.empty(M, (N + 3) // 4 * 4, device="cuda")[:, :N], torch.empty(M, (N + 3) // 4 * 4, device="cuda")[:, :N]

            def plain():
                for _ in range(inner):
                    ops.gemm_f32(a, w, bias, out=y0)

            def skinny():
                for _ in range(inner):
                    ops.gemm_f32_skinny(a, w, bias, out=y1)
            plain(), skinny()
            torch.cuda.synchronize()
            err = float((y0 - y1).abs().max() / y0.abs().max())
            rec = dict(shape=name, N=N, K=K, M=M, k_split_bytes=ops.gemm_f32_skinny_workspace(N, K), max_rel_diff=err, gemm_f32_us=[],
                       gemm_f32_skinny_us=[])
            for _ in range(runs):
                for key, fn in (("gemm_f32_us", plain), ("gemm_f32_skinny_us", skinny)):
                    s = spread([events_ms(fn) * 1000.0 / inner for _ in range(repeats)])
                    rec[key].append(s)
            out.append(rec)
            print(json.dumps(rec), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--drafted", default="2,4,8")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from f5e_tts_amd import ops
    ops.require_device()
    lines = [f"# python tools/whisper_assist_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# fp32, eager launches, synthetic weights and cross keys / values, R = 1; {args.runs} alternated runs, each the median / "
             f"min / max of {args.repeats} repeats; the acceptance rate of a real draft is unmeasured"]
    with torch.no_grad():
        for rec in time_gemms(args.runs, args.repeats):
            lines.append(json.dumps(rec))
        for rec in time_rounds([int(u) for u in args.drafted.split(",") if u], args.runs, args.repeats):
            lines.append(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
