"""Times Whisper's beam search step (eval/whisper.py, f5e_whisper_beam_step) at the whisper-large-v3 and -large-v3-turbo shapes with
synthetic weights (tools/synth.py), one 30 s utterance:
  * ms per decode step (all layers, logits GEMM, selection) at K = 5 against the greedy step at R = 1 and at R = 5 rows;
  * us of f5e_whisper_beam_step alone (both launches) on [K, 51866] logits, and of f5e_beam_step on the same logits: the
    one-wave-per-row selection that makes one pass over a row per kept candidate, as the yardstick for the one-pass selection
    (its semantics differ -- K candidates per row, finished rows inside the beam -- only its reading pattern is compared).
Device events around work on one stream after a warm-up; every figure is the median of ``--repeats`` measurements, with their
smallest and largest.  Nothing is gated on these figures.

    python tools/whisper_beam_time.py [--models large-v3,large-v3-turbo] [--tokens 24] [--beam 5] [--repeats 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.src_hash import csrc_sha256  # noqa: E402

F32, I32 = torch.float32, torch.int32


def events_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def spread(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values))


class BeamState:
    """The buffers of one search of B utterances, as Whisper._beam_from_kv allocates them."""

    def __init__(self, B, K, V, U, eos, dev):
        from f5e_tts_amd import ops
        R = B * K
        self.hyp = [torch.full((R, U), eos, dtype=I32, device=dev) for _ in range(2)]
        self.anc = [torch.arange(R, dtype=I32, device=dev)[:, None].repeat(1, U) for _ in range(2)]
        self.last = torch.zeros(R, dtype=I32, device=dev)
        self.score0 = torch.full((B, K), -float("inf"), dtype=F32, device=dev)
        self.score0[:, 0] = 0.0
        self.score = self.score0.view(R).clone()
        self.pool_hyp = torch.full((B, K, U), eos, dtype=I32, device=dev)
        self.pool_len = torch.zeros(B, K, dtype=I32, device=dev)
        self.pool_score = torch.full((B, K), -float("inf"), dtype=F32, device=dev)
        self.pool_n, self.open, self.alive = (torch.full((B,), v, dtype=I32, device=dev) for v in (0, 1, 1))
        self.scratch = torch.empty(ops.whisper_beam_scratch(B, K, V), dtype=torch.uint8, device=dev)
        self.cur = 0

    def step(self, ops, logits, p, n0, cap, eos, K, fd):
        c = self.cur
        ops.whisper_beam_step(logits, self.score, self.hyp[c], self.anc[c], self.hyp[1 - c], self.anc[1 - c], self.last,
                              self.pool_hyp, self.pool_len, self.pool_score, self.pool_n, self.open, self.alive, p, n0, cap, eos, K,
                              suppress=fd["suppress"], begin_suppress=fd["begin_suppress"], scratch=self.scratch)
        self.cur = 1 - c


def beam_decode_ms(model, kv, prompt, n_tokens, K):
    """Milliseconds per beam step (K rows through all layers, logits, selection) over ``n_tokens`` steps after the prompt."""
    from f5e_tts_amd import ops
    cfg, fd, dev = model.cfg, model._fold(), kv[0][0].device
    n0, U = len(prompt), len(prompt) + n_tokens + 1
    st = model._dec_state(K, U, dev)
    bs = BeamState(1, K, cfg.vocab_size, U, cfg.eos_token_id, dev)
    for h in bs.hyp:
        h[:, :n0] = torch.tensor(prompt, dtype=I32, device=dev)
    bs.last.copy_(bs.hyp[0][:, 0])

    def steps(lo, hi):
        for p in range(lo, hi):
            logits = model._dec_step(st, kv, bs.last, p, p + 1 >= n0, anc=bs.anc[bs.cur])
            if p + 1 < n0:
                bs.last.copy_(bs.hyp[0][:, p + 1])
            else:
                bs.step(ops, logits, p, n0, U, cfg.eos_token_id, K, fd)         # the cap is never reached: every step a full step
    steps(0, n0)                                                                # the prompt and the first pick: warm-up
    torch.cuda.synchronize()
    ms = events_ms(lambda: steps(n0, U - 2)) / (U - 2 - n0)
    return ms, int((bs.score > -float("inf")).sum())


def greedy_decode_ms(model, kv, prompt, n_tokens, R):
    """The greedy step of tools/whisper_time.py on R rows of the one utterance (``rows_per_utt`` = R)."""
    from f5e_tts_amd import ops
    cfg, fd, dev = model.cfg, model._fold(), kv[0][0].device
    U = len(prompt) + n_tokens + 1
    st = model._dec_state(R, U, dev)
    tokens = torch.full((R, U), cfg.eos_token_id, dtype=I32, device=dev)
    tokens[:, :len(prompt)] = torch.tensor(prompt, dtype=I32, device=dev)
    last = tokens[:, 0].clone()
    done, alive = torch.zeros(R, dtype=I32, device=dev), torch.zeros(1, dtype=I32, device=dev)

    def steps(lo, hi):
        for p in range(lo, hi):
            logits = model._dec_step(st, kv, last, p, True)
            done.zero_()
            ops.greedy_pick(logits, tokens, last, done, alive, p, cfg.eos_token_id, suppress=fd["suppress"],
                            begin_suppress=fd["begin_suppress"], first_step=False)
    steps(0, len(prompt))
    torch.cuda.synchronize()
    return events_ms(lambda: steps(len(prompt), U - 2)) / (U - 2 - len(prompt))


def selection_us(V, K, repeats, reps=200):
    """f5e_whisper_beam_step and f5e_beam_step alone on the same [K, V] logits, all K rows live, mid-search."""
    from f5e_tts_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(3)
    logits = (4.0 * torch.randn(K, (V + 3) // 4 * 4, generator=g)).to(dev)[:, :V]
    eos, U, p, n0 = V - 1, 64, 20, 4
    bs = BeamState(1, K, V, U, eos, dev)
    for h in bs.hyp:
        h.fill_(5)                                                 # no row ends in eos: f5e_beam_step scans every row
    live = -torch.rand(K, generator=g).to(dev)
    fd = dict(suppress=torch.arange(100, 190, dtype=I32, device=dev), begin_suppress=None)

    def new():
        bs.score.copy_(live)
        bs.open.fill_(1)
        bs.step(ops, logits, p, n0, U, eos, K, fd)
    alive2, done_at = torch.zeros(1, dtype=I32, device=dev), torch.full((1,), -1, dtype=I32, device=dev)
    score2 = live.clone()

    def old():
        score2.copy_(live)
        ops.beam_step(logits, score2, bs.hyp[0], bs.anc[0], bs.hyp[1], bs.anc[1], bs.last, alive2, done_at, p, K, eos)

    def copy_only():
        score2.copy_(live)
    out = {}
    for name, fn in (("whisper_beam_step_us", new), ("beam_step_us", old), ("score_reset_us", copy_only)):
        fn()
        torch.cuda.synchronize()
        out[name] = spread([1e3 * events_ms(lambda: [fn() for _ in range(reps)]) / reps for _ in range(repeats)])
    return out


def run_model(name, n_tokens, K, repeats):
    from f5e_tts_amd.eval import whisper as W
    from tools import synth as SY
    cfg = W.WhisperConfig(**SY.whisper_config_fields(name))
    with torch.device("cuda"):
        model = W.Whisper(cfg)
    shapes = {k: v.shape for k, v in model.state_dict().items()}
    model.load_state_dict(SY.init_whisper_state(shapes, 99, 4.0, device="cuda"), strict=False)
    wav = SY.synthetic_ref_wave(3000, seed=5, hop=160).cuda()           # 30 s
    kv = model.encode(wav)
    prompt = model.prompt_ids("en")
    rec = dict(model=name, decoder_layers=cfg.decoder_layers, beam=K, tokens=n_tokens)
    beam = [beam_decode_ms(model, kv, prompt, n_tokens, K) for _ in range(repeats)]
    rec["beam_step_ms"], rec["open_rows_at_the_end"] = spread([b[0] for b in beam]), beam[-1][1]
    rec["greedy_step_ms_r1"] = spread([greedy_decode_ms(model, kv, prompt, n_tokens, 1) for _ in range(repeats)])
    rec[f"greedy_step_ms_r{K}"] = spread([greedy_decode_ms(model, kv, prompt, n_tokens, K) for _ in range(repeats)])
    del model, kv
    torch.cuda.empty_cache()
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--models", default="large-v3,large-v3-turbo")
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from f5e_tts_amd import ops
    ops.require_device()
    lines = [f"# python tools/whisper_beam_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# one 30 s utterance, synthetic weights, fp32, eager launches, device events; median / min / max of {args.repeats} repeats"]
    with torch.no_grad():
        lines.append(json.dumps(dict(selection_at_V=51866, beam=args.beam, **selection_us(51866, args.beam, args.repeats))))
        print(lines[-1], flush=True)
        for name in [m for m in args.models.split(",") if m]:
            lines.append(json.dumps(run_model(name, args.tokens, args.beam, args.repeats)))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
