"""Times Whisper's timestamp decoding (eval/whisper.py, csrc/whisper.hip):
  * us per step of f5e_whisper_ts_pick (the ruled greedy pick, both launches) against f5e_greedy_pick on the same [R, 51866]
    logits: the unruled pick is the yardstick for what the rules cost;
  * us of f5e_whisper_beam_step_ts against f5e_whisper_beam_step on [K, 51866] logits (the pre-pass and the extra mask);
  * wall ms of ``transcribe_long`` on one 90 s recording at the whisper-large-v3-turbo shape with synthetic weights
    (tools/synth.py), greedy and with 5 beams, with the windows and segments it produced (synthetic weights emit what they emit:
    the figure is the cost of that many windows, not of a transcript).
Device events around work on one stream after a warm-up; every figure is the median of ``--repeats`` measurements, with their
smallest and largest.  Nothing is gated on these figures.

    python tools/whisper_long_time.py [--model large-v3-turbo] [--seconds 90] [--beam 5] [--repeats 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.src_hash import csrc_sha256  # noqa: E402
from tools.whisper_beam_time import BeamState, events_ms, spread  # noqa: E402

F32, I32 = torch.float32, torch.int32
NO_TS, EOS = 50364, 50257


def pick_us(V, R, repeats, reps=200):
    """The two greedy picks on the same logits, mid-sequence (history: <|0.00|> and five text tokens), no row done."""
    from f5e_tts_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(3)
    logits = (4.0 * torch.randn(R, (V + 3) // 4 * 4, generator=g)).to(dev)[:, :V]
    n0, p = 3, 8
    tokens = torch.full((R, 64), 11, dtype=I32, device=dev)
    tokens[:, n0] = NO_TS + 1
    last, done, alive = (torch.zeros(n, dtype=I32, device=dev) for n in (R, R, 1))
    slp = torch.zeros(R, dtype=F32, device=dev)
    sup = torch.arange(100, 190, dtype=I32, device=dev)

    def plain():
        ops.greedy_pick(logits, tokens, last, done, alive, p, EOS, suppress=sup)

    def ruled():
        ops.whisper_ts_pick(logits, tokens, last, done, alive, slp, p, n0, EOS, NO_TS, suppress=sup, max_initial=50)
    out = {}
    for name, fn in (("greedy_pick_us", plain), ("whisper_ts_pick_us", ruled)):
        fn()
        done.zero_()
        torch.cuda.synchronize()
        out[name] = spread([1e3 * events_ms(lambda: [fn() for _ in range(reps)]) / reps for _ in range(repeats)])
    return out


def beam_us(V, K, repeats, reps=200):
    from f5e_tts_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(3)
    logits = (4.0 * torch.randn(K, (V + 3) // 4 * 4, generator=g)).to(dev)[:, :V]
    U, p, n0 = 64, 20, 3
    bs = BeamState(1, K, V, U, EOS, dev)
    for h in bs.hyp:
        h.fill_(5)
        h[:, n0] = NO_TS + 1
    live = -torch.rand(K, generator=g).to(dev)
    sup = torch.arange(100, 190, dtype=I32, device=dev)
    desc = torch.zeros(K, 4, dtype=I32, device=dev)

    def step(ruled):
        bs.score.copy_(live)
        bs.open.fill_(1)
        c = bs.cur
        args = (logits, bs.score, bs.hyp[c], bs.anc[c], bs.hyp[1 - c], bs.anc[1 - c], bs.last, bs.pool_hyp, bs.pool_len, bs.pool_score,
                bs.pool_n, bs.open, bs.alive, p, n0, U, EOS, K)
        if ruled:
            ops.whisper_beam_step_ts(*args, NO_TS, desc, max_initial=50, suppress=sup, scratch=bs.scratch)
        else:
            ops.whisper_beam_step(*args, suppress=sup, scratch=bs.scratch)
    out = {}
    for name, ruled in (("whisper_beam_step_us", False), ("whisper_beam_step_ts_us", True)):
        step(ruled)
        torch.cuda.synchronize()
        out[name] = spread([1e3 * events_ms(lambda: [step(ruled) for _ in range(reps)]) / reps for _ in range(repeats)])
    return out


class _Enough(Exception):
    pass


def long_ms(name, seconds, K, repeats, max_windows=12):
    from f5e_tts_amd.eval import whisper as W
    from tools import synth as SY
    cfg = W.WhisperConfig(**SY.whisper_config_fields(name, max_initial_timestamp_index=50))
    with torch.device("cuda"):
        model = W.Whisper(cfg)
    shapes = {k: v.shape for k, v in model.state_dict().items()}
    model.load_state_dict(SY.init_whisper_state(shapes, 99, 4.0, device="cuda"), strict=False)
    wav = SY.synthetic_ref_wave(100 * seconds, seed=5, hop=160).cuda()
    rec = dict(model=name, seconds=seconds, decoder_layers=cfg.decoder_layers)
    # synthetic weights may emit early timestamps window after window: the run is stopped after ``max_windows`` windows, and the
    # record says so (``finished``)
    windows, decode = [], model.generate_from_kv

    def counted(*a, **kw):
        if len(windows) >= max_windows:
            raise _Enough()
        windows.append(kw["stats"])
        return decode(*a, **kw)
    model.generate_from_kv = counted

    def run(beam):
        del windows[:]
        try:
            model.transcribe_long(wav, language="en", beam_size=beam)
            done = True
        except _Enough:
            done = False
        torch.cuda.synchronize()
        return done
    for beam in (1, K):
        finished = run(beam)                                                             # warm-up, and what it did
        n_windows, wall = len(windows), []
        for _ in range(repeats):
            t0 = time.perf_counter()
            run(beam)
            wall.append(1e3 * (time.perf_counter() - t0))
        rec[f"beam{beam}"] = dict(wall_ms=spread(wall), windows=n_windows, finished=finished)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="large-v3-turbo")
    ap.add_argument("--seconds", type=int, default=90)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from f5e_tts_amd import ops
    ops.require_device()
    lines = [f"# python tools/whisper_long_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# synthetic weights, fp32, eager launches; median / min / max of {args.repeats} repeats"]
    with torch.no_grad():
        for R in (1, 8):
            lines.append(json.dumps(dict(pick_at_V=51866, rows=R, **pick_us(51866, R, args.repeats))))
            print(lines[-1], flush=True)
        lines.append(json.dumps(dict(beam_at_V=51866, beam=args.beam, **beam_us(51866, args.beam, args.repeats))))
        print(lines[-1], flush=True)
        lines.append(json.dumps(long_ms(args.model, args.seconds, args.beam, args.repeats)))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
