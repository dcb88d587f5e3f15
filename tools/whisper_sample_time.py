"""Times Whisper's sampled step (f5e_whisper_sample_pick, csrc/whisper.hip) against the ruled greedy pick it extends
(f5e_whisper_ts_pick, the yardstick) on the same [R, 51866] logits, mid-sequence, no row done: us per step, both launches of each.
The two are ALTERNATED in one process (ruled, sampled, ruled, sampled, ...), ``--runs`` runs each; a run is the median of
``--repeats`` measurements of 200 steps between device events after a warm-up, and the record keeps every run's median with the
smallest and largest measurement, so the spread between runs shows beside the spread inside one.  Nothing is gated on these
figures.

    python tools/whisper_sample_time.py [--runs 3] [--repeats 5] [--out FILE]
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
NO_TS, EOS = 50364, 50257


def pick_us(V, R, T, runs, repeats, reps=200):
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
    row_key, serial = torch.arange(R, dtype=I32, device=dev), torch.zeros(R, dtype=I32, device=dev)

    def ruled():
        ops.whisper_ts_pick(logits, tokens, last, done, alive, slp, p, n0, EOS, NO_TS, suppress=sup, max_initial=50)

    def sampled():
        ops.whisper_sample_pick(logits, tokens, last, done, alive, slp, p, n0, EOS, NO_TS, T, 1234, row_key, serial, suppress=sup,
                                max_initial=50)
    out = {"whisper_ts_pick_us": [], "whisper_sample_pick_us": []}
    for fn in (ruled, sampled):
        fn()
        done.zero_()
    torch.cuda.synchronize()
    for _ in range(runs):
        for name, fn in (("whisper_ts_pick_us", ruled), ("whisper_sample_pick_us", sampled)):
            out[name].append(spread([1e3 * events_ms(lambda: [fn() for _ in range(reps)]) / reps for _ in range(repeats)]))
    # the counters do not move, so every step draws the same class: no row may have ended, or the later steps timed done rows
    assert int(done.sum().item()) == 0, "a pick was eos: the rows turned into done rows"
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--temperature", type=float, default=0.6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from f5e_tts_amd import ops
    ops.require_device()
    lines = [f"# python tools/whisper_sample_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# fp32, eager launches; {max(args.runs, 2)} alternated runs, each the median / min / max of {args.repeats} repeats of "
             f"200 steps"]
    with torch.no_grad():
        for R in (1, 8):
            lines.append(json.dumps(dict(pick_at_V=51866, rows=R, temperature=args.temperature,
                                         **pick_us(51866, R, args.temperature, max(args.runs, 2), args.repeats))))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
