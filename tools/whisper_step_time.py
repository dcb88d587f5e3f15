"""Times Whisper's captured decode step (``generate_from_kv(step_graph=True)``) against the eager step at the
large-v3 and large-v3-turbo decoder shapes, synthetic weights and random cross keys / values of 1500 positions, B = 1 and B = 5
rows, 64 greedy picks behind a prompt of 4 tokens:

  * ``eager``: ``_dec_step`` and ``ops.greedy_pick`` per token, the launches of the path without ``step_graph`` (this is the
    yardstick: the feature does not change that code);
  * ``graph``: one launch of the captured step per token (``step_gemm="f32"``: the same kernels from a hipGraph);
  * ``graph_skinny``: the same with ``step_gemm="skinny"``.

The three arms are ALTERNATED in one process; a measurement is the 64-token loop between two device events, ended by a
synchronise; the record keeps the median, the smallest and the largest of ``--repeats`` measurements per arm (after a warm-up of
all), as ms per token.  Also, once per shape and arm: the host time of capture + instantiate (``_step_capture``, wall clock
around it with a synchronise before), and the number of tokens after which a capture has paid for itself,
capture / (eager - graph) per token.  Nothing is gated on these figures.

    python tools/whisper_step_time.py [--repeats 5] [--tokens 64] [--out FILE]
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
from tools.whisper_beam_time import events_ms, spread  # noqa: E402

F32, I32 = torch.float32, torch.int32
N0 = 4


def build(name, B, seed, weights="f32"):
    from f5e_tts_amd.eval import whisper as W
    from tools import synth as SY
    cfg = W.WhisperConfig(**SY.whisper_config_fields(name, encoder_layers=1))         # the decoder is what is timed
    with torch.device("cuda"):
        model = W.Whisper(cfg, weights=weights)
    shapes = {k: v.shape for k, v in model.state_dict().items()}
    model.load_state_dict(SY.init_whisper_state(shapes, seed, 4.0, device="cuda"), strict=False)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    kv = []
    for _ in range(cfg.decoder_layers):
        buf = torch.randn(B, cfg.max_source_positions, 2 * cfg.d_model, generator=g, device="cuda")
        kv.append((buf[..., :cfg.d_model], buf[..., cfg.d_model:]))
    return model, kv


def time_shape(name, B, tokens, repeats, weights="f32", inspect=None):
    from f5e_tts_amd import ops
    model, kv = build(name, B, 99, weights)
    cfg, fd = model.cfg, model._fold()
    eos, P = cfg.eos_token_id, cfg.max_target_positions
    sup = dict(suppress=fd["suppress"], begin_suppress=fd["begin_suppress"])
    prompt = torch.randint(0, 50000, (B, N0), device="cuda", dtype=I32)

    def feed(st, kv_, last, table):                        # the prompt's forced steps: the caches of positions 0 .. N0 - 2
        table[:, :N0] = prompt
        for p in range(N0 - 1):
            last.copy_(table[:, p])
            model._dec_step(st, kv_, last, p, False)
        last.copy_(table[:, N0 - 1])

    # the eager arm's buffers, as generate_from_kv allocates them
    st = model._dec_state(B, P, "cuda")
    table = torch.full((B, P), eos, dtype=I32, device="cuda")
    last, done, alive = torch.zeros(B, dtype=I32, device="cuda"), torch.zeros(B, dtype=I32, device="cuda"), \
        torch.zeros(1, dtype=I32, device="cuda")
    feed(st, kv, last, table)

    def eager():
        for p in range(N0 - 1, N0 - 1 + tokens):
            logits = model._dec_step(st, kv, last, p, True)
            ops.greedy_pick(logits, table, last, done, alive, p, eos, first_step=p + 1 == N0, **sup)

    arms, capture_ms, states = {"eager": eager}, {}, {}
    for arm, gemm in (("graph", "f32"), ("graph_skinny", "skinny")):
        S = model._step_state(B, "greedy", False, gemm, cfg.max_source_positions, torch.device("cuda", torch.cuda.current_device()))
        model._step_load(S, kv)
        S.tokens.fill_(eos)
        feed(S.st, S.kv, S.last, S.tokens)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model._step_capture(S, False)
        capture_ms[arm] = (time.perf_counter() - t0) * 1e3
        states[arm] = S

        def replay(S=S):
            for _ in range(tokens):
                S.graph.launch()
        arms[arm] = replay

    def reset():                                           # outside the events: every measurement starts at the prompt's end
        done.zero_()
        last.copy_(table[:, N0 - 1])
        for S in states.values():
            S.done.zero_()
            S.last.copy_(S.tokens[:, N0 - 1])
            S.rec.copy_(ops.whisper_step_record(N0 - 1, N0))
        torch.cuda.synchronize()

    for fn in arms.values():                               # warm-up of all
        reset()
        fn()
    torch.cuda.synchronize()
    same = torch.equal(states["graph"].tokens[:, :N0 + tokens], table[:, :N0 + tokens])
    ms = {arm: [] for arm in arms}
    for _ in range(repeats):
        for arm, fn in arms.items():
            reset()
            ms[arm].append(events_ms(fn) / tokens)
    rec = dict(model=name, rows=B, tokens=tokens, prompt=N0, graph_tokens_equal_eager=bool(same),
               skinny_tokens_equal_eager=bool(torch.equal(states["graph_skinny"].tokens[:, :N0 + tokens], table[:, :N0 + tokens])),
               state_bytes={arm: sum(t.numel() * t.element_size() for t in S.xkv) +
                            sum(k.numel() * 8 for k, _ in S.st["caches"]) for arm, S in states.items()},
               ms_per_token={arm: spread(v) for arm, v in ms.items()}, capture_instantiate_ms=capture_ms)
    e = rec["ms_per_token"]["eager"]["median"]
    rec["speedup_over_eager"] = {arm: e / rec["ms_per_token"][arm]["median"] for arm in states}
    rec["break_even_tokens"] = {arm: (capture_ms[arm] / (e - rec["ms_per_token"][arm]["median"])
                                      if e > rec["ms_per_token"][arm]["median"] else None) for arm in states}
    if inspect is not None:                                # a caller's own fields, read off the model that was timed
        rec.update(inspect(model))
    del model, kv, st, states, arms
    torch.cuda.empty_cache()
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--models", default="large-v3,large-v3-turbo")
    ap.add_argument("--rows", default="1,5")
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from f5e_tts_amd import ops
    ops.require_device()
    lines = [f"# python tools/whisper_step_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# fp32, synthetic weights and cross keys / values, {args.tokens} greedy picks behind a prompt of {N0}; three arms "
             f"alternated in one process, ms per token: median / min / max of {args.repeats} measurements between device events"]
    with torch.no_grad():
        for name in args.models.split(","):
            for B in (int(b) for b in args.rows.split(",")):
                rec = time_shape(name, B, args.tokens, args.repeats)
                print(json.dumps(rec), flush=True)
                lines.append(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
