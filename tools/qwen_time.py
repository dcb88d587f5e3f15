"""Times the Qwen2 path at the Qwen2.5-3B shapes with seeded bf16 weights, B = 1: 36 layers, D 2048, 16 / 2 heads of
128, I 11008, V 151936, tied.

  * ms per token of the decode step, eager and from the captured step, at cache lengths 64 / 1024 / 4000, with the per-token
    weight bytes over the step time beside it (every matrix is read once per token: the floor is weight bytes / HBM rate);
  * ms of a 256-token prefill;
  * the decode attention launch alone: us and GB/s of cache read (K and V of the key/value heads, p positions, fp32).

Method: HIP events around ``--steps`` consecutive steps after ``--warm`` warm ones, repeated ``--repeats`` times; the table
holds the median and the min .. max spread over the repeats.  Nothing is gated.

    python tools/qwen_time.py [--layers 36] [--out profiles/qwen_time.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(layers: int, seed: int = 0):
    from f5e_tts_amd.infer.qwen2 import Qwen2, Qwen2Config
    cfg = Qwen2Config(vocab_size=151936, hidden_size=2048, num_hidden_layers=layers, num_attention_heads=16, num_key_value_heads=2,
                      intermediate_size=11008, tie_word_embeddings=True)
    g = torch.Generator(device="cuda").manual_seed(seed)
    D, I, dk = 2048, 11008, 128

    def w(*shape, scale=0.02):
        return (torch.randn(*shape, generator=g, device="cuda") * scale).to(torch.bfloat16)
    sd = {"model.embed_tokens.weight": w(151936, D), "model.norm.weight": torch.ones(D, device="cuda")}
    for i in range(layers):
        p = f"model.layers.{i}."
        for n, h in (("q", 16), ("k", 2), ("v", 2)):
            sd[p + f"self_attn.{n}_proj.weight"], sd[p + f"self_attn.{n}_proj.bias"] = w(h * dk, D), w(h * dk).float()
        sd[p + "self_attn.o_proj.weight"] = w(D, 16 * dk)
        sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"], sd[p + "mlp.down_proj.weight"] = w(I, D), w(I, D), w(D, I)
        sd[p + "input_layernorm.weight"] = sd[p + "post_attention_layernorm.weight"] = torch.ones(D, device="cuda")
    return Qwen2(cfg, "bf16").load_state_dict(sd)


def timed(fn, steps: int, warm: int, repeats: int, before=None):
    out = []
    for _ in range(repeats):
        if before is not None:
            before()
        for _ in range(warm):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    from types import SimpleNamespace

    from f5e_tts_amd import ops
    m = build(a.layers)
    cfg = m.cfg
    sm = SimpleNamespace(do_sample=True, temperature=0.7, top_k=20, top_p=0.95, penalty=1.05)
    eos, pad = [151645, 151643], 151643
    S = m.new_state(1, 4096)
    S.tokens.random_(0, 151936, generator=torch.Generator(device="cuda").manual_seed(1))
    weight_bytes = sum(t.numel() * t.element_size() for L in m.layers for t in (L.wqkv, L.wo, L.wgu, L.wdown)) + \
        m.lm_head.numel() * m.lm_head.element_size()
    lines = [f"Qwen2 path at the Qwen2.5-3B shapes, {a.layers} layers, B = 1, bf16 weights ({weight_bytes / 1e9:.2f} GB read per token), "
             f"{torch.cuda.get_device_name(0)}",
             f"method: HIP events around {a.steps} steps after {a.warm} warm ones; median (min .. max) of {a.repeats} repeats", ""]

    def arm(p):
        def go():
            S.rec.copy_(ops.whisper_step_record(p, 1, 0))
            S.done.zero_()
        return go
    m._capture(S, sm, eos, pad)
    for p in (64, 1024, 4000):
        e = timed(lambda: m._step(S, sm, eos, pad), a.steps, a.warm, a.repeats, arm(p))
        g = timed(S.graph.launch, a.steps, a.warm, a.repeats, arm(p))
        lines.append(f"decode step at cache length {p:5d}: eager {e[0]:7.3f} ms ({e[1]:.3f} .. {e[2]:.3f}), captured {g[0]:7.3f} ms "
                     f"({g[1]:.3f} .. {g[2]:.3f}) = {weight_bytes / g[0] / 1e6:7.1f} GB/s of weights")
    ids = S.tokens[:, :256].contiguous()
    pf = timed(lambda: m.append(S, ids, 0), 1, 1, a.repeats)
    lines.append(f"prefill of 256 tokens: {pf[0]:.2f} ms ({pf[1]:.2f} .. {pf[2]:.2f})")
    H, Hkv, dk = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    qkv = torch.randn(1, (H + 2 * Hkv) * dk, device="cuda")
    out = torch.empty(1, H * dk, device="cuda")
    for p in (64, 1024, 4000):
        rec = ops.whisper_step_record(p, 1, 0).cuda()
        t = timed(lambda: ops.gqa_rope_decode_dev_f32(qkv, S.kc[0], S.vc[0], m.cos, m.sin, rec, H, Hkv, dk ** -0.5, out=out), 50, 10,
                  a.repeats)
        nbytes = 2 * (p + 1) * Hkv * dk * 4
        lines.append(f"decode attention alone at p = {p:5d}: {t[0] * 1e3:7.1f} us ({t[1] * 1e3:.1f} .. {t[2] * 1e3:.1f}) = "
                     f"{nbytes / t[0] / 1e6:6.1f} GB/s of cache read (eager launches: the time includes the host's launch cost)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
