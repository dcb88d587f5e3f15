"""Makes tests/golden/qwen2.npz from ``transformers`` (5.15.0 when this was run): a tiny seeded ``Qwen2ForCausalLM`` -- nothing is
downloaded.

Model: vocab 384, hidden 128, 4 query / 2 key-value heads of 32, intermediate 256, 2 layers, tied embeddings, rope_theta 1e6,
``initializer_range`` 0.08, random q / k / v biases and perturbed norm weights.  Weights are rounded to bf16-representable values
before the model runs and stored as their upper 16 bits (``w/<name>``).

Prompts: two rows of 9 and 5 ids, the second left-padded by 4 (attention mask, position ids from the mask as ``generate`` makes
them).  The pad id is the first real token of the padded row: ``transformers`` applies the repetition penalty to every id of
``input_ids``, the padding included, while the device pick reads a row's own tokens only; with this pad id the two agree.

Stored: the inputs of both layers at every position (``hidden_i``), the last position's logits of the prefill, 16 greedy tokens per
row from ``generate(do_sample=False, repetition_penalty=1.05)`` with the top-1 / top-2 gap of every step's processed scores, the
B = 1 greedy runs of both rows (asserted equal to the batch's), the logits after a second "turn" of 6 more ids behind row 0's
prompt and its 16 tokens, and 64 rows of the rotary module's cos / sin.

The seed is the first of ``SEEDS`` for which every recorded gap is >= 1e-2 and at least 8 distinct tokens occur in each row.

    python tests/golden/make_qwen2_golden.py
"""
import json
import os

import numpy as np
import torch

SEEDS = tuple(range(1, 201))
N_NEW, PENALTY, GAP, DISTINCT = 16, 1.05, 1e-2, 8
CFG = dict(vocab_size=384, hidden_size=128, num_attention_heads=4, num_key_value_heads=2, intermediate_size=256,
           num_hidden_layers=2, tie_word_embeddings=True, initializer_range=0.08, rope_theta=1000000.0,
           max_position_embeddings=128, rms_norm_eps=1e-6)


def build(seed):
    from transformers import Qwen2Config, Qwen2ForCausalLM
    torch.manual_seed(seed)
    cfg = Qwen2Config(**CFG, attn_implementation="eager", eos_token_id=None, pad_token_id=None, bos_token_id=None)
    model = Qwen2ForCausalLM(cfg).eval().float()
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("proj.bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.08)
            elif name.endswith("norm.weight") or name.endswith("layernorm.weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            p.copy_(p.to(torch.bfloat16).float())
    model.generation_config.eos_token_id = None
    model.generation_config.pad_token_id = None
    return model


def prompts(seed):
    g = np.random.RandomState(seed)
    a, b = g.randint(0, 381, size=9).tolist(), g.randint(0, 381, size=5).tolist()
    turn2 = g.randint(0, 381, size=6).tolist()
    return a, b, turn2


def greedy(model, ids, mask, pad):
    out = model.generate(ids, attention_mask=mask, do_sample=False, repetition_penalty=PENALTY, max_new_tokens=N_NEW,
                         pad_token_id=pad, output_scores=True, return_dict_in_generate=True)
    toks = out.sequences[:, ids.shape[1]:]
    gaps = []
    for s in out.scores:
        top = s.float().topk(2, dim=-1).values
        gaps.append((top[:, 0] - top[:, 1]))
    return toks, torch.stack(gaps, 1)


def attempt(seed):
    model = build(seed)
    a, b, turn2 = prompts(seed)
    pad = b[0]
    ids = torch.tensor([a, [pad] * 4 + b])
    mask = torch.tensor([[1] * 9, [0] * 4 + [1] * 5])
    pos = (mask.cumsum(-1) - 1).clamp(min=0)
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=mask, position_ids=pos, output_hidden_states=True)
        toks, gaps = greedy(model, ids, mask, pad)
        t0, g0 = greedy(model, ids[:1], mask[:1], pad)
        t1, g1 = greedy(model, torch.tensor([b]), torch.ones(1, 5, dtype=torch.long), pad)
        full = torch.tensor([a + toks[0].tolist() + turn2])
        turn2_logits = model(input_ids=full).logits[0, -1]
        cos, sin = model.model.rotary_emb(out.logits, torch.arange(64)[None])
    ok = float(min(gaps.min(), g0.min(), g1.min())) >= GAP and all(len(set(r.tolist())) >= DISTINCT for r in toks) \
        and torch.equal(t0[0], toks[0]) and torch.equal(t1[0], toks[1])
    if not ok:
        return None
    half = CFG["hidden_size"] // CFG["num_attention_heads"] // 2
    assert torch.equal(cos[0, :, :half], cos[0, :, half:]) and torch.equal(sin[0, :, :half], sin[0, :, half:])
    fx = dict(seed=np.int64(seed), cfg=np.array(json.dumps(CFG)), ids=ids.numpy().astype(np.int32), begin=np.array([0, 4], np.int32),
              pad=np.int32(pad), logits=out.logits[:, -1].numpy(), tokens=toks.numpy().astype(np.int32), gaps=gaps.numpy(),
              turn2_ids=np.array(turn2, np.int32), turn2_logits=turn2_logits.numpy(), cos=cos[0, :, :half].numpy(),
              sin=sin[0, :, :half].numpy())
    for i in range(CFG["num_hidden_layers"]):
        fx[f"hidden_{i}"] = out.hidden_states[i].numpy()
    for name, p in model.state_dict().items():
        if name == "lm_head.weight":
            continue
        bits = p.detach().float().contiguous().view(torch.int32).numpy()
        assert not (bits & 0xffff).any(), name
        fx["w/" + name] = (bits >> 16).astype(np.uint16)
    return fx


def main():
    for seed in SEEDS:
        fx = attempt(seed)
        if fx is None:
            continue
        assert float(fx["gaps"].min()) >= GAP and all(len(set(r.tolist())) >= DISTINCT for r in fx["tokens"])
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "qwen2.npz")
        np.savez(path, **fx)
        print(f"seed {seed}: min gap {fx['gaps'].min():.3e}, distinct {[len(set(r.tolist())) for r in fx['tokens']]}, "
              f"{os.path.getsize(path)} bytes")
        return
    raise SystemExit("no seed meets the conditions")


if __name__ == "__main__":
    main()
