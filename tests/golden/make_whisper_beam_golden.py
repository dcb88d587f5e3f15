"""Makes tests/golden/whisper_beam.npz from ``transformers`` (5.15.0 when this was run): the tiny seeded
``WhisperForConditionalGeneration`` of make_whisper_golden.py, searched with ``GenerationMixin.generate(num_beams=5,
num_return_sequences=5, length_penalty=1.0, early_stopping=False, do_sample=False)`` -- nothing is downloaded, data only.

A case is (seed, audio prefix, eos-row factor, cap): the model of that seed with the ``<|endoftext|>`` row of its tied embedding
scaled by the factor (as the greedy fixture's ``eos`` case does), the first ``prefix`` samples of the greedy fixture's wave, and
``max_length = cap``.  Stored per case: the encoder's output (the search is the decoder's; the GPU tests start from it), all K
pool sequences with their lengths and ``sequences_scores``, the greedy sequence of the same model, the number of steps the
search took and its smallest deciding gap.  Each case's best sequence is cross-checked here against the Whisper wrapper's own
``generate(num_beams=5)``, and all K against the float64 restatement tests/whisper_beam_ref.py (sequences equal, scores within
1e-4).  Only the decoders' weights are stored (bf16 bits), for at most two seeds.

Asserted for every stored case: the smallest gap over all steps (float64; between neighbours of the top 2K + 1 candidates, between
neighbouring pool scores, and |best open row / length - worst pool score| whenever the pool is full) is at least 1e-3 nats, 100x
what the device path drifts.  Asserted over the set:
  (a) one case runs into a cap of n0 + 12;
  (b) one case is closed by the pool-is-good-enough rule before the cap, with pool entries of at least two different lengths;
  (c) at least two cases whose best hypothesis differs from the greedy sequence;
  (d) one case of at least 12 steps before it closes.
The seeds are searched in order; the first seed, or else the first pair of seeds, whose cases cover (a) - (d) is taken.

    python tests/golden/make_whisper_beam_golden.py
"""
import copy
import itertools
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_whisper_golden as G   # noqa: E402
import whisper_beam_ref as BR     # noqa: E402

K = 5
SEEDS = tuple(range(1, 65))
FACTORS = (1.0, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0)
GAP = 1e-3
PROMPT = [G.SOT, G.EN, G.TRANSCRIBE, G.NOTIMESTAMPS]
SHORT_CAP = len(PROMPT) + 12


class HfRef:
    """What ``beam_search_ref`` needs of a model: the last position's logits of a prefix, here from the float64 copy of the
    ``transformers`` model itself."""

    def __init__(self, model):
        self.model = model

    def w(self, name):
        return self.model.state_dict()[name]

    def decoder_logits(self, enc, ids):
        with torch.no_grad():
            return self.model(encoder_outputs=(enc,), decoder_input_ids=torch.tensor(np.asarray(ids))[None]).logits[0].numpy()


def set_eos_row(model, base_row, fac):
    with torch.no_grad():
        model.model.decoder.embed_tokens.weight[G.EOS] = (base_row * fac).bfloat16().float()


def greedy(ref, enc, cap):
    ids = list(PROMPT)
    while len(ids) < cap:
        lg = ref.decoder_logits(enc, ids)[-1].copy()
        lg[G.SUPPRESS] = -np.inf
        if len(ids) == len(PROMPT):
            lg[G.BEGIN_SUPPRESS] = -np.inf
        ids.append(int(np.argmax(lg)))
        if ids[-1] == G.EOS:
            break
    return ids


def scan_seed(seed, feats):
    """Every (prefix, factor, cap) of one seed whose float64 search keeps the gap: a list of dicts with the tags it earns."""
    model = G.build_model(seed)
    base_row = model.model.decoder.embed_tokens.weight[G.EOS].detach().clone()
    found = []
    for fac, n in itertools.product(FACTORS, G.CASES):
        set_eos_row(model, base_row, fac)
        m64 = HfRef(copy.deepcopy(model).double())
        with torch.no_grad():
            enc64 = m64.model.model.encoder(feats[n].double()).last_hidden_state
        for cap in (G.MAX_TARGET, SHORT_CAP):
            toks, lens, scores, steps, gap = BR.beam_search_ref(m64, enc64, PROMPT, G.SUPPRESS, G.BEGIN_SUPPRESS, G.EOS, cap, K)
            if gap < GAP:
                continue
            gr = greedy(m64, enc64, cap)
            closed_early = len(PROMPT) - 1 + steps < cap - 1
            tags = set()
            if cap == SHORT_CAP and not closed_early:
                tags.add("a")
            if closed_early and len(set(lens.tolist())) >= 2:
                tags.add("b")
            if toks[0, :lens[0]].tolist() != gr:
                tags.add("c")
            if closed_early and steps >= 12:
                tags.add("d")
            found.append(dict(seed=seed, n=n, fac=fac, cap=cap, tags=tags, toks=toks, lens=lens, scores=scores, steps=steps, gap=gap,
                              greedy=gr))
            print(f"seed {seed} n {n} factor {fac:+.0f} cap {cap}: steps {steps} gap {gap:.2e} lens {lens.tolist()} "
                  f"tags {''.join(sorted(tags))}", flush=True)
    return found


def pick(cases):
    """The fewest cases that cover (a), (b), (c) twice and (d), or None."""
    for k in range(2, 6):
        for sub in itertools.combinations(cases, k):
            tags = [t for c in sub for t in c["tags"]]
            if all(t in tags for t in "abd") and tags.count("c") >= 2:
                return list(sub)
    return None


def hf_case(c, feats):
    """Runs ``transformers`` on a chosen case and checks the float64 search against it."""
    from transformers import GenerationConfig, GenerationMixin
    model = G.build_model(c["seed"])
    base_row = model.model.decoder.embed_tokens.weight[G.EOS].detach().clone()
    set_eos_row(model, base_row, c["fac"])
    model.generation_config = GenerationConfig(**G.generation_config_dict())
    f = feats[c["n"]]
    prompt = torch.tensor([PROMPT])
    kw = dict(decoder_input_ids=prompt, num_beams=K, do_sample=False, length_penalty=1.0, early_stopping=False, max_length=c["cap"])
    with torch.no_grad():
        enc = model.model.encoder(f).last_hidden_state
        out = GenerationMixin.generate(model, input_features=f, num_return_sequences=K, return_dict_in_generate=True,
                                       output_scores=True, **kw)
        best = model.generate(f, **kw)[0].tolist()
    seqs, scores = out.sequences.tolist(), out.sequences_scores.double().numpy()
    toks = np.full((K, c["cap"]), G.EOS, np.int32)
    lens = np.zeros(K, np.int32)
    for s, row in enumerate(seqs):
        row = row if row[:len(PROMPT)] == PROMPT else PROMPT + row
        gen = row[len(PROMPT):]
        ln = len(PROMPT) + (gen.index(G.EOS) + 1 if G.EOS in gen else len(gen))
        toks[s, :ln], lens[s] = row[:ln], ln
    assert lens.tolist() == c["lens"].tolist() and (toks == c["toks"]).all(), (c["seed"], c["n"], c["fac"], toks, c["toks"])
    assert np.abs(scores - c["scores"]).max() < 1e-4, (scores, c["scores"])
    best = best if best[:len(PROMPT)] == PROMPT else PROMPT + best
    want = toks[0, :lens[0]].tolist()
    want = want[:-1] if want[-1] == G.EOS and best[-1:] != [G.EOS] and len(best) == len(want) - 1 else want   # the wrapper may drop the eos
    assert best[:len(want)] == want and all(t == G.EOS for t in best[len(want):]), (best, want)
    sd = {k: v for k, v in model.state_dict().items() if k.startswith("model.decoder.")}
    return enc[0].numpy(), toks, lens, scores, sd


def main():
    from transformers import WhisperFeatureExtractor
    fe = WhisperFeatureExtractor(feature_size=128, chunk_length=3)
    wave = G.make_wave()
    feats = {n: torch.from_numpy(fe(wave[:n], sampling_rate=16000, return_tensors="np").input_features) for n in G.CASES}
    per_seed, chosen = {}, None
    for seed in SEEDS:
        per_seed[seed] = scan_seed(seed, feats)
        chosen = pick(per_seed[seed])
        for other in ([] if chosen else [s for s in per_seed if s != seed]):
            chosen = pick(per_seed[other] + per_seed[seed])
            if chosen:
                break
        if chosen:
            break
    assert chosen, "no seed or pair of seeds covers the four conditions"
    seeds = sorted({c["seed"] for c in chosen})
    out = {"K": np.int32(K), "prompt": np.array(PROMPT, np.int32), "n_models": np.int32(len(seeds)), "n_cases": np.int32(len(chosen)),
           "seeds": np.array(seeds, np.int32), "config_json": np.array(json.dumps(G.hf_config().to_dict())),
           "generation_config_json": np.array(json.dumps(G.generation_config_dict()))}
    for i, c in enumerate(chosen):
        enc, toks, lens, scores, sd = hf_case(c, feats)
        m = seeds.index(c["seed"])
        for k, v in sd.items():
            if f"w{m}/{k}" not in out:                                # the eos row of the embedding is the case's: eos_row_<i>
                out[f"w{m}/{k}"] = G.bf16_bits(v)
        with torch.no_grad():
            out[f"eos_row_{i}"] = G.bf16_bits(sd["model.decoder.embed_tokens.weight"][G.EOS])
        out[f"case_{i}"] = np.array([m, c["n"], c["cap"], c["steps"]], np.int32)
        out[f"factor_{i}"], out[f"gap_{i}"] = np.float32(c["fac"]), np.float64(c["gap"])
        out[f"tags_{i}"] = np.array("".join(sorted(c["tags"])))
        out[f"enc_{i}"], out[f"tokens_{i}"], out[f"lens_{i}"], out[f"scores_{i}"] = enc, toks, lens, scores
        out[f"greedy_{i}"] = np.array(c["greedy"], np.int32)
        assert c["gap"] >= GAP
        print("case", i, "seed", c["seed"], "n", c["n"], "factor", c["fac"], "cap", c["cap"], "steps", c["steps"], "gap", c["gap"],
              "tags", out[f"tags_{i}"], "lens", lens.tolist())
    tags = [t for c in chosen for t in c["tags"]]
    assert all(t in tags for t in "abd") and tags.count("c") >= 2
    path = os.path.join(HERE, "whisper_beam.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
