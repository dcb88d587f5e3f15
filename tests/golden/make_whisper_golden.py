"""Makes tests/golden/whisper.npz from ``transformers`` (5.15.0 when this was run): a tiny seeded ``WhisperForConditionalGeneration``
and ``WhisperFeatureExtractor`` (numpy only) -- nothing is downloaded.

Model: d_model 64, 2 + 2 layers, 4 heads, ffn 128, 128 mel bins, vocab 160 (ids >= 140 special), 150 source and 48 target positions,
non-trivial ``suppress_tokens`` / ``begin_suppress_tokens``, all dropouts 0.  After the seeded init every matrix (Linear, Conv1d and
the tied token embedding) is scaled x6, the decoder position embeddings are redrawn at unit variance and the LayerNorm parameters
perturbed: without that the greedy output is one token repeated, which tests nothing about the cache.  The seed is the first of
``SEEDS`` for which every case meets the asserted conditions (relative top-1 / top-2 margin of every step >= 1e-2, i.e. 50x the
2e-4 parity gate of the GPU tests; >= 12 distinct tokens per sequence).

Features: ``WhisperFeatureExtractor(feature_size=128, chunk_length=3)``: 300 frames, 150 positions.  One 3 s wave of noise + tone is
stored; the cases are its prefixes of 0.9 s, 2.5 s and 3 s (the ragged pair of the GPU tests is (2.5 s, 0.9 s) with garbage beyond
``len``; its expected rows are these cases' own).  Per case: the extractor's features (in full for 3 s; for the shorter ones the
frames listed in ``feat_idx_<n>``: the first 4, every 8th, and those around the end of the data, to stay under the 1 MiB limit of a
committed file), the encoder's ``last_hidden_state``, the teacher-forced logits of the first 12 tokens, the greedy sequence from a
manual loop over ``forward`` with the two suppress rules (cross-checked here against ``model.generate(features,
decoder_input_ids=prompt, do_sample=False)``) and every step's margin / RMS of the finite logits.

The case ``eos``: no seed was searched for one that ends by itself; the ``<|endoftext|>`` row of the tied embedding is scaled in THAT
case's model (``eos_row``; the first factor of ``EOS_FACTORS``, either sign, with which the 0.9 s wave ends on eos after at least 3 and before
the cap of new tokens).  ``feat80_<n>``: the features of a second extractor with 80 mel bins (front-end only).

The tokenizer part: a synthetic byte-level ``vocab.json`` (``vocab_json``; multi-byte UTF-8 split across tokens, an invalid byte
sequence) with id lists (``tok_ids``, padded with -1) and the strings ``WhisperTokenizer.batch_decode(skip_special_tokens=True)``
returns for them (``tok_text``, JSON).

Weights are rounded to bf16-representable values (stored as their upper 16 bits, ``w/<name>``) and the wave to 16-bit PCM before the
model runs, as the WavLM fixture does.

    python tests/golden/make_whisper_golden.py
"""
import json
import os

import numpy as np
import torch

SEEDS = tuple(range(1, 201))
CASES = (14400, 40000, 48000)
EOS_FACTORS = (1.0, 1.5, -1.5, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0, 6.0, -6.0, 8.0, -8.0, 12.0, -12.0)
N_SPECIAL0 = 140
EOS, SOT, EN, ZH, DE, TRANSLATE, TRANSCRIBE, NOTIMESTAMPS = 140, 141, 142, 143, 144, 145, 146, 159   # no timestamp ids: 159 is the last
SUPPRESS = [1, 2, 7, 8, 9, 63, 64, 65, 90] + list(range(141, 160))
BEGIN_SUPPRESS = [5, 140]
MAX_TARGET = 48
PREFIX = 12


def hf_config(n_mels=128):
    from transformers import WhisperConfig
    return WhisperConfig(
        vocab_size=160, num_mel_bins=n_mels, d_model=64, encoder_layers=2, decoder_layers=2, encoder_attention_heads=4,
        decoder_attention_heads=4, encoder_ffn_dim=128, decoder_ffn_dim=128, max_source_positions=150,
        max_target_positions=MAX_TARGET, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, encoder_layerdrop=0.0,
        decoder_layerdrop=0.0, pad_token_id=EOS, bos_token_id=EOS, eos_token_id=EOS, decoder_start_token_id=SOT,
        suppress_tokens=SUPPRESS, begin_suppress_tokens=BEGIN_SUPPRESS)


def generation_config_dict():
    return dict(suppress_tokens=SUPPRESS, begin_suppress_tokens=BEGIN_SUPPRESS, eos_token_id=EOS, pad_token_id=EOS,
                bos_token_id=EOS, decoder_start_token_id=SOT, no_timestamps_token_id=NOTIMESTAMPS, is_multilingual=True,
                lang_to_id={"<|en|>": EN, "<|zh|>": ZH, "<|de|>": DE}, task_to_id={"translate": TRANSLATE, "transcribe": TRANSCRIBE},
                max_length=MAX_TARGET)


def build_model(seed):
    from transformers import WhisperForConditionalGeneration
    torch.manual_seed(seed)
    model = WhisperForConditionalGeneration(hf_config()).eval()
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name == "model.decoder.embed_positions.weight":
                p.copy_(torch.randn(p.shape, generator=g))
            elif name == "model.encoder.embed_positions.weight":
                pass                                                   # the sinusoids stay
            elif "layer_norm" in name:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            elif p.ndim >= 2:
                p.mul_(6.0)
        # pad_token_id = eos makes that row the embedding's padding_idx, which the init zeroes; a trained checkpoint's is not zero
        emb = model.model.decoder.embed_tokens.weight
        emb[EOS] = emb[:N_SPECIAL0].std() * torch.randn(emb.shape[1], generator=g)
        for p in model.parameters():
            p.copy_(p.bfloat16().float())
    return model


def make_wave():
    g = torch.Generator().manual_seed(77)
    S = CASES[-1]
    t = torch.arange(S) / 16000.0
    w = 0.05 * torch.randn(S, generator=g) + 0.3 * torch.sin(2 * np.pi * 220.0 * t) * (1 + 0.5 * torch.sin(2 * np.pi * 3 * t)) \
        + 0.1 * torch.sin(2 * np.pi * (900.0 + 400.0 * t) * t)
    return (torch.round(w.clamp(-0.999, 0.999) * 32768) / 32768).numpy().astype(np.float32)


def greedy(model, enc, prompt):
    """The manual loop: forward on the whole prefix every step, the two suppress rules, argmax."""
    ids, margins = list(prompt), []
    while len(ids) < MAX_TARGET:
        lg = model(encoder_outputs=(enc,), decoder_input_ids=torch.tensor([ids])).logits[0, -1].double()
        lg[SUPPRESS] = -np.inf
        if len(ids) == len(prompt):
            lg[BEGIN_SUPPRESS] = -np.inf
        fin = lg[torch.isfinite(lg)]
        top = torch.topk(lg, 2).values
        margins.append(float((top[0] - top[1]) / fin.pow(2).mean().sqrt()))
        tok = int(torch.argmax(lg))
        ids.append(tok)
        if tok == EOS:
            break
    return ids, margins


def run_case(model, fe, wave, prompt, check_generate=True):
    feats = torch.from_numpy(fe(wave, sampling_rate=16000, return_tensors="np").input_features)
    with torch.no_grad():
        enc = model.model.encoder(feats).last_hidden_state
        ids, margins = greedy(model, enc, prompt)
        logits = model(input_features=feats, decoder_input_ids=torch.tensor([ids[:PREFIX]])).logits[0]
        if check_generate:
            from transformers import GenerationConfig
            model.generation_config = GenerationConfig(**generation_config_dict())
            gen = model.generate(feats, decoder_input_ids=torch.tensor([prompt]), do_sample=False)
            gen = gen[0].tolist()
            if gen[:len(prompt)] != list(prompt):                       # this generate returns the new tokens only
                gen = list(prompt) + gen
            if ids[-1] == EOS and gen == ids[:-1]:                       # ... and without the closing eos
                gen = gen + [EOS]
            assert gen[:len(ids)] == ids and all(t == EOS for t in gen[len(ids):]), (gen, ids)
    return feats[0].t().contiguous().numpy(), enc[0].numpy(), logits.numpy(), ids, margins


def bytes_to_unicode():
    """GPT-2's byte -> printable character table: the printable Latin-1 bytes map to themselves, the others to 256, 257, ..."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    table, n = {}, 0
    for b in range(256):
        if b in keep:
            table[b] = chr(b)
        else:
            table[b] = chr(256 + n)
            n += 1
    return table


def vocab_and_cases():
    """A synthetic byte-level vocabulary of 140 pieces + the specials, and id lists to decode."""
    b2u = bytes_to_unicode()
    pieces = []
    for word in (" hello", " world", " the", "ing", " caf"):
        pieces.append("".join(b2u[b] for b in word.encode()))
    for ch in "abcdefghijklmnopqrstuvwxyz ,.'-":
        pieces.append(b2u[ord(ch)])
    for by in (0xC3, 0xA9, 0xE4, 0xBD, 0xA0, 0xE5, 0xA5, 0xF0, 0x9F, 0x98, 0x80):      # e-acute, two CJK characters, an emoji
        pieces.append(b2u[by])
    i = 0
    while len(pieces) < N_SPECIAL0:
        pieces.append("".join(b2u[b] for b in f" w{i}".encode()))
        i += 1
    assert len(set(pieces)) == N_SPECIAL0
    specials = ["<|endoftext|>", "<|startoftranscript|>", "<|en|>", "<|zh|>", "<|de|>", "<|translate|>", "<|transcribe|>",
                "<|startoflm|>", "<|startofprev|>", "<|nospeech|>"] + [f"<|{l}|>" for l in ("fr", "es", "ru", "ko", "ja", "pt", "tr", "pl", "ca")] + ["<|notimestamps|>"]
    vocab = {p: k for k, p in enumerate(pieces)}
    added = {s: N_SPECIAL0 + k for k, s in enumerate(specials)}
    ix = {p: k for k, p in enumerate(pieces)}

    def by(*bs):
        return [ix[b2u[b]] for b in bs]

    def ch(s):
        return [ix[b2u[ord(c)]] for c in s]
    cases = [
        [SOT, EN, TRANSCRIBE, NOTIMESTAMPS, 0, 1, EOS],                                  # " hello world"
        [0] + ch(",") + [2, 1] + ch(".") + [EOS, EOS],
        [4] + by(0xC3, 0xA9) + ch(" ") + by(0xE4, 0xBD, 0xA0) + by(0xE5, 0xA5, 0xBD),      # " cafe' " + two CJK characters
        by(0xF0, 0x9F, 0x98, 0x80) + [0],                                                 # an emoji over four tokens
        by(0xA9) + ch("a") + by(0xE4, 0xBD) + ch("b"),                                    # invalid UTF-8: errors="replace"
        [SOT, ZH, 150, NOTIMESTAMPS, 3, 3, 155, EOS],
        [],
    ]
    return vocab, added, cases


def hf_decode(vocab, added, cases):
    from transformers import WhisperTokenizer
    full = dict(vocab)
    full.update(added)
    tok = WhisperTokenizer(vocab=full, merges=[])
    tok.add_special_tokens({"additional_special_tokens": list(added)})
    for s, k in added.items():
        assert tok.convert_tokens_to_ids(s) == k, (s, k, tok.convert_tokens_to_ids(s))
    return tok.batch_decode(cases, skip_special_tokens=True)


def bf16_bits(t):
    return (t.detach().contiguous().view(torch.int32) >> 16).to(torch.int16).numpy().view(np.uint16)


def main():
    from transformers import WhisperFeatureExtractor
    fe = WhisperFeatureExtractor(feature_size=128, chunk_length=3)
    wave = make_wave()
    prompt = [SOT, EN, TRANSCRIBE, NOTIMESTAMPS]
    chosen = None
    for seed in SEEDS:
        model = build_model(seed)
        res = {n: run_case(model, fe, wave[:n], prompt, check_generate=False) for n in CASES}
        ok = all(min(r[4]) >= 1e-2 and len(set(r[3][4:])) >= 12 for r in res.values())
        print("seed", seed, {n: (round(min(r[4]), 4), len(set(r[3][4:])), len(r[3])) for n, r in res.items()}, "ok" if ok else "")
        if ok:
            chosen = seed
            res = {n: run_case(model, fe, wave[:n], prompt) for n in CASES}      # now with the generate cross-check
            break
    assert chosen is not None, "no seed meets the margin / distinct-token conditions"
    out = {"seed": np.int32(chosen), "wave": np.round(wave * 32768).astype(np.int16), "cases": np.array(CASES, np.int32),
           "prompt": np.array(prompt, np.int32), "config_json": np.array(json.dumps(hf_config().to_dict())),
           "generation_config_json": np.array(json.dumps(generation_config_dict()))}
    for k, v in model.state_dict().items():
        if k != "proj_out.weight":                                      # tied to model.decoder.embed_tokens.weight
            out["w/" + k] = bf16_bits(v)
    for n, (feat, enc, logits, ids, margins) in res.items():
        if n == CASES[-1]:
            out[f"feat_{n}"] = feat
        else:
            nd = n // 160
            idx = sorted(set(list(range(4)) + list(range(0, 300, 8)) + list(range(max(nd - 6, 0), min(nd + 4, 300))) + [299]))
            out[f"feat_idx_{n}"], out[f"feat_{n}"] = np.array(idx, np.int32), feat[idx]
        out[f"enc_{n}"], out[f"logits_{n}"] = enc, logits
        out[f"tokens_{n}"], out[f"margin_{n}"] = np.array(ids, np.int32), np.array(margins, np.float64)
    # the eos case
    n0, done = CASES[0], False
    base_row = model.model.decoder.embed_tokens.weight[EOS].detach().clone()
    for fac in EOS_FACTORS:
        with torch.no_grad():
            model.model.decoder.embed_tokens.weight[EOS] = (base_row * fac).bfloat16().float()
        feat, enc, logits, ids, margins = run_case(model, fe, wave[:n0], prompt)
        print("eos factor", fac, len(ids), ids[-1], round(min(margins), 4))
        if ids[-1] == EOS and 4 + 3 <= len(ids) < MAX_TARGET and min(margins) >= 1e-2:
            done = True
            break
    assert done, "no factor ends the sequence on eos"
    out["eos_factor"], out["eos_row"] = np.float32(fac), bf16_bits(model.model.decoder.embed_tokens.weight[EOS])
    out["enc_eos"], out["logits_eos"] = enc, logits[:min(PREFIX, len(ids))]
    out["tokens_eos"], out["margin_eos"] = np.array(ids, np.int32), np.array(margins, np.float64)
    # 80 mel bins: front-end only
    fe80 = WhisperFeatureExtractor(feature_size=80, chunk_length=3)
    f80 = fe80(wave[:n0], sampling_rate=16000, return_tensors="np").input_features[0].T
    idx = out[f"feat_idx_{n0}"]
    out[f"feat80_{n0}"] = np.ascontiguousarray(f80[idx])
    # tokenizer
    vocab, added, cases = vocab_and_cases()
    texts = hf_decode(vocab, added, cases)
    L = max(len(c) for c in cases)
    out["vocab_json"], out["added_tokens_json"] = np.array(json.dumps(vocab)), np.array(json.dumps(added))
    out["tok_ids"] = np.array([c + [-1] * (L - len(c)) for c in cases], np.int32)
    out["tok_text"] = np.array(json.dumps(texts))
    print(texts)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "whisper.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
