"""Makes tests/golden/whisper_align.npz from ``transformers`` (5.15.0 when this was run): token timestamps of the tiny seeded Whisper
of tests/golden/make_whisper_golden.py (its builders are imported, nothing is copied or downloaded).

Truth: ``model.generate(features, decoder_input_ids=prompt, do_sample=False, return_token_timestamps=True, attention_mask=...)``
with ``generation_config.alignment_heads = [[0, 1], [1, 0], [1, 3]]``, ``config.median_filter_width = 7`` and eager attention.  In
this version the number of frames reaches ``_extract_token_timestamps`` through the attention mask (``num_frames =
attention_mask.sum(-1)``: a ``num_frames=`` keyword is overwritten), so the mask marks the samples // 160 frames of the wave.

Cases (``case_names``):
    a3s     the greedy fixture's seed, 3 s (M = 150), decoded to the cap of 48 positions (N = 43)
    a09cut  the same weights, 0.9 s (M = 45), cut to 2 new tokens (N = 1: the time is 0)
    b3s     a second weight seed (the first of ``SEEDS_B`` whose cases all meet the gap condition), 3 s, 20 new tokens
    b09     the second seed, 0.9 s, 12 new tokens
    b09eos  the second seed with its ``<|endoftext|>`` embedding row scaled (``eos_row_b``; the first factor of the greedy
            generator's ``EOS_FACTORS`` with which the 0.9 s wave ends on eos after at least 4 new tokens and before the cap)
Per case: ``tokens_<c>`` (prompt, new tokens and the closing eos when the sequence ended by itself: the layout of
``Whisper.generate``), ``frames_<c>`` (the times as integer frame indices = round(t / 0.02), prompt zeros included, the last
repeating the one before it), ``nframes_<c>`` (mel frames), ``probs_<c>`` f32 [heads][N][M] (the selected heads' cross-attention
weights of the N fed positions, cropped to M), ``cost_<c>`` f32 [N][M] (the matrix handed to ``_dynamic_time_warping``) and
``gap_<c>``.  The second seed's weights are stored as bf16 bits (``wb/<name>``), as the greedy fixture stores the first's.

Gap condition, asserted here in float64 for every case with N >= 2: on every cell of the DTW path the chosen predecessor cost and
the runner-up differ by at least 1e-3 (``gap_<c>`` holds the smallest difference).  It is a condition on the inputs, not a
tolerance of the kernel: a case that misses it is replaced by another seed, never loosened.

Words: the synthetic vocabulary of the greedy fixture, a few token lists (``word_ids``, padded with -1) and, per list,
the language it was grouped for and what ``_combine_tokens_into_words`` returns (``word_json``: words and token indices), in both split
modes (spaces for "english", unicode points for "chinese").

    python tests/golden/make_whisper_align_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_whisper_golden as G      # noqa: E402
import whisper_ref as R              # noqa: E402

ALIGNMENT_HEADS = [[0, 1], [1, 0], [1, 3]]
WIDTH = 7
SEEDS_B = tuple(range(3, 40))
MIN_GAP = 1e-3


def on_path_gap(C):
    """Float64 recursion of ``_dynamic_time_warping`` over C [N][M]; -> the smallest |chosen - runner-up| over the path's cells
    (cells whose two other predecessors are both +inf do not count: nothing can flip them)."""
    N, M = C.shape
    cost = np.full((N + 1, M + 1), np.inf)
    cost[0, 0] = 0.0
    move = np.zeros((N + 1, M + 1), np.int8)
    gap = np.full((N + 1, M + 1), np.inf)
    for i in range(1, N + 1):
        for j in range(1, M + 1):
            c = (cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1])
            t = 0 if c[0] < c[1] and c[0] < c[2] else 1 if c[1] < c[0] and c[1] < c[2] else 2
            rest = [c[k] for k in range(3) if k != t and np.isfinite(c[k])]
            if rest:
                gap[i, j] = min(abs(r - c[t]) for r in rest)
            cost[i, j] = C[i - 1, j - 1] + c[t]
            move[i, j] = t
    i, j, g = N, M, np.inf
    while i > 0 and j > 0:
        g = min(g, gap[i, j])
        t = move[i, j]
        i, j = (i - 1, j - 1) if t == 0 else (i - 1, j) if t == 1 else (i, j - 1)
    assert i == 0 and j == 0
    return float(g)


def run_case(model, fe, wave, prompt, max_new_tokens):
    import transformers.models.whisper.generation_whisper as GW
    from transformers import GenerationConfig
    gc = G.generation_config_dict()
    gc["alignment_heads"] = ALIGNMENT_HEADS
    model.generation_config = GenerationConfig(**gc)
    model.config.median_filter_width = WIDTH
    model.config._attn_implementation = "eager"
    nframes = len(wave) // 160
    M = nframes // 2
    feats = torch.from_numpy(fe(wave, sampling_rate=16000, return_tensors="np").input_features)
    mask = torch.zeros(1, feats.shape[-1], dtype=torch.long)
    mask[:, :nframes] = 1
    seen = {}
    dtw, extract = GW._dynamic_time_warping, model._extract_token_timestamps

    def spy_dtw(matrix):
        seen["cost"] = np.array(matrix)
        return dtw(matrix)

    def spy_extract(outputs, *a, **kw):
        seen["cross"] = outputs.cross_attentions
        return extract(outputs, *a, **kw)
    GW._dynamic_time_warping, model._extract_token_timestamps = spy_dtw, spy_extract
    try:
        kw = {} if max_new_tokens is None else dict(max_new_tokens=max_new_tokens)
        with torch.no_grad():
            out = model.generate(feats, attention_mask=mask, decoder_input_ids=torch.tensor([prompt]), do_sample=False,
                                 return_token_timestamps=True, **kw)
    finally:
        GW._dynamic_time_warping = dtw
        del model._extract_token_timestamps
    n0 = len(prompt)
    new = out["sequences"][0].tolist()
    if new[:n0] == list(prompt):
        new = new[n0:]
    ts = out["token_timestamps"][0].double().numpy()
    steps = len(seen["cross"])                                       # forward passes = tokens picked, a closing eos included
    tokens = list(prompt) + new
    if steps == len(new) + 1:                                        # this generate strips the closing eos
        tokens.append(G.EOS)
    assert len(tokens) == n0 + steps, (len(tokens), n0, steps)
    N = steps - 1
    frames = np.zeros(len(tokens), np.int32)
    t_new = np.round(ts / 0.02).astype(np.int32)
    assert np.abs(t_new * 0.02 - ts).max() < 1e-6
    if len(t_new) == len(tokens):                                    # with the prompt's zeros in front
        t_new = t_new[n0:]
    assert len(t_new) in (N + 1, N), (len(t_new), N)
    frames[n0:n0 + len(t_new)] = t_new
    if len(t_new) == N and N > 0:                                    # the stripped eos: it repeats the token before it
        frames[n0 + N] = t_new[-1]
    assert N == 0 or frames[n0 + N] == frames[n0 + N - 1]
    # the selected heads' weights of the fed positions n0 .. n0 + N - 1, cropped to M columns
    per_layer = [torch.cat([step[l] for step in seen["cross"]], dim=2) for l in range(model.config.decoder_layers)]
    probs = torch.stack([per_layer[l][0, h] for l, h in ALIGNMENT_HEADS])[:, n0:, :M].numpy().astype(np.float32)
    assert probs.shape == (len(ALIGNMENT_HEADS), N, M), probs.shape
    cost = seen["cost"].astype(np.float32) if N > 0 else np.zeros((0, M), np.float32)
    assert cost.shape == (N, M) and (N == 0 or np.array_equal(cost.astype(np.float64), seen["cost"], equal_nan=True))   # fp32 values (NaN at N = 1)
    gap = on_path_gap(seen["cost"]) if N >= 2 else np.inf
    return dict(tokens=np.array(tokens, np.int32), frames=frames, nframes=np.int32(nframes), probs=probs, cost=cost,
                gap=np.float64(gap))


def word_cases():
    """Token lists for the grouping rules and what the reference makes of them."""
    from transformers import WhisperTokenizer
    from transformers.models.whisper.tokenization_whisper import _combine_tokens_into_words
    vocab, added, _ = G.vocab_and_cases()
    full = dict(vocab)
    full.update(added)
    tok = WhisperTokenizer(vocab=full, merges=[])
    tok.add_special_tokens({"additional_special_tokens": list(added)})
    for s, k in added.items():
        assert tok.convert_tokens_to_ids(s) == k
    b2u = G.bytes_to_unicode()
    ix = dict(vocab)

    def ch(s):
        return [ix[b2u[ord(c)]] for c in s]

    def by(*bs):
        return [ix[b2u[b]] for b in bs]
    hello, world, the, ing, caf = 0, 1, 2, 3, 4
    cases = [
        ("english", [hello, world] + ch(".")),                                                  # " hello", " world."
        ("english", [hello] + ch(",") + [the, world, ing] + ch(".") + ch("-") + [the]),
        ("english", [G.SOT, G.EN, G.TRANSCRIBE, G.NOTIMESTAMPS, hello] + ch("ab") + [world, G.EOS]),
        ("english", ch(" ") + ch("'") + [hello] + ch("'") + ch(" -") + [world] + ch("s")),     # prepended and appended marks
        ("english", [caf] + by(0xC3, 0xA9) + [the] + by(0xE4, 0xBD, 0xA0) + [world]),           # characters split across tokens
        ("chinese", by(0xE4, 0xBD, 0xA0) + by(0xE5, 0xA5, 0xBD) + ch(",") + by(0xE4, 0xBD, 0xA0) + ch(".")),
        ("chinese", [G.SOT, G.ZH, G.TRANSCRIBE, G.NOTIMESTAMPS] + by(0xE5, 0xA5, 0xBD) + [hello] + by(0xF0, 0x9F, 0x98, 0x80) + [G.EOS]),
        ("english", []),
    ]
    got = []
    for lang, ids in cases:
        words, _, idx = _combine_tokens_into_words(tok, list(ids), lang) if ids else ([], [], [])
        got.append(dict(language=lang, words=words, indices=idx))
    return cases, got


def main():
    from transformers import WhisperFeatureExtractor
    fx = R.load_fixture()
    fe = WhisperFeatureExtractor(feature_size=128, chunk_length=3)
    wave = G.make_wave()
    assert np.array_equal(np.round(wave * 32768).astype(np.int16), fx["wave"])
    prompt = fx["prompt"].tolist()
    seed_a = int(fx["seed"])
    out = {"alignment_heads": np.array(ALIGNMENT_HEADS, np.int32), "median_filter_width": np.int32(WIDTH),
           "seed_a": np.int32(seed_a)}
    res = {}
    model = G.build_model(seed_a)
    for k, v in model.state_dict().items():
        if k != "proj_out.weight":
            assert np.array_equal(v.numpy(), fx["sd"][k]), k                 # the greedy fixture's weights, rebuilt
    res["a3s"] = run_case(model, fe, wave[:48000], prompt, None)
    res["a09cut"] = run_case(model, fe, wave[:14400], prompt, 2)
    assert res["a3s"]["tokens"].tolist() == fx["tokens_48000"].tolist()
    assert len(res["a09cut"]["tokens"]) == len(prompt) + 2 and res["a09cut"]["frames"].max() == 0
    assert res["a3s"]["gap"] >= MIN_GAP, res["a3s"]["gap"]
    # (the greedy fixture's own eos case has an on-path gap of 4.6e-4: it misses the condition, so the eos case is the second seed's)
    chosen = None
    for seed in SEEDS_B:
        if seed == seed_a:
            continue
        model = G.build_model(seed)
        rb = {"b3s": run_case(model, fe, wave[:48000], prompt, 20), "b09": run_case(model, fe, wave[:14400], prompt, 12)}
        print("seed", seed, {c: (float(r["gap"]), len(r["tokens"])) for c, r in rb.items()})
        if not all(r["gap"] >= MIN_GAP and r["frames"].max() > 0 for r in rb.values()):
            continue
        base_row = model.model.decoder.embed_tokens.weight[G.EOS].detach().clone()
        for fac in G.EOS_FACTORS:                                        # as the greedy fixture makes its eos case
            with torch.no_grad():
                model.model.decoder.embed_tokens.weight[G.EOS] = (base_row * fac).bfloat16().float()
            r = run_case(model, fe, wave[:14400], prompt, None)
            n_new = len(r["tokens"]) - len(prompt)
            print("  eos factor", fac, n_new, int(r["tokens"][-1]), float(r["gap"]))
            if r["tokens"][-1] == G.EOS and 4 <= n_new and len(r["tokens"]) < G.MAX_TARGET and r["gap"] >= MIN_GAP:
                rb["b09eos"] = r
                out["eos_row_b"] = G.bf16_bits(model.model.decoder.embed_tokens.weight[G.EOS])
                break
        with torch.no_grad():
            model.model.decoder.embed_tokens.weight[G.EOS] = base_row
        if "b09eos" in rb:
            chosen = seed
            res.update(rb)
            break
    assert chosen is not None, "no second seed meets the gap condition"
    out["seed_b"] = np.int32(chosen)
    for k, v in model.state_dict().items():
        if k != "proj_out.weight":
            out["wb/" + k] = G.bf16_bits(v)
    out["case_names"] = np.array(json.dumps(list(res)))
    for c, r in res.items():
        print(c, "n", len(r["tokens"]), "N x M", r["cost"].shape, "gap", float(r["gap"]), "frames", r["frames"].tolist())
        for k, v in r.items():
            out[f"{k}_{c}"] = v
    cases, got = word_cases()
    L = max(len(ids) for _, ids in cases)
    out["word_ids"] = np.array([ids + [-1] * (L - len(ids)) for _, ids in cases], np.int32)
    out["word_json"] = np.array(json.dumps(got))
    for g in got:
        print(g["language"], g["words"], g["indices"])
    path = os.path.join(HERE, "whisper_align.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
