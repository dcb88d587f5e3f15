"""float64 NumPy restatement of Whisper's prompt conditioning (``transformers``' long-form ``generate`` with
``condition_on_prev_tokens`` / ``prompt_ids``: ``_prepare_segments``, ``_prepare_decoder_input_ids``, ``_pad_to_max_length`` and
``_set_max_new_tokens_and_length``), on top of tests/whisper_ref.py (the model) and tests/whisper_long_ref.py (the rules, one
window, the segments), and of GPT-2's byte-level BPE.  tests/golden/make_whisper_prompt_golden.py asserts that it reproduces
``transformers``' tokens, segments and seeks for every case of tests/golden/whisper_prompt.npz; the CPU test pins it to that
fixture and the GPU test compares the device to both.

One row at a time: the reference for a row of a batch is that row's own B = 1 run."""
import json
import math
import os

import numpy as np

import whisper_long_ref as LR

HERE = os.path.dirname(os.path.abspath(__file__))


def load_fixture():
    """tests/golden/whisper_prompt.npz: the cases, on the model, wave and configs of tests/golden/whisper_long.npz."""
    fx = LR.load_fixture()
    z = np.load(os.path.join(HERE, "golden", "whisper_prompt.npz"))
    fx["cases"] = json.loads(str(z["cases_json"]))
    fx["tokenizer"] = json.loads(str(z["tokenizer_json"]))
    for k in z.files:
        if k.startswith("rows_"):
            fx[k] = z[k]
    return fx


# ---- the decoder input of a window --------------------------------------------------------------------------------------------
def previous_text_ref(history, tb, cut):
    seq = []
    for seg in history:
        seg = list(seg)
        if len(seg) > 2 and seg[-2] >= tb:
            seg = seg[:-1]
        seq += seg
    return seq[len(seq) - cut:] if len(seq) > cut else seq


def start_history(ctx, prev):
    """``_prepare_segments``: a "first-segment" prompt, without its <|startofprev|>, is the row's first previous segment."""
    ids = ctx.get("prompt_ids")
    if ids is not None and ctx.get("prompt_condition_type", "first-segment") == "first-segment":
        return [list(ids[1:] if ids[0] == prev else ids)]
    return []


def window_prompt_ref(ctx, forced, history, conditioned, prev, tb, cut):
    ids = ctx.get("prompt_ids")
    if conditioned and len(history) > 0:
        lead = list(ids) if ids is not None and ctx.get("prompt_condition_type") == "all-segments" else [prev]
        return lead + previous_text_ref(history, tb, cut) + list(forced)
    if ids is not None:
        return list(ids) + list(forced)
    return list(forced)


def no_speech_prob_at(ref, enc, prompt, sot_pos, gen):
    """The probability of <|nospeech|> after <|startoftranscript|>, wherever the prompt puts it."""
    x = ref.decoder_logits(enc, prompt[:sot_pos + 1])[-1]
    return float(np.exp(x[gen["no_timestamps_token_id"] - 1] - LR._lse(x)))


# ---- the seek loop ------------------------------------------------------------------------------------------------------------
def transcribe_prompt_ref(ref, feats, forced, gen, cap, window, ctx, K=1, no_speech_threshold=None, logprob_threshold=None,
                          fallback=None):
    """feats [T][n_mels] of one recording; ctx: dict(condition_on_prev_tokens, prompt_ids, prompt_condition_type) ->
    (segments as dicts, seeks, [rule gap, pick gap] of the greedy windows, one letter per window as ``transcribe_long_ref``, the
    windows' records dict(prompt, avg_logprob, no_speech_prob, n_new, temperature)).  The token bound is ``cap`` for prompt and picks
    together.  ``fallback``: dict(temperatures, compression_ratio_threshold, logprob_threshold, seed, row_key, vocab): a window is
    decoded again at the next temperature while ``need_fallback_ref`` asks for it (tests/whisper_sample_ref.py; a positive
    temperature samples, and gaps gains the smallest sampled margin as a third entry); a window kept at 0.5 or more does not
    condition the next one."""
    import whisper_sample_ref as S
    eos, tb, prev = gen["eos_token_id"], gen["no_timestamps_token_id"] + 1, gen.get("prev_sot_token_id")
    cut = cap // 2 - 1
    T, seek, segs, seeks, gaps, kinds, wins = feats.shape[0], 0, [], [], [np.inf, np.inf], "", []
    history, cond, serial = start_history(ctx, prev), bool(ctx.get("condition_on_prev_tokens")), 0
    while seek < T:
        seeks.append(seek)
        nf = min(window, T - seek)
        win = np.zeros((window, feats.shape[1]))
        win[:nf] = feats[seek:seek + nf]
        enc = ref.encoder(win)
        prompt = window_prompt_ref(ctx, forced, history, cond, prev, tb, cut)
        assert len(prompt) < cap, ("no room", len(prompt), cap)
        ns = no_speech_prob_at(ref, enc, prompt, len(prompt) - len(forced), gen)
        for temp in (fallback["temperatures"] if fallback else (0.0,)):
            if temp > 0:
                full, total, rg, sg = S.sampled_window_ref(ref, enc, prompt, gen, cap, temp, fallback["seed"], serial, fallback["row_key"])
                serial += 1
                gaps = [min(gaps[0], rg), gaps[1], min(gaps[2] if len(gaps) > 2 else np.inf, sg)]
                avg = total / len(full)
            elif K == 1:
                full, total, rg, pg = LR.greedy_window_ref(ref, enc, prompt, gen, cap)
                gaps = [min(gaps[0], rg), min(gaps[1], pg)] + gaps[2:]
                avg = total / len(full)
            else:
                full, avg = LR.beam_window_ref(ref, enc, prompt, gen, cap, K), float("nan")
            if not fallback or not S.need_fallback_ref(S.compression_ratio_ref(full, fallback["vocab"]), avg, ns,
                                                       fallback.get("compression_ratio_threshold"), fallback.get("logprob_threshold"),
                                                       no_speech_threshold)[0]:
                break
        wins.append(dict(prompt=prompt, avg_logprob=avg, no_speech_prob=ns, n_new=len(full), temperature=float(temp),
                         n_history=len(previous_text_ref(history, tb, 1 << 30))))
        cond = bool(ctx.get("condition_on_prev_tokens")) and temp < 0.5    # ``is_low_temperature``
        seq = full[:-1] if full[-1] == eos else full
        if no_speech_threshold is not None and avg < logprob_threshold and ns > no_speech_threshold:
            seek += nf
            kinds += "k"
            continue
        parts, step = LR.split_ref(seq, tb, seek, nf)
        pair = any(a >= tb and b >= tb for a, b in zip(seq[:-1], seq[1:]))
        kinds += ("p" if step < nf else "s") if pair else ("N" if len(full) == cap - len(prompt) and full[-1] != eos else "n")
        segs.extend(dict(start=s0, end=s1, tokens=tok, seek=seek, avg_logprob=avg, no_speech_prob=ns) for s0, s1, tok in parts)
        history.extend(tok for _, _, tok in parts)
        seek += step
    return segs, seeks, gaps, kinds, wins


# ---- byte-level BPE -----------------------------------------------------------------------------------------------------------
GPT2_PATTERN = r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"


def byte_table():
    keep = list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
    table, n = {}, 0
    for b in range(256):
        if b in keep:
            table[b] = chr(b)
        else:
            table[b], n = chr(256 + n), n + 1
    return table


def bpe_ref(symbols, ranks):
    word = list(symbols)
    while len(word) > 1:
        pairs = [(ranks.get((a, b), math.inf), i) for i, (a, b) in enumerate(zip(word[:-1], word[1:]))]
        best = min(pairs)
        if best[0] == math.inf:
            break
        a, b = word[best[1]], word[best[1] + 1]
        out, i = [], 0
        while i < len(word):
            if i + 1 < len(word) and (word[i], word[i + 1]) == (a, b):
                out.append(a + b)
                i += 2
            else:
                out.append(word[i])
                i += 1
        word = out
    return word


def encode_ref(text, vocab, merges):
    import regex
    ranks = {tuple(m.split(" ")): i for i, m in enumerate(merges)}
    table = byte_table()
    return [vocab[p] for tok in regex.findall(GPT2_PATTERN, text) for p in bpe_ref([table[b] for b in tok.encode("utf-8")], ranks)]
