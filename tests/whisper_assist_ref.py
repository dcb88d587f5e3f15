"""Float64 NumPy restatement of assisted generation (speculative decoding) as eval/whisper.py runs it, around ``whisper_ref.Ref``
and ``whisper_long_ref``: a draft model proposes U tokens per round with ordinary greedy steps, the target picks at all U + 1
positions from one pass over the drafted history, every row keeps the picks up to the first one that differs from its draft, and
ALL rows advance by the smallest such count (``accept_ref``).  In greedy decoding the output is by construction the target's own,
whatever the draft proposes; tests/golden/make_whisper_assist_golden.py asserts that against ``transformers``' assisted generation
(tests/golden/whisper_assist.npz) and tests/test_whisper_assist_cpu.py pins it.  It shares no code with f5e_tts_amd."""
import json
import os

import numpy as np

import whisper_long_ref as LR
import whisper_ref as WR

HERE = os.path.dirname(os.path.abspath(__file__))


def load_fixture():
    """tests/golden/whisper_assist.npz: the draft model (its own encoder, another width) for the model and wave of
    tests/golden/whisper.npz, and the tokens ``transformers``' assisted generation returned per case."""
    z = np.load(os.path.join(HERE, "golden", "whisper_assist.npz"))
    fx = {k: z[k] for k in z.files if not k.startswith("w/")}
    fx["sd"] = {k[2:]: (z[k].astype(np.uint32) << 16).view(np.float32) for k in z.files if k.startswith("w/")}
    fx["config"] = json.loads(str(fx["config_json"]))
    fx["cases"] = json.loads(str(fx["cases_json"]))
    return fx


# ---- the accept rule ---------------------------------------------------------------------------------------------------------------
def accept_ref(cand, logp, drafts, done, eos):
    """cand [R][U + 1] the target's picks at positions p .. p + U, logp their log-probabilities, drafts [R][U] the drafted tokens
    of positions p + 1 .. p + U, done [R] -> (a, new tokens [R][a], done afterwards [R], sum_logp increments [R]).
    m[r] = leading j < U with cand[r][j] == drafts[r][j], counting no further than a cand that is eos; a = min over the open
    rows of m[r] + 1 (1 without an open row).  An open row takes cand[r][:a], eos from its first eos on; a done row eos."""
    R, U = len(cand), len(cand[0]) - 1
    a = None
    for r in range(R):
        if done[r]:
            continue
        m = 0
        while m < U and cand[r][m] == drafts[r][m]:
            m += 1
            if cand[r][m - 1] == eos:
                break
        a = m + 1 if a is None else min(a, m + 1)
    a = 1 if a is None else a
    new, after, inc = [], [], []
    for r in range(R):
        row, closed, s = [], bool(done[r]), 0.0
        for i in range(a):
            if closed:
                row.append(eos)
                continue
            row.append(int(cand[r][i]))
            s += float(logp[r][i])
            closed = row[-1] == eos
        new.append(row)
        after.append(closed)
        inc.append(0.0 if done[r] else s)
    return a, new, after, inc


# Hand-made cases of the accept rule (eos = 9), each with what it must give, written out by hand: name, cand [R][U + 1], drafts
# [R][U], done [R] -> a, the new tokens [R][a], done afterwards, and per row how many leading picks' logp are kept.
ACCEPT_EOS = 9
ACCEPT_CASES = (
    dict(name="no match", cand=[[5, 6, 7, 8]], drafts=[[1, 2, 3]], done=[0], a=1, new=[[5]], after=[0], kept=[1]),
    dict(name="full match and the bonus token", cand=[[1, 2, 3, 4]], drafts=[[1, 2, 3]], done=[0], a=4, new=[[1, 2, 3, 4]], after=[0],
         kept=[4]),
    dict(name="eos in the middle", cand=[[1, 9, 3, 4]], drafts=[[1, 9, 3]], done=[0], a=3, new=[[1, 9, 9]], after=[1], kept=[2]),
    dict(name="eos drafted but not picked", cand=[[1, 2, 3, 4]], drafts=[[1, 9, 9]], done=[0], a=2, new=[[1, 2]], after=[0], kept=[2]),
    dict(name="a done row beside an open one", cand=[[1, 2, 7, 4], [3, 3, 3, 3]], drafts=[[1, 2, 3], [9, 9, 9]], done=[0, 1], a=3,
         new=[[1, 2, 7], [9, 9, 9]], after=[0, 1], kept=[3, 0]),
    dict(name="two open rows with different m", cand=[[1, 2, 3, 4], [5, 6, 0, 0]], drafts=[[1, 2, 3], [5, 7, 7]], done=[0, 0], a=2,
         new=[[1, 2], [5, 6]], after=[0, 0], kept=[2, 2]),
    dict(name="U = 1", cand=[[1, 2]], drafts=[[1]], done=[0], a=2, new=[[1, 2]], after=[0], kept=[2]),
    dict(name="eos picked against the draft", cand=[[9, 1, 1, 1]], drafts=[[4, 4, 4]], done=[0], a=1, new=[[9]], after=[1], kept=[1]),
    dict(name="a row closes inside the advance", cand=[[1, 9, 3, 4], [1, 2, 3, 4]], drafts=[[1, 9, 3], [1, 2, 3]], done=[0, 0], a=3,
         new=[[1, 9, 9], [1, 2, 3]], after=[1, 0], kept=[2, 3]),
    dict(name="no open row", cand=[[1, 2, 3, 4], [1, 2, 3, 4]], drafts=[[1, 2, 3], [1, 2, 3]], done=[1, 1], a=1, new=[[9], [9]],
         after=[1, 1], kept=[0, 0]),
)


def accept_logp(case):
    """The cases' log-probabilities: dyadic, so that every partial sum is exact in float32."""
    return [[-0.25 * (r + 1) * (j + 1) for j in range(len(row))] for r, row in enumerate(case["cand"])]


# ---- the picks -----------------------------------------------------------------------------------------------------------------------
def plain_pick(gen):
    """The greedy pick with the two suppress rules (``whisper_ref.Ref.greedy``): (history, logits, first step) -> (token, 0)."""
    sup, beg = list(gen["suppress_tokens"]), list(gen["begin_suppress_tokens"])

    def pick(_hist, x, first):
        x = np.array(x, dtype=np.float64)
        x[sup] = -np.inf
        if first:
            x[beg] = -np.inf
        return int(np.argmax(x)), 0.0
    return pick


def ruled_pick(gen):
    """The greedy pick under the timestamp rules (``whisper_long_ref.ts_pick_ref``) -> (token, its log-probability)."""
    eos, no_ts = gen["eos_token_id"], gen["no_timestamps_token_id"]

    def pick(hist, x, first):
        sup = list(gen["suppress_tokens"]) + (list(gen["begin_suppress_tokens"]) if first else [])
        tok, logp, _, _ = LR.ts_pick_ref(hist, x, eos, no_ts, gen.get("max_initial_timestamp_index"), sup)
        return tok, logp
    return pick


# ---- the round -------------------------------------------------------------------------------------------------------------------------
def assisted_ref(target, draft, prompts, cap, N, eos, pick):
    """``target(r, ids)`` / ``draft(r, ids)`` -> logits [len(ids)][V] of row r's prefix (position i predicts token i + 1);
    prompts [R][n0]; cap: the token bound; N drafts per round -> (tokens per row, cut behind the closing eos; sum of the picks'
    log-probabilities per row; {"rounds", "drafted", "accepted"}; the advance of every round)."""
    R, n0 = len(prompts), len(prompts[0])
    tokens, done, total = [list(p) for p in prompts], [False] * R, [0.0] * R
    stats, advances, p = dict(rounds=0, drafted=0, accepted=0), [], n0 - 1
    while p < cap - 1 and not all(done):
        U = min(N, cap - 2 - p)                               # the draft never steps past the bound
        hist = [list(t) for t in tokens]
        for r in range(R):                                    # U ordinary steps of the draft on its own table
            closed = done[r]
            for _ in range(U):
                tok = eos
                if not closed:
                    tok, _ = pick(hist[r][n0:], draft(r, hist[r])[-1], len(hist[r]) == n0)
                hist[r].append(tok)
                closed = closed or tok == eos
        cand, logp = [], []
        for r in range(R):                                    # one pass of the target over the drafted history
            x = target(r, hist[r])
            got = [pick(hist[r][n0:p + j + 1], x[p + j], p + j + 1 == n0) for j in range(U + 1)]
            cand.append([g[0] for g in got])
            logp.append([g[1] for g in got])
        a, new, done, inc = accept_ref(cand, logp, [h[p + 1:] for h in hist], done, eos)
        for r in range(R):
            tokens[r].extend(new[r])
            total[r] += inc[r]
        stats["rounds"] += 1
        stats["drafted"] += U
        stats["accepted"] += min(a - 1, U)
        advances.append(a)
        p += a
    out = []
    for row in tokens:
        gen = row[n0:]
        out.append(row[:n0 + gen.index(eos) + 1] if eos in gen else row)
    return out, total, stats, advances


def draft_gap(dref, denc, tokens, n0, gen):
    """How far the draft ``dref`` is from proposing the tokens the target picked (plain greedy rules): the smallest distance,
    over the generated positions, between the draft's largest allowed logit and its logit of the target's token, in units of the
    RMS of the draft's finite logits.  0: the draft proposes one of them.  A gap of 1e-2 or more means that an fp32 run of the
    same draft cannot propose it either (the margin the fixtures keep for the target's own picks)."""
    worst = np.inf
    for i in range(n0, len(tokens)):
        x = np.array(dref.decoder_logits(denc, tokens[:i])[-1], dtype=np.float64)
        x[list(gen["suppress_tokens"])] = -np.inf
        if i == n0:
            x[list(gen["begin_suppress_tokens"])] = -np.inf
        fin = x[np.isfinite(x)]
        worst = min(worst, float((fin.max() - x[tokens[i]]) / np.sqrt(np.mean(fin ** 2))))
    return worst


def model_fn(ref, encs):
    """``whisper_ref.Ref`` and the encoder outputs of the rows -> the callable ``assisted_ref`` takes, memoised per prefix."""
    memo = {}

    def fn(r, ids):
        key = (r, tuple(int(t) for t in ids))
        if key not in memo:
            memo[key] = ref.decoder_logits(encs[r], ids)
        return memo[key]
    return fn


# ---- the three drafts of the tests ------------------------------------------------------------------------------------------------------
def noisy_decoder_sd(sd, seed=5, rel=0.05):
    """The target with seeded noise on every decoder matrix (``rel`` x the matrix' own standard deviation): a draft that agrees
    with the target most of the time but not always."""
    g, out = np.random.default_rng(seed), {}
    for k in sorted(sd):                                      # by name: the same draft whatever order the weights come in
        v = np.asarray(sd[k], dtype=np.float32)
        if k.startswith("model.decoder.layers.") and v.ndim == 2:
            v = (v + rel * v.std() * g.standard_normal(v.shape)).astype(np.float32)
        out[k] = v
    return out


def random_sd(sd, seed=12):
    """A seeded random model of the target's shapes (the encoder's sinusoids stay): a draft that is wrong.  The seed is the
    first from 11 on with which ``draft_gap`` is at least 1e-2 on all four cases of whisper.npz (float64; 11 proposes one of the
    target's tokens), so that no round accepts anything there, in fp32 either, and the rounds equal the picks
    (tests/test_whisper_assist_cpu.py asserts the gap)."""
    g, out = np.random.default_rng(seed), {}
    for k in sorted(sd):
        v = np.asarray(sd[k], dtype=np.float32)
        if k == "model.encoder.embed_positions.weight":
            out[k] = v.copy()
        elif k.endswith("layer_norm.weight"):
            out[k] = np.ones_like(v)
        elif k.endswith("layer_norm.bias"):
            out[k] = np.zeros_like(v)
        else:
            out[k] = (max(float(v.std()), 1e-3) * g.standard_normal(v.shape)).astype(np.float32)
    return out


# ---- long form ------------------------------------------------------------------------------------------------------------------------
def transcribe_long_assisted_ref(ref, dref, feats, prompt, gen, cap, window, N, no_speech_threshold=None, logprob_threshold=None,
                                 denc_of=None):
    """``whisper_long_ref.transcribe_long_ref`` (greedy) with every window decoded by ``assisted_ref``: -> (segments, seeks, the
    assistant's figures summed over the windows).  ``denc_of(win, enc)``: the draft's encoder output (None: its own encoder)."""
    eos, tb = gen["eos_token_id"], gen["no_timestamps_token_id"] + 1
    T, seek, segs, seeks, tot = feats.shape[0], 0, [], [], dict(rounds=0, drafted=0, accepted=0)
    pick = ruled_pick(gen)
    while seek < T:
        seeks.append(seek)
        nf = min(window, T - seek)
        win = np.zeros((window, feats.shape[1]))
        win[:nf] = feats[seek:seek + nf]
        enc = ref.encoder(win)
        denc = dref.encoder(win) if denc_of is None else denc_of(win, enc)
        rows, total, st, _ = assisted_ref(model_fn(ref, [enc]), model_fn(dref, [denc]), [list(prompt)], cap, N, eos, pick)
        for k in tot:
            tot[k] += st[k]
        full = rows[0][len(prompt):]
        avg = total[0] / len(full)
        ns = LR.no_speech_prob_ref(ref, enc, gen)
        seq = full[:-1] if full[-1] == eos else full
        if no_speech_threshold is not None and avg < logprob_threshold and ns > no_speech_threshold:
            seek += nf
            continue
        parts, step = LR.split_ref(seq, tb, seek, nf)
        segs.extend(dict(start=s0, end=s1, tokens=tok, seek=seek, avg_logprob=avg, no_speech_prob=ns) for s0, s1, tok in parts)
        seek += step
    return segs, seeks, tot


__all__ = ["WR", "LR", "ACCEPT_CASES", "ACCEPT_EOS", "accept_logp", "accept_ref", "assisted_ref", "draft_gap", "load_fixture", "model_fn", "noisy_decoder_sd", "plain_pick", "random_sd",
           "ruled_pick", "transcribe_long_assisted_ref"]
