"""Float64 NumPy restatement of Whisper's sampled step and temperature fallback as ``transformers`` 5.15.0 runs them, on top of
tests/whisper_long_ref.py: the counter noise (``philox4x32_10``, ``uniform``, ``gumbel``, ``noise``), one sampled step under the
timestamp rules (``sample_pick_ref``: rules and log-probability at T = 1 on the raw logits, Gumbel-max on x / T + g), a sampled
window (``sampled_window_ref``), the decision of ``_need_fallback`` (``need_fallback_ref``) and the seek loop around
``generate_with_fallback`` (``transcribe_fallback_ref``).  Pinned to tests/golden/whisper_fallback.npz by
tests/test_whisper_fallback_cpu.py and used as the reference of the GPU tests.  It shares no code with f5e_tts_amd."""
import json
import math
import os
import zlib

import numpy as np

import whisper_long_ref as LR

HERE = os.path.dirname(os.path.abspath(__file__))
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


# ---- the noise -------------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """counter: 4 words (each an int or a uint64 array of one shape), key: 2 ints -> 4 words of the same shape."""
    c = [np.uint64(int(v) & MASK) if np.ndim(v) == 0 else np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in counter]   # i32 -> u32
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        a, b = np.uint64(M0) * c[0], np.uint64(M1) * c[2]            # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(b >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), b & np.uint64(MASK), (a >> np.uint64(32)) ^ c[3] ^ np.uint64(k1),
             a & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def uniform(w):
    """u = ((w >> 8) + 0.5) * 2^-24 in float64 (exact)."""
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def gumbel(w):
    """g = -log(-log(u)); the upper half through log1p(-(1 - u)), which loses nothing where 1 - u is small."""
    n = (np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(np.float64)
    lo = n < 2.0 ** 23
    e = np.where(lo, -np.log(np.where(lo, (n + 0.5) * 2.0 ** -24, 0.5)),
                 -np.log1p(-np.where(lo, 0.5, (2.0 ** 24 - 1.0 - n + 0.5) * 2.0 ** -24)))
    return -np.log(e)


def noise(V, step, serial, row_key, seed):
    """g [V] float64 of one row at one step: class i takes word i & 3 of the block with counter (i >> 2, step, serial, row_key)."""
    blocks = np.arange((V + 3) // 4, dtype=np.uint64)
    w = philox4x32_10((blocks, step, serial, row_key), (seed & MASK, (seed >> 32) & MASK))
    words = np.stack([np.broadcast_to(x, blocks.shape) for x in w], 1).reshape(-1)[:V]
    return gumbel(words)


# ---- one sampled step ------------------------------------------------------------------------------------------------------------
def sample_mask(hist, x, eos, no_ts, max_initial=None, suppress=()):
    """``LR.ts_mask``, or with ``no_ts`` None only the suppressed and the non-finite classes."""
    if no_ts is not None:
        return LR.ts_mask(hist, x, eos, no_ts, max_initial, suppress)[0]
    ban = ~np.isfinite(np.asarray(x, dtype=np.float64))
    ban[[t for t in suppress if 0 <= t < len(x)]] = True
    return ban


def sample_pick_ref(hist, x, eos, no_ts, T, seed, step, serial, row_key, max_initial=None, suppress=(), dtype=np.float64):
    """-> (pick, T = 1 log-probability of the pick among the allowed classes, gap between the two largest perturbed values).  The
    rules see the raw logits; the pick is the first maximum of x / T + g over the allowed classes, 0 when there is none."""
    ban = sample_mask(hist, x, eos, no_ts, max_initial, suppress)
    x64 = np.asarray(x, dtype=np.float64)
    if ban.all():
        return 0, 0.0, np.inf
    y = np.where(ban, -np.inf, np.where(ban, 0.0, x64) / T + noise(len(x64), step, serial, row_key, seed))
    pick = int(np.argmax(y))
    xd = np.asarray(x, dtype=dtype)
    ok = xd[~ban]
    m = ok.max()
    logp = float((xd[pick] - m) - np.log(np.exp(ok - m).sum(dtype=dtype)))
    top = np.sort(y[~ban])[::-1]
    return pick, logp, float(top[0] - top[1]) if len(top) > 1 else np.inf


def sampled_window_ref(ref, enc, prompt, gen, cap, T, seed, serial, row_key, timestamps=True):
    """One sampled decode: -> (generated tokens with the closing eos, sum of the picks' T = 1 log-probabilities, smallest rule gap
    and smallest perturbed pick gap relative to the logits' RMS)."""
    eos = gen["eos_token_id"]
    no_ts = gen["no_timestamps_token_id"] if timestamps else None
    ids, total, rule_gap, pick_gap = list(prompt), 0.0, np.inf, np.inf
    n0 = len(prompt)
    while len(ids) < cap:
        x = ref.decoder_logits(enc, ids)[-1]
        sup = list(gen["suppress_tokens"]) + (list(gen["begin_suppress_tokens"]) if len(ids) == n0 else [])
        pick, logp, gap = sample_pick_ref(ids[n0:], x, eos, no_ts, T, seed, len(ids) - 1, serial, row_key,
                                          gen.get("max_initial_timestamp_index"), sup)
        rms = math.sqrt(float(np.mean(np.square(x))))
        if timestamps:
            rule_gap = min(rule_gap, LR.ts_pick_ref(ids[n0:], x, eos, no_ts, gen.get("max_initial_timestamp_index"), sup)[2] / rms)
        pick_gap = min(pick_gap, gap / rms)
        ids.append(pick)
        total += logp
        if pick == eos:
            break
    return ids[n0:], total, rule_gap, pick_gap


# ---- fallback --------------------------------------------------------------------------------------------------------------------
def compression_ratio_ref(tokens, vocab_size):
    width = int(math.log2(vocab_size) / 8) + 1
    raw = b"".join(int(t).to_bytes(width, "little") for t in tokens)
    return len(raw) / len(zlib.compress(raw))


def need_fallback_ref(cr, avg, ns, cr_thr, lp_thr, ns_thr):
    """``_need_fallback``: -> (needs_fallback, should_skip)."""
    need = (cr_thr is not None and cr > cr_thr) or (lp_thr is not None and avg < lp_thr)
    if ns_thr is not None and avg < lp_thr and ns > ns_thr:
        return False, True
    return bool(need), False


def transcribe_fallback_ref(ref, feats, prompt, gen, cap, window, vocab, temperatures, cr_thr=None, lp_thr=None, ns_thr=None, K=1,
                            seed=0, row_key=0):
    """``LR.transcribe_long_ref`` around ``generate_with_fallback``: every window is decoded at temperatures[0], and again at the
    next temperature while ``need_fallback_ref`` asks for it; the last attempt is kept.  Temperature 0 is the greedy (K = 1) or
    beam decode, a positive one a sampled single row with serial = the sampled decodes this recording has started before.
    -> (segments as dicts with the window's temperature, seeks, per window the list of attempts (temperature, compression ratio,
    average log-probability, needs_fallback, should_skip), the smallest relative margins [rule, greedy pick, sampled pick])."""
    eos, tb = gen["eos_token_id"], gen["no_timestamps_token_id"] + 1
    T, seek, segs, seeks, windows, gaps, serial = feats.shape[0], 0, [], [], [], [np.inf, np.inf, np.inf], 0
    while seek < T:
        seeks.append(seek)
        nf = min(window, T - seek)
        win = np.zeros((window, feats.shape[1]))
        win[:nf] = feats[seek:seek + nf]
        enc = ref.encoder(win)
        ns = LR.no_speech_prob_ref(ref, enc, gen)
        attempts = []
        for temp in temperatures:
            if temp > 0:
                full, total, rg, sg = sampled_window_ref(ref, enc, prompt, gen, cap, temp, seed, serial, row_key)
                serial += 1
                gaps = [min(gaps[0], rg), gaps[1], min(gaps[2], sg)]
                avg = total / len(full)
            elif K == 1:
                full, total, rg, pg = LR.greedy_window_ref(ref, enc, prompt, gen, cap)
                gaps = [min(gaps[0], rg), min(gaps[1], pg), gaps[2]]
                avg = total / len(full)
            else:
                full, avg = LR.beam_window_ref(ref, enc, prompt, gen, cap, K), float("nan")
            cr = compression_ratio_ref(full, vocab)
            need, skip = need_fallback_ref(cr, avg, ns, cr_thr, lp_thr, ns_thr)
            attempts.append((float(temp), cr, avg, need, skip))
            if not need:
                break
        windows.append(attempts)
        seq = full[:-1] if full[-1] == eos else full
        if skip:
            seek += nf
            continue
        parts, step = LR.split_ref(seq, tb, seek, nf)
        segs.extend(dict(start=s0, end=s1, tokens=tok, seek=seek, avg_logprob=avg, no_speech_prob=ns, temperature=float(temp))
                    for s0, s1, tok in parts)
        seek += step
    return segs, seeks, windows, gaps


# ---- the fixture -----------------------------------------------------------------------------------------------------------------
def load_fixture():
    """tests/golden/whisper_fallback.npz: the cases, on the model, wave and configs of tests/golden/whisper_long.npz."""
    fx = LR.load_fixture()
    z = np.load(os.path.join(HERE, "golden", "whisper_fallback.npz"))
    fx["cases"] = json.loads(str(z["cases_json"]))
    fx["fallback_seed"] = int(z["seed"])
    for k in z.files:
        if k.startswith("rows_"):
            fx[k] = z[k]
    return fx


# ---- inputs of the step tests (tests/test_whisper_fallback_gpu.py; their caps are proved on this oracle alone by the CPU test) ------
PICK_SHAPES = ((5, 1), (7, 3), (162, 3), (1025, 1), (51866, 3))
PICK_TEMPERATURES = (0.2, 1.0)
PICK_SEED = 0x1234_5678_9ABC_DEF0


def pick_layout(V):
    """-> (eos, no_ts, suppress, begin_suppress, max_initial) for a row of V classes: a third of them timestamps."""
    if V < 8:
        return 1, 2, [0] if V > 5 else [], [], None
    no_ts = V - V // 3 - 1
    eos = no_ts - 10 if V > 64 else no_ts - 2
    return eos, no_ts, [1, 2, 7, eos + 1], [5, eos], (V // 3) // 2


def pick_histories(V):
    """One history per rule state: first step, 2 (timestamp after nothing / a pair), 3 (text, timestamp), 4 (plain text)."""
    eos, no_ts, *_ = pick_layout(V)
    tb, t = no_ts + 1, 0
    return [[], [tb], [tb, t, tb + 1] if V - tb > 1 else [tb, t, tb], [tb, t, t]]


def pick_inputs(V, R, T):
    """-> list over the histories of (hist, x f32 [R, V], row_key i32 [R], serial i32 [R]).  |x| <= 12, so |x / T| <= 60."""
    g = np.random.default_rng(V * 131 + R * 7 + int(T * 10))
    out = []
    for h, hist in enumerate(pick_histories(V)):
        x = np.clip(g.standard_normal((R, V)) * 3.0, -12.0, 12.0).astype(np.float32)
        if V > 64:
            x[:, -(V // 3):] -= np.float32(2.0 if h % 2 else 6.0)      # the timestamps' sum against the best text
        x = np.clip(x, -12.0, 12.0)
        out.append((hist, x, np.array([1000 + 17 * r + h for r in range(R)], np.int32), np.array([3 + r for r in range(R)], np.int32)))
    return out


def pick_tau(T, xmax=12.0):
    """The fp32 evaluation error of a GAP of x / T + g as the kernel computes it (twice the error of one value): the division
    (2.5 ulp allowed) on |x / T| <= xmax / T, e = -log(u) or -log1p(-(1 - u)) from an exact argument (3 ulp of e, which moves
    log(e) by 3 * 2^-23), g = -log(e) (3 ulp of |g| <= 17.33 < 32: 3 * 2^-19), and the rounding of the sum (half an ulp of
    |y| < 128: 2^-18)."""
    return 2.0 * (2.5 * 2.0 ** -23 * xmax / T + 3.0 * 2.0 ** -23 + 3.0 * 2.0 ** -19 + 2.0 ** -18)
