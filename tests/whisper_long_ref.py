"""Float64 NumPy restatement of Whisper's timestamp decoding as ``transformers`` 5.15.0 runs it: the bans of
``WhisperTimeStampLogitsProcessor`` (``ts_mask``), one greedy and one beam step under them (``ts_pick_ref``, ``beam_step_ts_ref``),
the slicing of a window's tokens into segments (``split_ref``, ``_retrieve_segment``) and the sequential seek loop of the long-form
``generate`` with ``condition_on_prev_tokens=False`` at temperature 0 (``transcribe_long_ref``), around ``whisper_ref.Ref``'s encoder
and decoder.  Pinned to tests/golden/whisper_long.npz by tests/test_whisper_long_cpu.py and used as the reference of the GPU
tests.  It shares no code with f5e_tts_amd."""
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_fixture():
    z = np.load(os.path.join(HERE, "golden", "whisper_long.npz"))
    fx = {k: z[k] for k in z.files if not k.startswith("w/")}
    fx["sd"] = {k[2:]: (z[k].astype(np.uint32) << 16).view(np.float32) for k in z.files if k.startswith("w/")}
    fx["config"] = json.loads(str(fx["config_json"]))
    fx["generation_config"] = json.loads(str(fx["generation_config_json"]))
    fx["cases"] = json.loads(str(fx["cases_json"]))
    fx["wave_f32"] = fx["wave"].astype(np.float32) / 32768.0
    return fx


def case_sd(fx, case):
    """The weights of a case: the shared model with the case's own scaled rows of the tied embedding."""
    sd = dict(fx["sd"])
    emb = sd["model.decoder.embed_tokens.weight"].copy()
    for lo, hi, fac in case["row_scale"]:
        emb[lo:hi] = (fx["rows_" + case["name"] + f"_{lo}"].astype(np.uint32) << 16).view(np.float32)
    sd["model.decoder.embed_tokens.weight"] = emb
    return sd


# ---- the rules -----------------------------------------------------------------------------------------------------------------------
def ts_mask(hist, x, eos, no_ts, max_initial=None, suppress=()):
    """hist: the generated tokens of a row, x [V] its logits -> bool [V], True = banned: the suppressed classes, the bans of the
    processor, and all text when log-sum-exp(allowed timestamps) > max(allowed text).  NaN and infinite logits count as banned."""
    x = np.asarray(x, dtype=np.float64)
    V, tb = len(x), no_ts + 1
    ban = ~np.isfinite(x)
    ban[[t for t in suppress if 0 <= t < V]] = True
    ban[no_ts] = True
    hist = [int(t) for t in hist]
    last_ts = len(hist) >= 1 and hist[-1] >= tb
    pen_ts = len(hist) < 2 or hist[-2] >= tb
    if last_ts:
        if pen_ts:
            ban[tb:] = True
        else:
            ban[:eos] = True
    stamps = [t for t in hist if t >= tb]
    if stamps:
        ban[tb:min(stamps[-1] if (last_ts and not pen_ts) else stamps[-1] + 1, V)] = True
    if not hist:
        ban[:tb] = True
        if max_initial is not None:
            ban[tb + max_initial + 1:] = True
    ts_ok, tx_ok = ~ban[tb:], ~ban[:tb]
    lse_ts = _lse(x[tb:][ts_ok])
    max_tx = x[:tb][tx_ok].max() if tx_ok.any() else -np.inf
    if lse_ts > max_tx:
        ban[:tb] = True
    return ban, (lse_ts, max_tx)


def _lse(v, dtype=np.float64):
    v = np.asarray(v, dtype=dtype)
    if v.size == 0:
        return -np.inf
    m = v.max()
    return float(m + np.log(np.exp(v - m).sum(dtype=dtype)))


def ts_pick_ref(hist, x, eos, no_ts, max_initial=None, suppress=(), dtype=np.float64):
    """-> (pick, log-probability of the pick among the allowed classes, |lse_ts - max_text|, top-1 / top-2 gap).  ``dtype``
    float32 evaluates the log-probability's formula (x[pick] - M) - log(sum exp(x - M)) in float32 (the bound of the GPU test)."""
    ban, (lse_ts, max_tx) = ts_mask(hist, x, eos, no_ts, max_initial, suppress)
    xs = np.where(ban, -np.inf, np.asarray(x, dtype=np.float64))
    if not np.isfinite(xs).any():
        return 0, 0.0, np.inf, np.inf
    pick = int(np.argmax(xs))
    ok = np.asarray(x, dtype=dtype)[~ban]
    m = ok.max()
    logp = float((np.asarray(x, dtype=dtype)[pick] - m) - np.log(np.exp(ok - m).sum(dtype=dtype)))
    top = np.sort(xs[np.isfinite(xs)])[::-1]
    with np.errstate(invalid="ignore"):
        rule_gap = abs(lse_ts - max_tx) if np.isfinite(lse_ts) and np.isfinite(max_tx) else np.inf
    return pick, logp, float(rule_gap), float(top[0] - top[1]) if len(top) > 1 else np.inf


def desc_mask(desc, V, eos, no_ts, suppress=()):
    """The ban mask a rule descriptor (kind, lo, hi, .) of f5e_whisper_ts_rule stands for, finite logits assumed."""
    kind, lo, hi = int(desc[0]), int(desc[1]), int(desc[2])
    tb = no_ts + 1
    ban = np.zeros(V, bool)
    ban[[t for t in suppress if 0 <= t < V]] = True
    ban[no_ts] = True
    ban[:tb if kind == 2 else eos if kind == 1 else 0] = True
    v = np.arange(V)
    ban |= (v >= tb) & ((v < lo) | (v > hi))
    return ban


def beam_step_ts_ref(logits, st, p, n0, cap, eos, K, no_ts, max_initial=None, suppress=(), begin_suppress=(), length_penalty=1.0):
    """whisper_beam_ref.beam_step_ref under the rules: the log-probabilities are normalised over ALL raw classes, then the classes
    banned for the row's own history st["hyp"][r, n0:p + 1] become -inf."""
    x = np.asarray(logits, dtype=np.float64)
    R, V = x.shape
    B = R // K
    out = {k: np.array(v, copy=True) for k, v in st.items()}
    gap = np.inf
    mx = x.max(1, keepdims=True)
    logp = (x - mx) - np.log(np.exp(x - mx).sum(1, keepdims=True))
    sup = list(suppress) + (list(begin_suppress) if p + 1 == n0 else [])
    for r in range(R):
        ban, (a, b_) = ts_mask(st["hyp"][r, n0:p + 1], x[r], eos, no_ts, max_initial, sup)
        logp[r, ban] = -np.inf
        if st["score"][r] > -np.inf and np.isfinite(a) and np.isfinite(b_):
            gap = min(gap, abs(a - b_))
    denom = float(p + 2 - n0) ** length_penalty
    for b in range(B):
        r0 = b * K
        with np.errstate(invalid="ignore"):
            cand = (st["score"][r0:r0 + K, None] + logp[r0:r0 + K]).reshape(-1)
        cand = np.where(np.isfinite(cand), cand, -np.inf)
        order = np.argsort(-cand, kind="stable")[:2 * K + 1]
        order = [int(i) for i in order if cand[i] > -np.inf]
        vals = [cand[i] for i in order]
        gap = min([gap] + [vals[i] - vals[i + 1] for i in range(len(vals) - 1)])
        order, vals = order[:2 * K], vals[:2 * K]
        hit = [(i % V) == eos or p + 2 >= cap for i in order]
        run = [j for j in range(len(order)) if not hit[j]][:K]
        for q in range(K):
            if q < len(run):
                par, cls = divmod(order[run[q]], V)
                out["score"][r0 + q] = vals[run[q]]
            else:
                par, cls = q, eos
                out["score"][r0 + q] = -np.inf
            out["hyp"][r0 + q, :p + 1] = st["hyp"][r0 + par, :p + 1]
            out["hyp"][r0 + q, p + 1] = cls
            out["anc"][r0 + q, :p] = st["anc"][r0 + par, :p]
            out["anc"][r0 + q, p] = r0 + par
            out["last"][r0 + q] = cls
        n = int(st["pool_n"][b])
        pool = [(st["pool_score"][b, s], st["pool_hyp"][b, s].copy(), int(st["pool_len"][b, s])) for s in range(n)]
        if st["open"][b]:
            for j in range(min(K, len(order))):
                if hit[j]:
                    par, cls = divmod(order[j], V)
                    row = np.full(st["hyp"].shape[1], eos, np.int64)
                    row[:p + 1] = st["hyp"][r0 + par, :p + 1]
                    row[p + 1] = cls
                    sc = vals[j] / denom
                    pos = len(pool)
                    while pos > 0 and pool[pos - 1][0] < sc:
                        pos -= 1
                    pool.insert(pos, (sc, row, p + 2))
                    pool = pool[:K]
        for s, (sc, row, ln) in enumerate(pool):
            out["pool_score"][b, s], out["pool_len"][b, s] = sc, ln
            out["pool_hyp"][b, s, :ln] = row[:ln]
        out["pool_n"][b] = len(pool)
        gap = min([gap] + [pool[s][0] - pool[s + 1][0] for s in range(len(pool) - 1)])
        op = int(st["open"][b])
        if len(pool) == K:
            best = out["score"][r0] / denom
            if op and np.isfinite(best):
                gap = min(gap, abs(best - pool[K - 1][0]))
            op = int(op and best > pool[K - 1][0])
        out["open"][b] = op
        out["alive"][b] = int(op and not all(hit))
    return out, float(gap)


# ---- one window ------------------------------------------------------------------------------------------------------------------------
def greedy_window_ref(ref, enc, prompt, gen, cap):
    """-> (generated tokens with the closing eos, sum of the picks' log-probabilities, smallest rule gap, smallest pick gap)."""
    eos, no_ts = gen["eos_token_id"], gen["no_timestamps_token_id"]
    ids, total, rule_gap, pick_gap = list(prompt), 0.0, np.inf, np.inf
    n0 = len(prompt)
    while len(ids) < cap:
        x = ref.decoder_logits(enc, ids)[-1]
        sup = list(gen["suppress_tokens"]) + (list(gen["begin_suppress_tokens"]) if len(ids) == n0 else [])
        pick, logp, rg, pg = ts_pick_ref(ids[n0:], x, eos, no_ts, gen.get("max_initial_timestamp_index"), sup)
        rms = math.sqrt(float(np.mean(np.square(x))))
        rule_gap, pick_gap = min(rule_gap, rg / rms), min(pick_gap, pg / rms)
        ids.append(pick)
        total += logp
        if pick == eos:
            break
    return ids[n0:], total, rule_gap, pick_gap


def beam_window_ref(ref, enc, prompt, gen, cap, K):
    """-> the best hypothesis' generated tokens (closing eos included when it has one)."""
    import whisper_beam_ref as BR
    eos, n0 = gen["eos_token_id"], len(prompt)
    st = BR.new_state(1, K, cap, prompt, eos)
    V = ref.w("model.decoder.embed_tokens.weight").shape[0]
    for p in range(n0 - 1, cap - 1):
        logits = np.zeros((K, V))
        for q in range(K):
            if st["score"][q] > -np.inf:
                logits[q] = ref.decoder_logits(enc, st["hyp"][q, :p + 1])[-1]
        st, _ = beam_step_ts_ref(logits, st, p, n0, cap, eos, K, gen["no_timestamps_token_id"], gen.get("max_initial_timestamp_index"),
                                 gen["suppress_tokens"], gen["begin_suppress_tokens"])
        if not st["alive"][0]:
            break
    return [int(t) for t in st["pool_hyp"][0, 0, n0:st["pool_len"][0, 0]]]


def no_speech_prob_ref(ref, enc, gen):
    x = ref.decoder_logits(enc, [gen["decoder_start_token_id"]])[-1]
    return float(np.exp(x[gen["no_timestamps_token_id"] - 1] - _lse(x)))


def detect_language_ref(ref, enc, gen):
    x = ref.decoder_logits(enc, [gen["decoder_start_token_id"]])[-1]
    ids = sorted(gen["lang_to_id"].values())
    return ids[int(np.argmax(x[ids]))]


# ---- segments and the seek loop --------------------------------------------------------------------------------------------------------
def split_ref(seq, tb, seek, num_frames):
    """-> ([(start, end, tokens)], frames to advance): ``_retrieve_segment`` with time_precision 0.02 and input_stride 2."""
    seq = [int(t) for t in seq]
    ts = np.array([t >= tb for t in seq])
    off = np.float64(seek) * 0.02 / 2
    single = ts[-2:].tolist() == [False, True]
    idx = (np.where(ts[:-1] & ts[1:])[0] + 1).tolist()
    if idx:
        if single:
            idx.append(len(seq))
        else:
            idx[-1] += 1
        segs, last = [], 0
        for i, cur in enumerate(idx):
            sl = seq[last:cur]
            e = sl[-1] if (i != len(idx) - 1 or single) else sl[-2]
            segs.append((float(off + np.float64(sl[0] - tb) * 0.02), float(off + np.float64(e - tb) * 0.02), sl))
            last = cur
        return segs, num_frames if single else (seq[last - 2] - tb) * 2
    stamps = [t for t in seq if t >= tb]
    pos = int(np.float32(num_frames) * np.float32(0.01) / np.float32(0.02))
    if stamps and stamps[-1] != tb:
        pos = np.float64(stamps[-1] - tb)
    return [(float(off), float(off + pos * 0.02), seq)], num_frames


def transcribe_long_ref(ref, feats, prompt, gen, cap, window, K=1, no_speech_threshold=None, logprob_threshold=None):
    """feats [T][n_mels]: the features of one recording -> (segments as dicts, the seek at the start of every window, the
    smallest relative rule / pick gaps of the greedy windows, one letter per window: k skipped, p cut at a timestamp pair, s
    single-timestamp ending, n no pair, N no pair and the token bound reached without eos)."""
    eos, tb = gen["eos_token_id"], gen["no_timestamps_token_id"] + 1
    T, seek, segs, seeks, gaps, kinds = feats.shape[0], 0, [], [], [np.inf, np.inf], ""
    while seek < T:
        seeks.append(seek)
        nf = min(window, T - seek)
        win = np.zeros((window, feats.shape[1]))
        win[:nf] = feats[seek:seek + nf]
        enc = ref.encoder(win)
        if K == 1:
            full, total, rg, pg = greedy_window_ref(ref, enc, prompt, gen, cap)
            gaps = [min(gaps[0], rg), min(gaps[1], pg)]
            avg = total / len(full)
        else:
            full, avg = beam_window_ref(ref, enc, prompt, gen, cap, K), float("nan")
        ns = no_speech_prob_ref(ref, enc, gen)
        seq = full[:-1] if full[-1] == eos else full
        if no_speech_threshold is not None and avg < logprob_threshold and ns > no_speech_threshold:
            seek += nf
            kinds += "k"
            continue
        parts, step = split_ref(seq, tb, seek, nf)
        pair = any(a >= tb and b >= tb for a, b in zip(seq[:-1], seq[1:]))
        kinds += ("p" if step < nf else "s") if pair else ("N" if len(full) == cap - len(prompt) and full[-1] != eos else "n")
        segs.extend(dict(start=s0, end=s1, tokens=tok, seek=seek, avg_logprob=avg, no_speech_prob=ns) for s0, s1, tok in parts)
        seek += step
    return segs, seeks, gaps, kinds
