"""Float64 NumPy restatement of Whisper's pooled beam search as ``transformers`` 5.15.0 runs it (``GenerationMixin._beam_search``,
``early_stopping=False``, ``do_sample=False``), its -1e9 sentinels replaced by flags.  ``beam_step_ref`` is the contract of
f5e_whisper_beam_step (include/f5e_abi.h has the same rules in words); ``beam_search_ref`` is the loop around
``whisper_ref.Ref``'s decoder, without a cache: every open row's whole prefix goes through the decoder at every step.  Pinned to
tests/golden/whisper_beam.npz by tests/test_whisper_beam_cpu.py and used as the reference of the GPU tests.  It shares no code
with f5e_tts_amd/eval/whisper.py."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_fixture():
    z = np.load(os.path.join(HERE, "golden", "whisper_beam.npz"))
    fx = {k: z[k] for k in z.files if not k.startswith("w")}
    fx["models"] = []
    for m in range(int(z["n_models"])):
        pre = f"w{m}/"
        fx["models"].append({k[len(pre):]: (z[k].astype(np.uint32) << 16).view(np.float32) for k in z.files if k.startswith(pre)})
    fx["config"] = json.loads(str(fx["config_json"]))
    fx["generation_config"] = json.loads(str(fx["generation_config_json"]))
    fx["n_cases"] = int(z["n_cases"])
    return fx


def new_state(B, K, ld, prompt, eos):
    """The state before the first pick: the prompt in every row, a row's own cache for the prompt's positions, an empty pool."""
    R, n0 = B * K, len(prompt)
    hyp = np.full((R, ld), eos, np.int64)
    hyp[:, :n0] = np.asarray(prompt)
    anc = np.repeat(np.arange(R)[:, None], ld, 1)
    score = np.full((B, K), -np.inf)
    score[:, 0] = 0.0
    return dict(score=score.reshape(R), hyp=hyp, anc=anc, last=hyp[:, n0 - 1].copy(), pool_hyp=np.full((B, K, ld), eos, np.int64),
                pool_len=np.zeros((B, K), np.int64), pool_score=np.full((B, K), -np.inf), pool_n=np.zeros(B, np.int64),
                open=np.ones(B, np.int64), alive=np.ones(B, np.int64))


def beam_step_ref(logits, st, p, n0, cap, eos, K, suppress=(), begin_suppress=(), length_penalty=1.0):
    """One step.  logits [B * K][V] (raw), ``st`` as ``new_state`` makes it -> (the state after the step, the smallest gap that
    decided anything in it: between neighbours of the top 2K + 1 candidates, between neighbouring pool scores, and between the
    best open row's normalised score and the worst pool entry when the pool is full)."""
    x = np.asarray(logits, dtype=np.float64)
    R, V = x.shape
    B = R // K
    out = {k: np.array(v, copy=True) for k, v in st.items()}
    gap = np.inf
    mx = x.max(1, keepdims=True)
    logp = (x - mx) - np.log(np.exp(x - mx).sum(1, keepdims=True))          # rule 1: over ALL classes, then suppress
    banned = [t for t in suppress if 0 <= t < V] + ([t for t in begin_suppress if 0 <= t < V] if p + 1 == n0 else [])
    logp[:, banned] = -np.inf
    denom = float(p + 2 - n0) ** length_penalty
    for b in range(B):
        r0 = b * K
        with np.errstate(invalid="ignore"):
            cand = (st["score"][r0:r0 + K, None] + logp[r0:r0 + K]).reshape(-1)     # rule 2; index = row * V + class
        cand = np.where(np.isfinite(cand), cand, -np.inf)
        order = np.argsort(-cand, kind="stable")[:2 * K + 1]                # rule 3: ties to the lower row, then class
        order = [int(i) for i in order if cand[i] > -np.inf]
        vals = [cand[i] for i in order]
        gap = min([gap] + [vals[i] - vals[i + 1] for i in range(len(vals) - 1)])
        order, vals = order[:2 * K], vals[:2 * K]
        hit = [(i % V) == eos or p + 2 >= cap for i in order]
        run = [j for j in range(len(order)) if not hit[j]][:K]
        for q in range(K):                                                   # rule 4
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
        if st["open"][b]:                                                    # rule 5
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
        if len(pool) == K:                                                   # rule 6
            best = out["score"][r0] / denom
            if op and np.isfinite(best):
                gap = min(gap, abs(best - pool[K - 1][0]))
            op = int(op and best > pool[K - 1][0])
        out["open"][b] = op
        out["alive"][b] = int(op and not all(hit))                           # rule 7
    return out, float(gap)


def beam_search_ref(ref, enc, prompt, suppress, begin_suppress, eos, cap, K, length_penalty=1.0):
    """One utterance.  -> (pool tokens [K][cap] (eos beyond an entry's length), lens [K], scores [K], steps taken, smallest gap)."""
    n0 = len(prompt)
    st = new_state(1, K, cap, prompt, eos)
    gap, steps = np.inf, 0
    for p in range(n0 - 1, cap - 1):
        logits = np.zeros((K, ref.w("model.decoder.embed_tokens.weight").shape[0]))
        for q in range(K):
            if st["score"][q] > -np.inf:
                logits[q] = ref.decoder_logits(enc, st["hyp"][q, :p + 1])[-1]
        st, g = beam_step_ref(logits, st, p, n0, cap, eos, K, suppress, begin_suppress, length_penalty)
        gap, steps = min(gap, g), steps + 1
        if not st["alive"][0]:
            break
    toks = np.full((K, cap), eos, np.int64)
    for s in range(K):
        toks[s, :st["pool_len"][0, s]] = st["pool_hyp"][0, s, :st["pool_len"][0, s]]
    return toks, st["pool_len"][0].copy(), st["pool_score"][0].copy(), steps, gap
