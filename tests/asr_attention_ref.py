"""NumPy / torch restatement, in fp64 and fp32, of the attention decoder's beam search (reference ``ASRModel.recognize``,
ppg/asr_model.py:309-414, with ``TransformerDecoder.forward_one_step``, decoder.py:137-181, decoder_layer.py:86-137):

* ``beam_step``: one step -- first prune, ``mask_finished_scores`` / ``mask_finished_preds``, score + logp, second prune,
  hypothesis and ancestry update -- with the ties the reference's ``topk`` leaves open settled as the kernel settles them
  (lower class first; lower (parent row, rank) first);
* ``search``: the loop with its early stop, over any ``logp(p, hyp, anc)`` callback;
* ``CachedDecoder``: the decoder one position at a time with per-layer key / value caches in both cache modes.  The
  reference caches each layer's OUTPUT rows and never reorders them when the second prune reshuffles the beam
  (asr_model.py:397-400 gathers ``hyps`` only): the keys of layer 0 come from the re-embedded, reordered hypotheses, those
  of the layers above from whatever their row index computed at that step.  ``reorder=False`` is that; ``reorder=True``
  follows the ancestry in every layer, which equals recomputing the decoder on the whole prefix at every step;
* ``margin``: the smallest gap over every decision of a run and E, the largest fp32-vs-fp64 difference of a kept score.

Pinned against the reference's own outputs by tests/golden/asr_attention.npz (tests/golden/make_asr_attention_golden.py);
the GPU tests compare f5e_beam_step, f5e_attn_decode_f32 and ``ConformerPPG.recognize`` to it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

# (B, maxlen, V, beam, plant): the loop cases; their table seeds are in the fixture (``loop<i>_seed``).  plant "early": eos
# is boosted in every row from step 4 on, so that every hypothesis finishes well before maxlen; "never": eos is pushed down
# so that no row ever finishes
LOOP_CASES = [
    (1, 12, 9, 1, None),
    (1, 20, 12, 4, None),
    (2, 30, 40, 10, None),
    (3, 25, 70, 16, None),
    (1, 6, 5, 5, None),
    (2, 24, 20, 4, "early"),
    (1, 10, 16, 4, "never"),
]


def loop_table(maxlen, V, seed, plant=None, scale=16.0):
    """The seeded table of a loop case: log-probabilities f32 [maxlen, V, V] indexed by (step, last token).  Built from
    32-bit integers so that it does not depend on a library's floating-point sampler."""
    u = np.random.default_rng(seed).integers(0, 1 << 32, size=(maxlen, V, V), dtype=np.uint64).astype(np.float64)
    x = (u / 4294967296.0 - 0.5) * 2.0 * scale
    if plant == "early":
        x[4:, :, V - 1] += 4.0 * scale
    if plant == "never":
        x[:, :, V - 1] -= 4.0 * scale
    x = x - x.max(-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)


def start(B, beam, sos, width, dtype=np.float64):
    """The reference's start state: hyp [R, width] (column 0 = sos), anc [R, width], score 0, -inf, ... per utterance."""
    R = B * beam
    hyp, anc = np.zeros((R, width), np.int64), np.zeros((R, width), np.int64)
    hyp[:, 0] = sos
    score = np.tile(np.array([0.0] + [-np.inf] * (beam - 1), dtype), B)
    return hyp, anc, score


def beam_step(logp, score, hyp, anc, p, beam, eos, dtype=np.float64):
    """One step on log-probabilities [R, V]: hyp / anc [R, >= p + 2] hold columns 0..p / 0..p-1.  -> (score, hyp, anc, alive
    [B], gaps): new tables (copies), rows not ending in eos per utterance, and the decision gaps of the step -- first prune
    rank beam vs beam + 1 of every alive row with a finite score; second prune every adjacent pair of kept entries and the
    last kept against the first dropped; finite candidates only."""
    logp = np.asarray(logp, dtype)
    R, V = logp.shape
    B = R // beam
    finished = (hyp[:, p] == eos) if p > 0 else np.zeros(R, bool)
    order = np.argsort(-logp, axis=1, kind="stable")            # value descending, class ascending
    top_i = order[:, :beam].copy()
    top_v = np.take_along_axis(logp, top_i, 1)
    gaps = []
    if V > beam:
        nxt_v = np.take_along_axis(logp, order[:, beam:beam + 1], 1)[:, 0]
        gaps += [float(top_v[r, -1] - nxt_v[r]) for r in range(R) if not finished[r] and np.isfinite(score[r])]
    top_v[finished, 0], top_v[finished, 1:], top_i[finished] = 0.0, -np.inf, eos
    cand = (np.asarray(score, dtype)[:, None] + top_v).astype(dtype).reshape(B, beam * beam)
    n_score, n_hyp, n_anc = np.empty(R, dtype), hyp.copy(), anc.copy()
    alive = np.zeros(B, np.int64)
    for b in range(B):
        rank = np.argsort(-cand[b], kind="stable")              # value descending, (parent row, rank) ascending
        keep = rank[:beam]
        vals = cand[b][rank[:beam + 1]].astype(np.float64)
        gaps += [float(vals[i] - vals[i + 1]) for i in range(len(vals) - 1) if np.isfinite(vals[i]) and np.isfinite(vals[i + 1])]
        for q, c in enumerate(keep):
            par, cls = b * beam + c // beam, top_i[b * beam + c // beam, c % beam]
            n_score[b * beam + q] = cand[b][c]
            n_hyp[b * beam + q, :p + 1], n_hyp[b * beam + q, p + 1] = hyp[par, :p + 1], cls
            n_anc[b * beam + q, :p], n_anc[b * beam + q, p] = anc[par, :p], par
            alive[b] += cls != eos
    return n_score, n_hyp, n_anc, alive, gaps


def search(logp_fn, B, beam, maxlen, sos, eos, dtype=np.float64, early_stop=True):
    """The loop: ``logp_fn(p, hyp, anc)`` -> log-probabilities [R, V] of step p.  -> dict(hyp [R, L + 1], anc, score [R],
    done_at [B], steps, delta, kept = the kept scores of every step, trace = (score, hyp, anc, alive, done_at) after every
    step).  ``early_stop`` False runs all maxlen steps."""
    hyp, anc, score = start(B, beam, sos, maxlen + 1, dtype)
    hyp[:, 1:] = eos
    done_at, delta, kept, steps, trace = np.full(B, -1, np.int64), np.inf, [], 0, []
    for p in range(maxlen):
        if early_stop and p > 0 and bool((hyp[:, p] == eos).all()):
            break
        score, hyp, anc, alive, gaps = beam_step(logp_fn(p, hyp, anc), score, hyp, anc, p, beam, eos, dtype)
        done_at = np.where((alive == 0) & (done_at < 0), p, done_at)
        delta = min([delta] + gaps)
        kept.append(score.copy())
        trace.append((score.copy(), hyp[:, :p + 2].copy(), anc[:, :p + 1].copy(), alive, done_at.copy()))
        steps = p + 1
    return dict(hyp=hyp[:, :steps + 1], anc=anc[:, :steps], score=score, done_at=done_at, steps=steps, delta=float(delta),
                kept=kept, trace=trace)


def table_fn(table):
    return lambda p, hyp, anc: table[p][hyp[:, p]]


def best(res, B, beam):
    """``recognize``'s return: hyps[:, 1:] of each utterance's max-score row (the first maximum) and its score."""
    sc = res["score"].reshape(B, beam)
    idx = sc.argmax(1)
    return res["hyp"].reshape(B, beam, -1)[np.arange(B), idx, 1:], sc[np.arange(B), idx]


def margin(make_fn, B, beam, maxlen, sos, eos, early_stop=True):
    """``make_fn(dtype)`` -> a fresh logp callback computing in that precision.  -> (fp64 result, delta, E, same): delta
    = the smallest decision gap of the fp64 run, E = the largest |fp32 - fp64| over every kept score of every step, ``same``
    = the fp32 run gives the same tables."""
    r64 = search(make_fn(np.float64), B, beam, maxlen, sos, eos, np.float64, early_stop)
    r32 = search(make_fn(np.float32), B, beam, maxlen, sos, eos, np.float32, early_stop)
    same = r64["steps"] == r32["steps"] and np.array_equal(r64["hyp"], r32["hyp"]) and np.array_equal(r64["anc"], r32["anc"])
    E = float("inf")
    if same:
        E = 0.0
        for a, b in zip(r32["kept"], r64["kept"]):
            fin = np.isfinite(b)
            E = max(E, float(np.abs(a[fin].astype(np.float64) - b[fin]).max()) if fin.any() else 0.0)
    return r64, r64["delta"], E, same


def usable(delta, E, factor=100.0):
    return delta >= factor * max(E, 1e-6)


def pos_row(p, d, dtype):
    """PositionalEncoding.pe[p] (embedding.py:34-46): the table is built in fp32 by the reference."""
    pos = torch.tensor([[float(p)]], dtype=torch.float32)
    div = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe = torch.zeros(d, dtype=torch.float32)
    pe[0::2], pe[1::2] = torch.sin(pos * div)[0], torch.cos(pos * div)[0]
    return pe.to(dtype)


class CachedDecoder:
    """forward_one_step for R = B * beam rows with per-layer key / value caches [R, maxlen, D]: ``w`` = state dict (numpy or
    torch), ``pre`` = "decoder." / "decoder.left_decoder.", memory [B, T, D], mem_len [B] or None.  ``logits(p, hyp, anc)``
    feeds hyp[:, p] at position p; ``__call__`` returns its log-softmax as NumPy in the search's precision."""

    def __init__(self, w, pre, memory, mem_len, heads, beam, maxlen, dtype=torch.float64, reorder=False):
        self.dt, self.pre, self.H, self.reorder = dtype, pre, heads, reorder
        g = lambda k: (w[k] if torch.is_tensor(w[k]) else torch.from_numpy(np.asarray(w[k]))).to(dtype)     # noqa: E731
        self.g = g
        memory = torch.as_tensor(memory).to(dtype)
        B, T, D = memory.shape
        self.D, self.R = D, B * beam
        self.memory = memory.repeat_interleave(beam, 0)                                                     # [R, T, D]
        lens = torch.full((B,), T) if mem_len is None else torch.as_tensor(mem_len).long()
        self.hide = ~(torch.arange(T)[None, :] < lens.repeat_interleave(beam)[:, None])                     # [R, T]
        self.n = 0
        while f"{pre}decoders.{self.n}.norm1.weight" in w:
            self.n += 1
        self.kc = torch.zeros(self.n, self.R, maxlen, D, dtype=dtype)
        self.vc = torch.zeros(self.n, self.R, maxlen, D, dtype=dtype)
        self.mem_kv = []
        for i in range(self.n):
            a = f"{pre}decoders.{i}.src_attn."
            self.mem_kv.append((F.linear(self.memory, g(a + "linear_k.weight"), g(a + "linear_k.bias")),
                                F.linear(self.memory, g(a + "linear_v.weight"), g(a + "linear_v.bias"))))

    def _attend(self, q, k, v, hide=None):
        """q [R, D], k / v [R, n, D] -> [R, D]"""
        R, n, D = k.shape
        dk = D // self.H
        q, k, v = q.view(R, self.H, 1, dk), k.view(R, n, self.H, dk).transpose(1, 2), v.view(R, n, self.H, dk).transpose(1, 2)
        s = (q @ k.transpose(-2, -1)) / math.sqrt(dk)                                                       # [R, H, 1, n]
        if hide is not None:
            s = s.masked_fill(hide[:, None, None, :], -float("inf"))
        a = torch.softmax(s, -1)
        if hide is not None:
            a = a.masked_fill(hide[:, None, None, :], 0.0)
        return (a @ v).transpose(1, 2).reshape(R, D)

    def logits(self, p, hyp, anc):
        g, pre, D = self.g, self.pre, self.D
        lin = lambda a, n, x: F.linear(x, g(a + f"linear_{n}.weight"), g(a + f"linear_{n}.bias"))          # noqa: E731
        ln = lambda n, x: F.layer_norm(x, (D,), g(n + ".weight"), g(n + ".bias"), 1e-5)                      # noqa: E731
        tok = torch.as_tensor(np.asarray(hyp)[:, p]).long()
        x = g(pre + "embed.0.weight")[tok] * math.sqrt(D) + pos_row(p, D, self.dt)
        rows = torch.arange(self.R)
        src = torch.as_tensor(np.asarray(anc)[:, :p]).long()                                                # [R, p]
        for i in range(self.n):
            a = f"{pre}decoders.{i}."
            h = ln(a + "norm1", x)
            self.kc[i, :, p], self.vc[i, :, p] = lin(a + "self_attn.", "k", h), lin(a + "self_attn.", "v", h)
            take = src if (i == 0 or self.reorder) else rows[:, None].expand(-1, p)
            take = torch.cat((take, rows[:, None]), 1)                                                      # [R, p + 1]
            pos = torch.arange(p + 1)[None, :]
            x = x + lin(a + "self_attn.", "out", self._attend(lin(a + "self_attn.", "q", h), self.kc[i][take, pos],
                                                              self.vc[i][take, pos]))
            h = ln(a + "norm2", x)
            x = x + lin(a + "src_attn.", "out", self._attend(lin(a + "src_attn.", "q", h), *self.mem_kv[i], hide=self.hide))
            h = ln(a + "norm3", x)
            x = x + F.linear(torch.relu(F.linear(h, g(a + "feed_forward.w_1.weight"), g(a + "feed_forward.w_1.bias"))),
                             g(a + "feed_forward.w_2.weight"), g(a + "feed_forward.w_2.bias"))
        x = ln(pre + "after_norm", x)
        return F.linear(x, g(pre + "output_layer.weight"), g(pre + "output_layer.bias"))

    def __call__(self, p, hyp, anc):
        return torch.log_softmax(self.logits(p, hyp, anc), -1).numpy()


def model_fn(w, pre, memory, mem_len, heads, beam, maxlen, reorder=False):
    """``make_fn`` of ``margin`` for a model case."""
    to = {np.float64: torch.float64, np.float32: torch.float32}
    return lambda dtype: CachedDecoder(w, pre, memory, mem_len, heads, beam, maxlen, to[dtype], reorder)
