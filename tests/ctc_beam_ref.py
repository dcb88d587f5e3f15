"""NumPy restatement of the CTC prefix beam search of csrc/ctc_beam.hip (include/f5e_abi.h: f5e_ctc_beam): the reference's loop
(ppg/asr_model.py:461-546) with a dict per frame, in fp64 or, with ``dtype=np.float32``, in fp32.  Pinned against the
reference's own ``_ctc_prefix_beam_search`` by tests/golden/ctc_beam.npz (tests/golden/make_ctc_beam_golden.py).

The margin rule.  Which prefixes survive a frame depends on the order of the candidates' totals, so two implementations that
differ in rounding agree on the lists only where no decisive pair of totals is close.  ``search`` reports ``delta``: at every
frame the candidates' totals are sorted descending, the first min(n, K + 1) are kept (the survivors and the best loser), and
delta is the smallest gap between neighbours among them over all frames.  A case is usable for exact list equality iff
delta >= 20 * max(E, 1e-6), E being the largest score difference between this file's fp32 and fp64 runs (``margin``)."""
import numpy as np


def normalise(scores, dtype=np.float64):
    """x - logsumexp(x) per frame, in ``dtype``: raw logits and log-probabilities give the same numbers."""
    x = np.asarray(scores).astype(dtype)
    m = x.max(-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True))


def _log_add(dtype, *args):
    if all(a == -np.inf for a in args):
        return dtype(-np.inf)
    a_max = max(args)
    return dtype(a_max + np.log(sum(np.exp(dtype(a - a_max)) for a in args), dtype=dtype))


def search(scores, beam, blank=0, dtype=np.float64, normalised=False):
    """scores [T, V] (logits or log-probabilities) -> (hyps: list of (tuple ids, score) best first, delta).  T = 0 gives the
    empty prefix with score 0.  ``normalised``: take the scores as log-probabilities as they are (the reference's arithmetic
    on its own fp32 log_softmax) instead of normalising every frame again, as the kernel does."""
    f = dtype
    if not len(scores):
        logp = np.zeros((0, 1), f)
    else:
        logp = np.asarray(scores).astype(f) if normalised else normalise(scores, f)
    ninf = f(-np.inf)
    cur = [(tuple(), (f(0.0), ninf))]
    delta = np.inf
    for t in range(logp.shape[0]):
        row = logp[t]
        top = np.argsort(-row, kind="stable")[:beam]         # value descending, the lower class first among equal values
        nxt = {}
        for s in top:
            s, ps = int(s), row[s]
            for prefix, (pb, pnb) in cur:
                last = prefix[-1] if prefix else None
                if s == blank:
                    n_pb, n_pnb = nxt.get(prefix, (ninf, ninf))
                    nxt[prefix] = (_log_add(f, n_pb, f(pb + ps), f(pnb + ps)), n_pnb)
                elif s == last:
                    n_pb, n_pnb = nxt.get(prefix, (ninf, ninf))
                    nxt[prefix] = (n_pb, _log_add(f, n_pnb, f(pnb + ps)))
                    n_prefix = prefix + (s,)
                    n_pb, n_pnb = nxt.get(n_prefix, (ninf, ninf))
                    nxt[n_prefix] = (n_pb, _log_add(f, n_pnb, f(pb + ps)))
                else:
                    n_prefix = prefix + (s,)
                    n_pb, n_pnb = nxt.get(n_prefix, (ninf, ninf))
                    nxt[n_prefix] = (n_pb, _log_add(f, n_pnb, f(pb + ps), f(pnb + ps)))
        ranked = sorted(nxt.items(), key=lambda kv: _log_add(f, *kv[1]), reverse=True)
        totals = np.array([_log_add(f, *v) for _, v in ranked[:beam + 1]], np.float64)
        if len(totals) > 1:
            with np.errstate(invalid="ignore"):
                gaps = -np.diff(totals)
            delta = min(delta, float(np.nan_to_num(gaps, nan=0.0).min()))
        cur = ranked[:beam]
    return [(p, float(_log_add(f, *v))) for p, v in cur], float(delta)


def margin(scores, beam, blank=0, normalised=False):
    """(hyps of the fp64 run, delta, E, same): E = the largest |score_fp32 - score_fp64| over the final list, ``same`` = the
    fp32 run gives the same list."""
    h64, delta = search(scores, beam, blank, np.float64, normalised)
    h32, _ = search(scores, beam, blank, np.float32, normalised)
    same = [p for p, _ in h32] == [p for p, _ in h64]
    E = max((abs(a[1] - b[1]) for a, b in zip(h32, h64)), default=0.0) if same else float("inf")
    return h64, delta, E, same


def usable(delta, E, factor=20.0):
    return delta >= factor * max(E, 1e-6)


def pack(hyps, beam, ld_hyp):
    """The kernel's output layout for one sequence: hyp i32 [beam, ld_hyp] (-1 padded, cut at ld_hyp), hyp_len, score."""
    hyp = np.full((beam, ld_hyp), -1, np.int32)
    n = np.full(beam, -1, np.int32)
    sc = np.full(beam, -np.inf, np.float64)
    for i, (p, s) in enumerate(hyps):
        hyp[i, :min(len(p), ld_hyp)] = p[:ld_hyp]
        n[i], sc[i] = len(p), s
    return hyp, n, sc
