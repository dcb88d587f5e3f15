"""Whisper's beam search on the GPU (f5e_whisper_beam_step in csrc/whisper.hip, the loop in eval/whisper.py) against
  * ``beam_step_ref`` (tests/whisper_beam_ref.py, float64), one step at a time on constructed logits: chosen rows, classes, tables,
    pool and flags exactly, scores within 1e-4 absolute;
  * the fixture made from ``transformers``' ``generate(num_beams=5)`` (tests/golden/whisper_beam.npz): all K pool sequences and
    lengths equal, scores within 1e-4;
  * its own B = 1 runs, bit for bit, for a ragged batch; and teacher forcing for the ancestry.

The score bound.  A candidate is score + (x - max) - log(sum exp(x - max)) in fp32.  The sum is a per-thread sequential sum of
V / 256 terms, a wave tree, four partial sums per chunk and the chunks in order: about 5e-5 relative on the normaliser at
V = 51866 with the per-lane figure of V / 64 terms, i.e. 5e-5 absolute on its logarithm; the other roundings are a few 2^-24 of
values below 300.  1e-4 absolute covers it.  The fixture's gaps are at least 1e-3 nats (asserted by its generator), the
constructed logits' at least 1e-2 (asserted here from the reference's own figure), so no order can flip within the bound.

Constructed logits: every row gets 2K + 2 "peak" classes whose CANDIDATE values are dealt from one descending ladder with steps of
0.5 (so the utterance's ranking is known by design and every gap is 0.5), the other classes lie 30 or more below.  The suppressed
classes are the largest logits of every row and one of them is the sink that brings the row's logsumexp to one common value, so a
normaliser without them, or a pick that ignores the list, cannot pass.

Every test prints its measured error before it asserts."""
import numpy as np
import pytest
import torch

import whisper_beam_ref as BR
from test_whisper_beam_cpu import case, gold, tiny_model

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
SCORE_TOL, GAP = 1e-4, 1e-2
CANARY_I, CANARY_F = -77, -123.25
CHUNK = 8192


def _ops():
    from f5e_tts_amd import ops
    return ops


# ---- one step: construction, run, comparison ------------------------------------------------------------------------------------

def build(seed, B, K, V, *, p=6, n0=3, cap=40, ld=44, eos=None, eos_rank=None, pool=None, open_=None, dead=(), n_sup=3, n_beg=0):
    """-> (logits f64 [B K][V], state, kwargs of the step).  ``eos_rank[b]``: the rank (0-based, in the utterance) at which eos
    stands among the candidates (None: far below).  ``pool[b]``: the normalised scores of the entries the pool already holds.
    ``dead``: local rows with score -inf.  Candidate of rank j = -14 - j / 2 (every row's logsumexp is LSE; the first suppressed
    class is the sink that makes it so).  Without a suppressed class (n_sup + n_beg = 0) every row is shifted to logsumexp 0
    instead and the ranking is the reference's, not the ladder's."""
    rng = np.random.default_rng(seed)
    R_, LSE = B * K, 50.0
    eos = V - 1 if eos is None else eos
    n_ban = n_sup + n_beg
    T = min(2 * K + 2, V - 1 - n_ban)                               # peaks per row (eos and the suppressed classes apart)
    st = BR.new_state(B, K, ld, list(range(1, n0 + 1)), eos)
    st["hyp"][:, :p + 1] = rng.integers(0, V, (R_, p + 1))
    st["hyp"][:, p + 1:] = CANARY_I
    st["anc"][:, :p] = (np.arange(R_) // K * K)[:, None] + rng.integers(0, K, (R_, p))
    st["anc"][:, p:] = CANARY_I
    st["score"] = -rng.uniform(1.0, 9.0, R_)
    for b in range(B):
        for q in dead:
            st["score"][b * K + q] = -np.inf
    if p + 1 == n0:                                                # the first pick: only row 0 of an utterance is live
        st["score"] = np.where(np.arange(R_) % K == 0, 0.0, -np.inf)
    pool = pool or [[] for _ in range(B)]
    for b in range(B):
        for s, sc in enumerate(pool[b]):
            ln = int(rng.integers(n0 + 1, p + 2))
            st["pool_score"][b, s], st["pool_len"][b, s] = sc, ln
            st["pool_hyp"][b, s, :ln] = rng.integers(0, V, ln)
            st["pool_hyp"][b, s, ln:] = CANARY_I
        st["pool_hyp"][b, len(pool[b]):] = CANARY_I
        st["pool_score"][b, len(pool[b]):] = CANARY_F
        st["pool_len"][b, len(pool[b]):] = CANARY_I
        st["pool_n"][b] = len(pool[b])
    if open_ is not None:
        st["open"][:] = open_
    forced = [c for c in (0, CHUNK - 1, CHUNK, V - 2) if 0 <= c < V and c != eos][:T]    # peaks at the chunks' edges
    banned = [int(c) for c in rng.permutation(V) if c != eos and c not in forced][:n_ban]
    suppress, begin = banned[:n_sup], banned[n_sup:]
    c = rng.normal(0.0, 1.0, (R_, V)) - 60.0                        # candidate values; logits = c - score + LSE
    c[:, eos] = -45.0
    for b in range(B):
        live = [q for q in range(K) if st["score"][b * K + q] > -np.inf]
        ladder = -14.0 - 0.5 * np.arange(len(live) * T)
        deal = rng.permutation(len(live) * T)
        classes = []
        for i, q in enumerate(live):
            free = [int(k) for k in rng.permutation(V) if k != eos and k not in banned and k not in forced]
            classes.append((forced + free)[:T])
            c[b * K + q, classes[i]] = ladder[deal[i * T:(i + 1) * T]]
        if eos_rank is not None and eos_rank[b] is not None:
            slot = int(np.where(deal == eos_rank[b])[0][0])
            r = b * K + live[slot // T]
            c[r, eos], c[r, classes[slot // T][slot % T]] = c[r, classes[slot // T][slot % T]], -55.0
    x = c + LSE - np.where(np.isfinite(st["score"]), st["score"], 0.0)[:, None]
    if n_ban:
        x[:, banned[1:]] = LSE - 3.0 - 0.5 * np.arange(n_ban - 1)
        x[:, banned[0]] = -np.inf
        rest = x.max(1) + np.log(np.exp(x - x.max(1, keepdims=True)).sum(1))
        assert (rest < LSE - 0.5).all()
        x[:, banned[0]] = LSE + np.log1p(-np.exp(rest - LSE))       # the sink: the row's largest logit, and suppressed
    else:
        x -= (x.max(1, keepdims=True) + np.log(np.exp(x - x.max(1, keepdims=True)).sum(1, keepdims=True)))
    return x, st, dict(p=p, n0=n0, cap=cap, eos=eos, K=K, suppress=suppress + [-3, V + 5], begin_suppress=begin)


def run_step(x, st, kw, ld_logits=None, pad=64):
    """Runs the device step on copies of ``st`` under canaries and checks that the inputs and the scratch beyond the queried
    size are untouched -> the state after the step."""
    ops = _ops()
    dev = torch.device("cuda")
    R_, V = x.shape
    K, B = kw["K"], R_ // kw["K"]
    ldl = ld_logits or (V + 3) // 4 * 4
    big = torch.full((R_, ldl), 7.5, dtype=F32, device=dev)
    big[:, :V] = torch.from_numpy(x).to(dev, F32)
    logits = big[:, :V]
    t = lambda a, d: torch.from_numpy(np.ascontiguousarray(a)).to(dev, d)   # noqa: E731
    score, last = t(st["score"], F32), torch.full((R_,), CANARY_I, dtype=I32, device=dev)
    hyp_in, anc_in = t(st["hyp"], I32), t(st["anc"], I32)
    hyp_out, anc_out = torch.full_like(hyp_in, CANARY_I), torch.full_like(anc_in, CANARY_I)
    pool_hyp, pool_len, pool_score = t(st["pool_hyp"], I32), t(st["pool_len"], I32), t(st["pool_score"], F32)
    pool_n, open_, alive = t(st["pool_n"], I32), t(st["open"], I32), torch.full((B,), CANARY_I, dtype=I32, device=dev)
    need = ops.whisper_beam_scratch(B, K, V)
    scratch = torch.full((need + pad,), 0xA5, dtype=torch.uint8, device=dev)
    sup = t(np.array(kw["suppress"], np.int32), I32) if kw["suppress"] else None
    beg = t(np.array(kw["begin_suppress"], np.int32), I32) if kw["begin_suppress"] else None
    big0, hyp0, anc0 = big.clone(), hyp_in.clone(), anc_in.clone()
    ops.whisper_beam_step(logits, score, hyp_in, anc_in, hyp_out, anc_out, last, pool_hyp, pool_len, pool_score, pool_n, open_,
                          alive, kw["p"], kw["n0"], kw["cap"], kw["eos"], K, suppress=sup, begin_suppress=beg,
                          length_penalty=kw.get("length_penalty", 1.0), scratch=scratch[:need])
    torch.cuda.synchronize()
    assert torch.equal(big, big0) and torch.equal(hyp_in, hyp0) and torch.equal(anc_in, anc0)      # inputs are only read
    assert (scratch[need:] == 0xA5).all()                                                           # scratch beyond the queried size
    n = lambda a: a.cpu().numpy()   # noqa: E731
    return dict(score=n(score), hyp=n(hyp_out), anc=n(anc_out), last=n(last), pool_hyp=n(pool_hyp), pool_len=n(pool_len),
                pool_score=n(pool_score), pool_n=n(pool_n), open=n(open_), alive=n(alive))


def compare(got, want, st, kw, what):
    p, K = kw["p"], kw["K"]
    B = len(want["pool_n"])
    fin = np.isfinite(want["score"])
    err = float(np.abs(got["score"][fin] - want["score"][fin]).max()) if fin.any() else 0.0
    perr = 0.0
    assert (got["hyp"][:, :p + 2] == want["hyp"][:, :p + 2]).all(), what
    assert (got["anc"][:, :p + 1] == want["anc"][:, :p + 1]).all(), what
    assert (got["hyp"][:, p + 2:] == CANARY_I).all() and (got["anc"][:, p + 1:] == CANARY_I).all(), what   # containment
    assert (got["last"] == want["last"]).all() and (np.isfinite(got["score"]) == fin).all(), what
    assert (got["score"][~fin] == -np.inf).all(), what
    for k in ("pool_n", "open", "alive"):
        assert (got[k] == want[k]).all(), (what, k, got[k], want[k])
    for b in range(B):
        n = int(want["pool_n"][b])
        assert (got["pool_len"][b, :n] == want["pool_len"][b, :n]).all(), what
        perr = max([perr] + [abs(float(got["pool_score"][b, s]) - want["pool_score"][b, s]) for s in range(n)])
        for s in range(K):
            if s < n:
                ln = int(want["pool_len"][b, s])
                assert (got["pool_hyp"][b, s, :ln] == want["pool_hyp"][b, s, :ln]).all(), (what, b, s)
            same = s < st["pool_n"][b] and s < n and want["pool_score"][b, s] == st["pool_score"][b, s] \
                and want["pool_len"][b, s] == st["pool_len"][b, s]
            if s >= n or same:                                      # a slot that does not change is not written at all
                assert (got["pool_hyp"][b, s] == st["pool_hyp"][b, s]).all(), (what, b, s)
                assert got["pool_score"][b, s] == np.float32(st["pool_score"][b, s]) and got["pool_len"][b, s] == st["pool_len"][b, s]
    print(f"{what}: score error {err:.2e}, pool score error {perr:.2e} (bound {SCORE_TOL:g})")
    assert err < SCORE_TOL and perr < SCORE_TOL, what


def check(seed, B, K, V, ld_logits=None, **knobs):
    x, st, kw = build(seed, B, K, V, **knobs)
    want, gap = BR.beam_step_ref(x.astype(np.float32), st, kw["p"], kw["n0"], kw["cap"], kw["eos"], K, kw["suppress"],
                                 kw["begin_suppress"])
    assert gap >= GAP, f"the constructed case has a gap of {gap:.2e}"
    got = run_step(x, st, kw, ld_logits)
    compare(got, want, st, kw, f"B={B} K={K} V={V} {knobs}")
    return got, want, st


SHAPES = ((10, 12), (63, 64), (64, 64), (65, 68), (CHUNK - 1, CHUNK), (CHUNK, CHUNK), (CHUNK + 1, CHUNK + 4), (51866, 51868))


GRID = [(V, ld, K, B) for V, ld in SHAPES for K in (1, 2, 5, 16) for B in (1, 3) if 2 * K <= V]     # 2 K <= V is the kernel's limit


@pytest.mark.parametrize("V,ld,K,B", GRID)
def test_step_matches_the_reference(V, ld, K, B):
    if V == 2 * K:                                                  # every class is a candidate: no room for a suppressed one
        check(V + K, B, K, V, ld, n_sup=0, pool=[[-2.0]] * B, dead=(K - 1,))
        return
    got, want, _ = check(V + K, B, K, V, ld, eos_rank=[min(1, K - 1)] + [None] * (B - 1), pool=[[-2.0, -5.0][:K]] * B,
                         dead=(K - 1,) if K > 2 else ())
    assert want["pool_n"][0] == min(K, 3)                           # eos inside the first K entered the pool (K > 1)


def test_unaligned_rows_take_the_scalar_loads():
    check(5, 2, 5, 777, 779)


def test_more_survivors_than_the_lds_holds():
    """K * chunks * 2K > 4096: the selection runs on the scratch records themselves."""
    check(6, 1, 16, 9 * CHUNK + 5, eos_rank=[3], pool=[[-0.5]])


def test_first_step_with_begin_suppress():
    got, want, _ = check(11, 3, 5, 300, p=3, n0=4, n_beg=2)
    assert (want["anc"][:, 3].reshape(3, 5) == np.arange(3)[:, None] * 5).all()      # every new row descends from row 0
    x, st, kw = build(11, 3, 5, 300, p=4, n0=4, n_beg=2)                                # one step later the list is off
    want2, gap = BR.beam_step_ref(x.astype(np.float32), st, 4, 4, kw["cap"], kw["eos"], 5, kw["suppress"], [])
    assert gap >= GAP and all(c in want2["last"] for c in kw["begin_suppress"])         # ... and its classes are picked
    compare(run_step(x, st, kw), want2, st, kw, "begin_suppress after the first step")


def test_eos_inside_and_outside_the_first_k():
    _, want, st = check(12, 2, 5, 300, eos_rank=[2, 7], pool=[[-2.0], [-2.0]])
    assert want["pool_n"].tolist() == [2, 1]                       # rank 2 enters; rank 7 (K .. 2K-1) neither runs nor enters
    assert 299 not in want["last"][5:].tolist() and 299 not in want["last"][:5].tolist()


def test_full_pool_replaces_its_worst_entry_and_rule_six_closes():
    # p + 2 - n0 = 5: the eos candidate at rank 0 has value -14, normalised -2.8; the best open row then has -14.5 / 5 = -2.9
    _, want, st = check(13, 1, 5, 300, eos_rank=[0], pool=[[-1.0, -2.0, -2.5, -3.0, -4.0]])
    assert want["pool_len"][0, 3] == 8 and want["pool_score"][0, 4] == st["pool_score"][0, 3] and want["open"][0] == 1
    # a worst entry of -2.8 after the replacement: the best open row cannot beat it: closed
    _, want, st = check(13, 1, 5, 300, eos_rank=[0], pool=[[-1.0, -2.0, -2.5, -2.6, -2.85]])
    assert want["pool_len"][0, 4] == 8 and want["open"][0] == 0 and want["alive"][0] == 0
    # a newcomer worse than a full pool's worst entry is dropped
    _, want, st = check(13, 1, 5, 300, eos_rank=[0], pool=[[-1.0, -1.5, -2.0, -2.5, -2.7]])
    assert (want["pool_score"][0] == st["pool_score"][0]).all() and 8 not in want["pool_len"][0] and want["open"][0] == 0


def test_cap_step_hits_everything():
    _, want, _ = check(14, 2, 5, 300, p=6, cap=8, ld=8, pool=[[-1.0], []])
    assert want["pool_n"].tolist() == [5, 5] and want["alive"].tolist() == [0, 0] and not np.isfinite(want["score"]).any()
    assert (want["pool_len"][1] == 8).all()


def test_closed_utterance_beside_an_open_one_keeps_its_pool():
    got, want, st = check(15, 3, 5, 300, eos_rank=[0, 0, 0], pool=[[-1.0, -2.0]] * 3, open_=[1, 0, 1])
    assert want["pool_n"].tolist() == [3, 2, 3] and want["alive"].tolist() == [1, 0, 1]
    assert (got["pool_hyp"][1] == st["pool_hyp"][1]).all() and (got["pool_len"][1] == st["pool_len"][1]).all()
    assert got["pool_score"][1].tobytes() == st["pool_score"][1].astype(np.float32).tobytes()      # bit-identical
    assert np.isfinite(got["score"][5:10]).all()                   # ... while its rows keep running


def test_rows_at_minus_infinity():
    _, want, _ = check(16, 2, 5, 300, dead=(0, 2, 3))
    assert np.isfinite(want["score"]).all()                        # 2 live rows x 12 peaks still fill the beam
    _, want, _ = check(16, 1, 5, 11, dead=(0, 1, 2, 3), n_sup=0, eos_rank=[0])
    assert np.isfinite(want["score"]).sum() == 5


def test_the_rows_maximum_is_a_suppressed_class():
    """build() makes a suppressed class the largest of every row: the normaliser of rule 1 includes it.  Here the reference
    WITHOUT the suppressed classes in the normaliser is shown to differ by far more than the bound, so the parity does test it."""
    x, st, kw = build(17, 1, 5, 300)
    assert all(int(np.argmax(x[r])) in kw["suppress"] for r in range(5))
    want, _ = BR.beam_step_ref(x.astype(np.float32), st, kw["p"], kw["n0"], kw["cap"], kw["eos"], 5, kw["suppress"], [])
    y = x.copy()
    y[:, [c for c in kw["suppress"] if 0 <= c < 300]] = -np.inf
    wrong, _ = BR.beam_step_ref(y, st, kw["p"], kw["n0"], kw["cap"], kw["eos"], 5)
    assert np.abs(wrong["score"] - want["score"]).min() > 3.0
    compare(run_step(x, st, kw), want, st, kw, "suppressed maximum")


def test_length_penalty():
    x, st, kw = build(18, 1, 5, 300, eos_rank=[0], pool=[[-0.3]])
    kw["length_penalty"] = 2.0
    want, gap = BR.beam_step_ref(x.astype(np.float32), st, kw["p"], kw["n0"], kw["cap"], kw["eos"], 5, kw["suppress"], [], 2.0)
    assert gap >= GAP and want["pool_score"][0, 1] == pytest.approx(-14.0 / 25.0, abs=1e-5)
    compare(run_step(x, st, kw), want, st, kw, "length_penalty 2")


def test_refusals():
    from f5e_tts_amd import _C
    ops = _ops()
    dev = torch.device("cuda")

    def call(K=5, V=64, p=6, n0=3, cap=40, ld=44, eos=63, R_=5, B=1, same=False, scratch_cut=0, cols=64):
        logits = torch.zeros(R_, cols, device=dev)
        hyp, anc = (torch.zeros(R_, ld, dtype=I32, device=dev) for _ in range(2))
        hyp2, anc2 = (hyp, anc) if same else (torch.zeros_like(hyp), torch.zeros_like(anc))
        need = ops.whisper_beam_scratch(1, 5, 64)
        ops.whisper_beam_step(logits, torch.zeros(R_, device=dev), hyp, anc, hyp2, anc2, torch.zeros(R_, dtype=I32, device=dev),
                              torch.zeros(B, K, ld, dtype=I32, device=dev), torch.zeros(B, K, dtype=I32, device=dev),
                              torch.zeros(B, K, device=dev), *(torch.zeros(B, dtype=I32, device=dev) for _ in range(3)),
                              p, n0, cap, eos, K, V=V, scratch=torch.zeros(need - scratch_cut, dtype=torch.uint8, device=dev))
    call()                                                          # the base call is accepted
    bad = dict(K0=dict(K=0, R_=5), K17=dict(K=17, R_=17, cols=64), V_below_2K=dict(V=9), V_above_columns=dict(V=65),
               eos_negative=dict(eos=-1), eos_V=dict(eos=64), n0_zero=dict(n0=0), p_below_prompt=dict(p=1, n0=3),
               ld_below_p2=dict(p=43), cap_above_ld=dict(cap=45), same_tables=dict(same=True), short_scratch=dict(scratch_cut=4),
               rows_not_B_K=dict(R_=7))
    for name, over in bad.items():
        with pytest.raises(_C.F5EError):
            call(**over)
            pytest.fail(name)
    for args in ((0, 5, 64), (65536, 5, 64), (1, 0, 64), (1, 17, 64), (1, 5, 9), (1, 5, 262145)):
        with pytest.raises(_C.F5EError):
            ops.whisper_beam_scratch(*args)
    assert ops.whisper_beam_scratch(2, 5, CHUNK + 1) == 2 * 5 * 2 * (2 + 20) * 4
    torch.cuda.synchronize()


# ---- the search against the fixture --------------------------------------------------------------------------------------------

_dev = {}


def model_gpu(i):
    if ("m", i) not in _dev:
        _dev[("m", i)] = tiny_model(i).cuda()
    return _dev[("m", i)]


def kv_gpu(i):
    if ("kv", i) not in _dev:
        _dev[("kv", i)] = model_gpu(i).cross_kv(torch.from_numpy(case(i)["enc"].copy()).cuda()[None])
    return _dev[("kv", i)]


def search(i, sync_every=8):
    fx, c = gold(), case(i)
    return model_gpu(i).generate_from_kv(kv_gpu(i), fx["prompt"].tolist(), max_new_tokens=c["cap"] - len(fx["prompt"]),
                                         sync_every=sync_every, beam_size=int(fx["K"]), return_beams=True)


@pytest.mark.parametrize("i", range(3))
def test_search_equals_the_fixture_whatever_sync_every(i):
    c = case(i)
    tokens, n, (beams, lens, scores) = search(i, 1)
    tokens8, n8, (beams8, lens8, scores8) = search(i, 8)
    err = float(np.abs(scores[0].cpu().numpy().astype(np.float64) - c["scores"]).max())
    print(f"case {i} ({c['tags']}): lens {lens[0].tolist()}, score error {err:.2e} (bound {SCORE_TOL:g})")
    assert lens[0].tolist() == c["lens"].tolist() and (beams[0].cpu().numpy() == c["tokens"]).all()
    assert err < SCORE_TOL
    assert torch.equal(tokens[0], beams[0, 0]) and int(n[0]) == int(lens[0, 0]) and tokens.shape == (1, c["cap"])
    assert torch.equal(beams, beams8) and torch.equal(lens, lens8) and torch.equal(scores, scores8) and torch.equal(tokens, tokens8)


def test_beam_size_one_still_returns_the_greedy_fixture():
    import test_whisper_gpu as TG
    fx = TG.gold()
    for name, eos_case in (("14400", False), ("eos", True)):
        tokens, cnt = TG.model_gpu(eos_case).generate_from_kv(TG.kv_gpu(14400, eos_case), fx["prompt"].tolist(), beam_size=1)
        assert tokens[0, :int(cnt[0])].tolist() == fx[f"tokens_{name}"].tolist()


def test_ragged_batch_equals_its_own_single_runs_bit_for_bit():
    """Two utterances of different lengths in one B = 2 call, garbage beyond ``len``, against their own B = 1 runs: tokens and
    scores bit for bit (the greedy fixture's full model, from audio)."""
    import test_whisper_gpu as TG
    fx, model = TG.gold(), TG.model_gpu()
    lens = (40000, 14400)
    wav = torch.full((2, 48000), 0.37, device="cuda")
    for b, n in enumerate(lens):
        wav[b, :n] = torch.from_numpy(fx["wave_f32"][:n].copy()).cuda()
    out = model.generate(wav, list(lens), "english", max_new_tokens=16, beam_size=5, return_beams=True)
    for b, n in enumerate(lens):
        one = model.generate(TG.wave_gpu(n), None, "english", max_new_tokens=16, beam_size=5, return_beams=True)
        assert torch.equal(out[0][b], one[0][0]) and int(out[1][b]) == int(one[1][0])
        for k in range(3):
            assert torch.equal(out[2][k][b], one[2][k][0]), (b, k)
    assert not torch.equal(out[0][0], out[0][1])


@pytest.mark.parametrize("i", range(3))
def test_ancestry_by_teacher_forcing(i):
    """No reference: the returned hypotheses go through ``decoder_logits`` (no ancestry table, a fresh cache per row) and the sum
    of their tokens' log-probabilities must equal score x generated length within 1e-4 per token.  A wrong ancestry column,
    or a cache row that moved, shows here."""
    fx = gold()
    g = fx["generation_config"]
    n0 = len(fx["prompt"])
    _, _, (beams, lens, scores) = search(i)
    K = beams.shape[1]
    kvK = [(k.expand(K, -1, -1).contiguous(), v.expand(K, -1, -1).contiguous()) for k, v in kv_gpu(i)]
    logp = torch.log_softmax(model_gpu(i).decoder_logits(kvK, beams[0]).double(), -1).cpu().numpy()
    worst = 0.0
    for s in range(K):
        ln, ids = int(lens[0, s]), beams[0, s].tolist()
        total = sum(logp[s, u - 1, ids[u]] for u in range(n0, ln))
        assert not any(ids[u] in g["suppress_tokens"] for u in range(n0, ln)) and ids[n0] not in g["begin_suppress_tokens"]
        worst = max(worst, abs(total - float(scores[0, s]) * (ln - n0)) / (ln - n0))
    print(f"case {i}: worst |teacher-forced sum - score x length| per token {worst:.2e} (bound {SCORE_TOL:g})")
    assert worst < SCORE_TOL
