"""The resumable CTC prefix beam search (f5e_ctc_beam_state_init / f5e_ctc_beam_chunk through ops.ctc_beam_state and
ops.ctc_beam_chunk) against the whole-utterance search (ops.ctc_beam_search) on the same frames.

The property is exact: however T frames are cut into chunks (empty ones included), hyp / hyp_len / score after the last chunk
equal those of ONE ctc_beam_search call BIT FOR BIT -- a frame's first prune depends on that frame alone, the recurrence is the
same code doing the same fp32 operations in the same order, and trie nodes are numbered by the absolute frame.  So every
comparison with the one-call search is ``array_equal`` on the raw bits, and needs no margin rule; the comparisons with the
fp64 restatement (tests/ctc_beam_ref.py) and the reference's stored lists keep that file's rule and bound."""
import os

import numpy as np
import pytest
import torch

import ctc_beam_ref as BR
import test_ctc_beam_gpu as G

pytestmark = pytest.mark.gpu

GOLD = G.GOLD
I32, F32 = torch.int32, torch.float32
EDGE_IDS = [f"T{c[0]}-V{c[2]}-K{c[3]}-blank{c[6]}" for c in G.EDGE_CASES]


@pytest.fixture(scope="module")
def ops():
    import f5e_tts_amd.ops as ops_mod
    ops_mod.require_device()
    return ops_mod


def splits_of(T):
    """[T], all ones, sevens, sixteens (each with its remainder) and two empty chunks around a short one."""
    cut = lambda n: [n] * (T // n) + ([T % n] if T % n else [])   # noqa: E731
    return {"whole": [T], "ones": [1] * T, "sevens": cut(7), "sixteens": cut(16), "empties": [0, 3, 0, T - 3]}


def bits(got):
    return [np.ascontiguousarray(a).view(np.int32) for a in got]


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))


def host(out):
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def readout(ops, state, V, ld_hyp=None, blank=0):
    """A call that feeds nothing: the result so far, into sentinel-filled outputs."""
    B, K = state.B, state.beam
    ld_hyp = ld_hyp or state.T_cap
    hyp = torch.full((B, K, ld_hyp), -7, dtype=I32, device="cuda")
    n = torch.full((B, K), -7, dtype=I32, device="cuda")
    sc = torch.full((B, K), 123.0, dtype=F32, device="cuda")
    ops.ctc_beam_chunk(torch.zeros(B, 1, V, device="cuda"), torch.zeros(B, dtype=I32, device="cuda"), state, blank,
                       hyp=hyp, hyp_len=n, score=sc)
    return host((hyp, n, sc))


def feed(ops, state, scores_dev, t, n, blank=0, want=False):
    """Frames [t, t + n) of the single sequence ``scores_dev`` [T, V]; an empty chunk hands over one unread frame."""
    T = scores_dev.shape[0]
    lo = min(t, T - 1) if n == 0 else t
    part = scores_dev[lo:lo + max(n, 1)][None]
    return ops.ctc_beam_chunk(part, G.i32([n]), state, blank, want_result=want)


def run_chunks(ops, scores, splits, K, blank=0):
    """One sequence fed in ``splits``, read out with the LAST call only -> host arrays; T_cap = T, so ld_hyp = T as the
    one-call search's default."""
    T, V = scores.shape
    assert sum(splits) == T
    dev = torch.from_numpy(scores).cuda()
    before = dev.clone()
    state = ops.ctc_beam_state(1, T, max(max(splits), 1), K)
    t, out = 0, None
    for i, n in enumerate(splits):
        out = feed(ops, state, dev, t, n, blank, want=i == len(splits) - 1)
        t += n
    got = host(out)
    assert torch.equal(dev, before)
    return got


def one_call(ops, scores, K, blank=0, ld_hyp=None):
    return G.run_beam(ops, torch.from_numpy(scores)[None].cuda(), [scores.shape[0]], K, blank, ld_hyp)


# ------------------------------------------------------------------ every split, bit for bit

@pytest.mark.parametrize("case", G.EDGE_CASES, ids=EDGE_IDS)
def test_every_split_equals_one_call_bit_for_bit(ops, case):
    T, L, V, K, boost, seed, blank = case
    scores = G.planted_case(T, L, V, boost, seed, blank)
    want = one_call(ops, scores, K, blank)
    assert (want[1][0] >= 0).any()
    for name, splits in splits_of(T).items():
        got = run_chunks(ops, scores, splits, K, blank)
        assert same_bits(got, want), f"split {name}: the chunked search differs from the one-call search"


@pytest.mark.parametrize("case", G.EDGE_CASES, ids=EDGE_IDS)
def test_final_scores_equal_the_fp64_restatement_within_its_bound(ops, case):
    T, L, V, K, boost, seed, blank = case
    scores = G.planted_case(T, L, V, boost, seed, blank)
    hyps, E = G.restated(scores, K, blank)                       # asserts the margin rule on these very scores
    G.check_rows(run_chunks(ops, scores, splits_of(T)["sevens"], K, blank), 0, hyps, E, K, T, T)


# ------------------------------------------------------------------ beam 1 and the reference's stored lists

@pytest.mark.parametrize("case", G.EDGE_CASES, ids=EDGE_IDS)
def test_beam_one_every_split_equals_one_call(ops, case):
    T, L, V, _, boost, seed, blank = case
    scores = G.planted_case(T, L, V, boost, seed, blank)
    want = one_call(ops, scores, 1, blank)
    for name, splits in splits_of(T).items():
        assert same_bits(run_chunks(ops, scores, splits, 1, blank), want), f"beam 1, split {name}"


def test_stored_cases_in_chunks_of_sixteen_equal_one_call_and_the_reference_lists(ops):
    z = np.load(os.path.join(GOLD, "ctc_beam.npz"))
    seen = set()
    for i in range(int(z["n_cases"])):
        logp, K = z[f"logp_{i}"], int(z[f"beam_{i}"])
        T = len(logp)
        splits = splits_of(T)["sixteens"]
        got = run_chunks(ops, logp, splits, K)
        assert same_bits(got, one_call(ops, logp, K)), f"stored case {i} (T={T}, K={K})"
        hyp, n, _ = got
        ids, lens = z[f"ids_{i}"], z[f"len_{i}"]
        assert np.array_equal(n[0], lens) and np.array_equal(hyp[0][:, :ids.shape[1]], ids)
        assert (hyp[0][:, ids.shape[1]:] == -1).all()
        if T == 1100:                                            # the parent chains of re-created prefixes cross 68 chunk borders
            assert len(splits) == 69
            seen.add("T1100")
        seen |= {"K16"} if K == 16 else set()
        seen |= {"T1"} if T == 1 else set()
    assert seen == {"T1100", "K16", "T1"}


# ------------------------------------------------------------------ partial results

def test_partial_results_equal_the_search_on_the_frames_so_far_and_do_not_disturb_the_state(ops):
    T, L, V, K, boost, seed, blank = G.EDGE_CASES[2]
    scores = G.planted_case(T, L, V, boost, seed, blank)
    dev = torch.from_numpy(scores).cuda()
    state = ops.ctc_beam_state(1, T, 7, K)
    first = readout(ops, state, V)                               # before any frame: the empty prefix alone
    assert first[1][0].tolist() == [0] + [-1] * (K - 1) and first[2][0, 0] == 0.0 and (first[0] == -1).all()
    t = 0
    for n in splits_of(T)["sevens"]:
        got = host(feed(ops, state, dev, t, n, blank, want=True))
        t += n
        want = one_call(ops, scores[:t], K, blank, ld_hyp=T)
        assert same_bits(got, want), f"partial result after {t} frames"
        assert same_bits(readout(ops, state, V), want), f"second readout after {t} frames"
    assert t == T
    assert same_bits(got, run_chunks(ops, scores, splits_of(T)["sevens"], K, blank))     # no partials were read there


# ------------------------------------------------------------------ a batch advancing unevenly

def test_batch_with_different_frames_per_call_equals_each_sequence_alone(ops):
    V, K, C = 41, 10, 8
    seqs = [G.planted_case(40, 9, V, 8.0, 9501), G.planted_case(19, 4, V, 8.0, 9502), G.planted_case(33, 7, V, 8.0, 9503)]
    # per call the frames of (a, b, c): b ends early, c idles twice, a idles once
    plan = [(8, 8, 0), (8, 8, 5), (0, 3, 8), (8, 0, 0), (8, 0, 8), (8, 0, 8), (0, 0, 4)]
    assert [sum(p[i] for p in plan) for i in range(3)] == [len(s) for s in seqs]
    state = ops.ctc_beam_state(3, 40, C, K)
    solo = [ops.ctc_beam_state(1, 40, C, K) for _ in seqs]
    off = [0, 0, 0]
    rng = np.random.default_rng(9504)
    for call, ns in enumerate(plan):
        block = rng.standard_normal((3, C, V)).astype(np.float32)        # frames past n_frames[b] are noise nobody reads
        for b, n in enumerate(ns):
            block[b, :n] = seqs[b][off[b]:off[b] + n]
            off[b] += n
        block = torch.from_numpy(block).cuda()
        got = host(ops.ctc_beam_chunk(block, G.i32(ns), state))
        for b, n in enumerate(ns):
            alone = host(ops.ctc_beam_chunk(block[b:b + 1], G.i32([n]), solo[b]))
            assert same_bits([g[b] for g in got], [a[0] for a in alone]), f"call {call}, sequence {b}"
    for b, s in enumerate(seqs):
        want = one_call(ops, s, K, ld_hyp=40)
        assert same_bits([g[b] for g in got], [w[0] for w in want]), f"sequence {b} against the one-call search"


# ------------------------------------------------------------------ capacity, failures, containment

def dead(got, b):
    hyp, n, sc = got
    return bool((hyp[b] == -1).all() and (n[b] == -1).all() and (sc[b] == -np.inf).all())


def test_capacity_reached_works_one_frame_more_fails_for_good_and_nothing_else_is_touched(ops):
    V, K, C, T_cap = 41, 10, 8, 20
    a, b_, c = G.planted_case(20, 5, V, 8.0, 9601), G.planted_case(21, 5, V, 8.0, 9602), G.planted_case(18, 4, V, 8.0, 9603)
    need = ops.ctc_beam_state_bytes(3, T_cap, C, K)
    flat = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device="cuda")        # the state, then a guard zone
    state = ops.ctc_beam_state(3, T_cap, C, K, buf=flat[:need])
    assert state.nbytes == need
    off = 0
    for ns in ((8, 8, 8), (8, 8, 8), (4, 5, 2)):
        block = np.zeros((3, C, V), np.float32)
        for i, (s, n) in enumerate(zip((a, b_, c), ns)):
            block[i, :n] = s[off:off + n]
        off += 8
        got = host(ops.ctc_beam_chunk(torch.from_numpy(block).cuda(), G.i32(ns), state))
    assert dead(got, 1)                                                             # 21 frames into a state for 20
    for i, s in ((0, a), (2, c)):                                                   # T_cap reached exactly; a neighbour
        want = one_call(ops, s, K, ld_hyp=T_cap)
        assert same_bits([g[i] for g in got], [w[0] for w in want])
    again = readout(ops, state, V)                                                  # the next call: still dead, others intact
    assert dead(again, 1) and same_bits([g[[0, 2]] for g in again], [g[[0, 2]] for g in got])
    assert (flat[need:] == 0x5A).all()

    # n_frames below 0 and above T_chunk fail the sequence; the one between them goes on
    state = ops.ctc_beam_state(3, T_cap, C, K, buf=flat[:need])
    block = torch.from_numpy(np.stack([a[:4], c[:4], a[:4]])).cuda()
    got = host(ops.ctc_beam_chunk(block, G.i32([-1, 4, 5]), state))
    assert dead(got, 0) and dead(got, 2)
    want = one_call(ops, c[:4], K, ld_hyp=T_cap)
    assert same_bits([g[1] for g in got], [w[0] for w in want])
    got = host(ops.ctc_beam_chunk(block, G.i32([4, 0, 0]), state))                  # a valid count does not revive it
    assert dead(got, 0) and dead(got, 2) and same_bits([g[1] for g in got], [w[0] for w in want])
    assert (flat[need:] == 0x5A).all()
    # state_init revives every sequence
    state.init()
    fresh = readout(ops, state, V)
    assert (fresh[1][:, 0] == 0).all() and (fresh[2][:, 0] == 0.0).all()


def test_ld_hyp_shorter_than_a_hypothesis_reports_the_true_length(ops):
    z = np.load(os.path.join(GOLD, "ctc_beam.npz"))
    logp, K, ids, lens = z["logp_0"], int(z["beam_0"]), z["ids_0"], z["len_0"]
    assert lens.max() > 3
    dev = torch.from_numpy(logp).cuda()
    state = ops.ctc_beam_state(1, len(logp), 16, K)
    flat = torch.full((K * 3 + 64,), -7, dtype=I32, device="cuda")                  # the rows, then a guard zone
    hyp = flat[:K * 3].view(1, K, 3)
    t = 0
    for n in splits_of(len(logp))["sixteens"]:
        feed(ops, state, dev, t, n)
        t += n
    _, n_out, _ = ops.ctc_beam_chunk(dev[:1][None], G.i32([0]), state, hyp=hyp)
    torch.cuda.synchronize()
    assert np.array_equal(n_out.cpu().numpy()[0], lens)
    assert np.array_equal(hyp.cpu().numpy()[0], ids[:, :3]) and (flat[K * 3:] == -7).all()


def test_caller_bugs_raise_before_any_launch(ops):
    from f5e_tts_amd._C import F5EError
    V, K = 12, 4
    state = ops.ctc_beam_state(2, 30, 8, K)
    ok, n = torch.zeros(2, 8, V, device="cuda"), G.i32([1, 1])
    for bad_beam in (0, 17):
        with pytest.raises(F5EError, match="beam"):
            ops.ctc_beam_state(1, 30, 8, bad_beam)
    with pytest.raises(F5EError, match="chunk_cap"):
        ops.ctc_beam_chunk(torch.zeros(2, 9, V, device="cuda"), n, state)            # more frames than chunk_cap
    with pytest.raises(F5EError, match="same B"):
        ops.ctc_beam_chunk(ok[:1], G.i32([1]), state)
    with pytest.raises(F5EError, match="n_frames"):
        ops.ctc_beam_chunk(ok, n.long(), state)
    with pytest.raises(F5EError, match="beam"):
        ops.ctc_beam_chunk(ok[:, :, :3], n, state)                                   # beam above V
    with pytest.raises(F5EError, match="want_result"):
        ops.ctc_beam_chunk(ok, n, state, want_result=False, hyp=torch.zeros(2, K, 4, dtype=I32, device="cuda"))
    with pytest.raises(F5EError, match="CPU"):
        ops.ctc_beam_chunk(ok.cpu(), n, state)
    with pytest.raises(F5EError, match="buf"):
        ops.ctc_beam_state(2, 30, 8, K, buf=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    assert ops.ctc_beam_chunk(ok, n, state, want_result=False) is None
