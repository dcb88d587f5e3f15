"""Whisper word timestamps on the GPU (csrc/whisper_align.hip, eval/whisper.py) against
  * the NumPy restatement (tests/whisper_align_ref.py, pinned to ``transformers`` by tests/test_whisper_align_cpu.py), kernel by
    kernel;
  * the fixture made from ``transformers`` (tests/golden/whisper_align.npz): the frame indices exactly.

f5e_dtw_path: EXACT (``first`` and the -1 tail).  The recursion is fp32 additions and strict comparisons; the restatement runs it
in float32 on the same matrix.  Small-integer matrices are full of exact ties (the tie rule), random ones have none.

f5e_dtw_cost_f32: relative L2 against the float64 restatement below 10x the error that the float32 NumPy evaluation of the same
formulas shows against float64 on the same inputs (computed here, printed).

f5e_cross_attn_probs_f32: relative L2 against float64 below tol(Tk + dk) = 10 sqrt(Tk + dk) 2^-24, the bound of
f5e_cross_attn_decode_f32 in tests/test_whisper_gpu.py (the dk products of a score, the Tk terms of the normaliser); the kept
columns of a row sum to at most 1 (+ tol(Tk), the rounding of Tk fp32 terms).

Fixture: exact frame indices -- the generator asserted a gap of at least 1e-3 between the chosen predecessor and the runner-up on
every path cell, and the device's cost matrix must lie within a hundredth of the stored smallest gap of the stored matrix.

Every output and the workspace sit between canaries.  Every test prints its measured figures before it asserts.

Measured on an MI355X: see DESIGN.md 4o."""
import math

import numpy as np
import pytest
import torch

import whisper_align_ref as A
import whisper_ref as R
from test_whisper_align_cpu import N0, align_gold, align_model, heads
from test_whisper_cpu import gold

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
CANARY_I, CANARY_F = -77, -7.0
GUARD = 64


def tol(K):
    return 10.0 * math.sqrt(K) * 2.0 ** -24


def dev_i32(v):
    return torch.tensor(list(v), dtype=I32).cuda()


_dev = {}


def model_gpu(which):
    if ("model", which) not in _dev:
        _dev[("model", which)] = align_model(which).cuda()
    return _dev[("model", which)]


def kv_gpu(which, samples):
    key = ("kv", which, samples)
    if key not in _dev:
        wav = torch.from_numpy(gold()["wave_f32"][:samples].copy()).cuda()[None]
        _dev[key] = model_gpu(which).encode(wav)
    return _dev[key]


CASE_MODEL = {"a3s": "a", "a09cut": "a", "b3s": "b", "b09": "b", "b09eos": "beos"}


def case(c):
    """(model key, kv, tokens i32 [1, n] on the device, n, mel frames) of a fixture case."""
    ax = align_gold()
    frames = int(ax[f"nframes_{c}"])
    tok = torch.from_numpy(ax[f"tokens_{c}"].copy()).cuda()[None]
    return CASE_MODEL[c], kv_gpu(CASE_MODEL[c], frames * 160), tok, tok.shape[1], frames


# ---- f5e_dtw_path, exact -----------------------------------------------------------------------------------------------------------

def run_path(mats):
    """mats: one [n][m] float32 matrix per utterance -> first i32 [B][N_cap] from the device, under canaries."""
    from f5e_tts_amd import ops
    B, N_cap, M_cap = len(mats), max(m.shape[0] for m in mats), max(m.shape[1] for m in mats)
    cost = np.full((B, N_cap, M_cap), np.nan, np.float32)                 # cells outside (n, m) are never used
    for b, m in enumerate(mats):
        cost[b, :m.shape[0], :m.shape[1]] = m
    words = ops.dtw_workspace_bytes(B, N_cap, M_cap) // 4
    assert words == B * N_cap * ((M_cap + 15) // 16)
    fbuf = torch.full((B * N_cap + 2 * GUARD,), CANARY_I, dtype=I32, device="cuda")
    wbuf = torch.full((words + 2 * GUARD,), CANARY_I, dtype=I32, device="cuda")
    first = fbuf[GUARD:GUARD + B * N_cap].view(B, N_cap)
    ops.dtw_path(torch.from_numpy(cost).cuda(), dev_i32(m.shape[0] for m in mats), dev_i32(m.shape[1] for m in mats), first=first,
                 workspace=wbuf[GUARD:GUARD + words])
    torch.cuda.synchronize()
    for buf, n in ((fbuf, B * N_cap), (wbuf, words)):
        host = buf.cpu().numpy()
        assert (host[:GUARD] == CANARY_I).all() and (host[GUARD + n:] == CANARY_I).all(), "a canary was overwritten"
    return first.cpu().numpy()


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("N,M", ((1, 1), (1, 7), (5, 1), (3, 4), (7, 3), (64, 65), (65, 64), (100, 300), (448, 1500)))
def test_dtw_path_equals_the_restatement(N, M, B):
    g = np.random.default_rng(1000 * N + M + B)
    shapes = [(N, M), (max(N // 2, 1), max(M - 1, 1)), (N, max(M // 3, 1))][:B]          # ragged: shorter rows, shorter columns
    for kind in ("ties", "random"):
        mats = [g.integers(-2, 3, s).astype(np.float32) if kind == "ties" else g.standard_normal(s).astype(np.float32)
                for s in shapes]
        got = run_path(mats)
        for b, m in enumerate(mats):
            want = A.dtw_first(m)
            bad = int((got[b, :m.shape[0]] != want).sum())
            print(f"N={N} M={M} B={B} {kind} row {b} {m.shape}: {bad} of {m.shape[0]} entries differ, "
                  f"path enters the rows at columns {want[:4].tolist()} .. {want[-1]}")
            assert bad == 0
            assert (got[b, m.shape[0]:] == -1).all()


def test_dtw_path_refuses_and_marks_bad_lengths():
    from f5e_tts_amd import _C, ops
    cost = torch.zeros(2, 3, 5, device="cuda")
    first = ops.dtw_path(cost, dev_i32((0, 4)), dev_i32((5, 5)))                         # no rows / more rows than the matrix
    assert (first.cpu().numpy() == -1).all()
    first = ops.dtw_path(cost, dev_i32((3, 2)), dev_i32((6, 0)))                         # columns outside the matrix
    assert (first.cpu().numpy() == -1).all()
    with pytest.raises(_C.F5EError, match="N_cap <= 448"):
        ops.dtw_path(torch.zeros(1, 449, 4, device="cuda"), dev_i32((1,)), dev_i32((1,)))
    with pytest.raises(_C.F5EError, match="workspace"):
        ops.dtw_path(cost, dev_i32((3, 3)), dev_i32((5, 5)), workspace=torch.zeros(2, dtype=I32, device="cuda"))
    with pytest.raises(_C.F5EError, match="N_cap"):
        ops.dtw_workspace_bytes(1, 449, 10)


# ---- f5e_dtw_cost_f32 against float64 --------------------------------------------------------------------------------------------

def random_probs(g, S, N, M):
    """Rows of a softmax over M + 9 keys, cut to M: column deviations well away from 0."""
    x = 2.0 * g.standard_normal((S, N, M + 9))
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True))[..., :M].astype(np.float32)


@pytest.mark.parametrize("B", (1, 2))
@pytest.mark.parametrize("S", (1, 3))
@pytest.mark.parametrize("N,M", ((2, 4), (2, 3), (9, 8), (20, 150), (33, 257)))
def test_dtw_cost_against_float64(N, M, S, B):
    from f5e_tts_amd import ops
    g = np.random.default_rng(100 * N + M + 10 * S + B)
    shapes = [(N, M), (max(N - 1, 2), max(M - 2, 1))][:B]
    ld = (M + 3) // 4 * 4
    host = np.zeros((B, S, N, ld), np.float32)
    ps = [random_probs(g, S, n, m) for n, m in shapes]
    for b, p in enumerate(ps):
        host[b, :, :p.shape[1], :p.shape[2]] = p
    out = torch.full((B, N, ld), CANARY_F, dtype=F32, device="cuda")
    ops.dtw_cost_f32(torch.from_numpy(host).cuda(), dev_i32(s[0] for s in shapes), dev_i32(s[1] for s in shapes), 7, out=out)
    got = out.cpu().numpy()
    for b, p in enumerate(ps):
        n, m = p.shape[1:]
        want = A.cost_matrix(p, 7, np.float64)
        e32 = R.rel_l2(A.cost_matrix(p, 7, np.float32), want)
        e = R.rel_l2(got[b, :n, :m], want)
        print(f"N={N} M={M} heads={S} B={B} row {b} ({n} x {m}): rel L2 {e:.2e}, NumPy float32 {e32:.2e} (gate {10 * e32:.2e})")
        assert np.isfinite(got[b, :n, :m]).all()
        assert e <= 10 * e32                                               # both are exactly 0 on a one-column matrix of two rows
        assert (got[b, n:] == CANARY_F).all() and (got[b, :, m:] == CANARY_F).all(), "a cell outside (n_rows, m_len) was written"


def test_dtw_cost_constant_column_and_refusals():
    from f5e_tts_amd import _C, ops
    p = torch.from_numpy(random_probs(np.random.default_rng(3), 2, 4, 8)).cuda()[None].contiguous()
    p[0, :, :, 5] = 0.25                                                                # zero deviation: z = 0 there, not NaN
    got = ops.dtw_cost_f32(p, dev_i32((4,)), dev_i32((8,)), 1).cpu().numpy()           # width 1: no filter, the column itself
    assert np.isfinite(got).all() and (got[0, :, 5] == 0.0).all() and (got[0, :, 4] != 0.0).any()
    one = ops.dtw_cost_f32(p, dev_i32((1,)), dev_i32((8,)), 7).cpu().numpy()           # N = 1: every column is constant
    assert (one[0, 0] == 0.0).all()
    for width in (0, 4, 17):
        with pytest.raises(_C.F5EError, match="odd filter width"):
            ops.dtw_cost_f32(p, dev_i32((4,)), dev_i32((8,)), width)


# ---- f5e_cross_attn_probs_f32 against float64 ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dk", (16, 64))
@pytest.mark.parametrize("Tk", (1, 63, 150, 1500))
def test_cross_attn_probs_against_float64(Tk, dk):
    from f5e_tts_amd import ops
    H, B, sel = 3, 2, (2, 0)                                              # head 1 is not selected
    D = H * dk
    g = torch.Generator().manual_seed(77 * dk + Tk)
    for rpu in (1, 5):
        R_ = B * rpu
        q = torch.randn(R_, D, generator=g, dtype=torch.float64).to(F32)
        kv = torch.randn(B, Tk, D + 4, generator=g, dtype=torch.float64).to(F32)          # a row stride beyond D
        qd, kd = q.cuda(), kv.cuda()[..., :D]
        for m0 in (1, Tk // 2, Tk):
            m = (m0, max(Tk - m0, 0))                                                      # per utterance; 0 columns: nothing written
            buf = torch.full((R_, len(sel) + 1, Tk + 3), CANARY_F, dtype=F32, device="cuda")
            ops.cross_attn_probs_f32(qd, kd, dev_i32(sel), H, dk ** -0.5, buf[:, :len(sel), :Tk], rows_per_utt=rpu, m_len=dev_i32(m))
            got = buf.cpu().numpy().astype(np.float64)
            num = den = 0.0
            top = 0.0
            for r in range(R_):
                u = r // rpu
                for s, h in enumerate(sel):
                    want = A.softmax_rows(q[r, h * dk:(h + 1) * dk].numpy(), kv[u, :, h * dk:(h + 1) * dk].numpy(), dk ** -0.5)
                    num += ((got[r, s, :m[u]] - want[:m[u]]) ** 2).sum()
                    den += (want[:m[u]] ** 2).sum()
                    top = max(top, got[r, s, :m[u]].sum())
                    assert (got[r, s, m[u]:] == CANARY_F).all(), "a column at or beyond m_len was written"
            err = math.sqrt(num / den) if den else 0.0
            print(f"Tk={Tk} dk={dk} rows_per_utt={rpu} m_len={m}: rel L2 {err:.2e} (bound {tol(Tk + dk):.2e}), largest row sum "
                  f"{top:.7f}")
            assert (got[:, len(sel)] == CANARY_F).all(), "a slot beyond the selected heads was written"
            assert err < tol(Tk + dk) and top <= 1.0 + tol(Tk)


def test_cross_attn_probs_refusals():
    from f5e_tts_amd import _C, ops
    q = torch.zeros(2, 48, device="cuda")
    k = torch.zeros(1, 5, 48, device="cuda")
    out = torch.zeros(2, 1, 8, device="cuda")
    with pytest.raises(_C.F5EError, match="head dim"):
        ops.cross_attn_probs_f32(q, k, dev_i32((0,)), 2, 1.0, out, rows_per_utt=2)          # dk = 24
    with pytest.raises(_C.F5EError, match="inconsistent"):
        ops.cross_attn_probs_f32(q, k, dev_i32((0,)), 3, 1.0, out, rows_per_utt=1)          # 2 rows, 1 utterance
    buf = torch.full((2, 1, 8), CANARY_F, device="cuda")
    ops.cross_attn_probs_f32(q, k, dev_i32((3,)), 3, 1.0, buf, rows_per_utt=2)               # a head outside the layer: nothing
    assert (buf.cpu().numpy() == CANARY_F).all()


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------

def frames_of(times):
    """times f32 [n] in seconds -> integer frames; every time must be EXACTLY float32(frame * 0.02)."""
    t = times.cpu().numpy()
    fr = np.round(t.astype(np.float64) / 0.02).astype(np.int64)
    assert np.array_equal(t, (fr * 0.02).astype(np.float32))
    return fr


@pytest.mark.parametrize("c", ("a3s", "a09cut", "b3s", "b09", "b09eos"))
def test_token_timestamps_equal_the_fixture(c):
    from f5e_tts_amd import ops
    ax = align_gold()
    which, kv, tok, n, frames = case(c)
    model = model_gpu(which)
    times = model.token_timestamps(kv, tok, [n], frames, N0)
    got, want = frames_of(times[0]), ax[f"frames_{c}"]
    print(f"{c}: n = {n}, M = {frames // 2}, frames {got.tolist()}")
    assert times.shape == (1, n) and np.array_equal(got, want)
    probs, n_rows, m_len = model.alignment_probs(kv, tok, [n], frames, N0)
    N, M = ax[f"probs_{c}"].shape[1:]
    assert (int(n_rows[0]), int(m_len[0])) == (N, M)
    e_p = R.rel_l2(probs[0, :, :N, :M].cpu().numpy(), ax[f"probs_{c}"])
    print(f"{c}: probabilities against the fixture, rel L2 {e_p:.2e} (gate 2e-4)")
    assert e_p < 2e-4                                                   # the project's gate for fp32 chains against fixtures
    assert (probs[0, :, :, M:] == 0).all()                              # columns beyond M are not written
    if N >= 2:
        cost = ops.dtw_cost_f32(probs, n_rows, m_len, 7)[0, :N, :M].cpu().numpy()
        d, gap = float(np.abs(cost - ax[f"cost_{c}"]).max()), float(ax[f"gap_{c}"])
        print(f"{c}: cost matrix against the fixture, max abs {d:.2e}; smallest on-path gap {gap:.2e} (gate {gap / 100:.2e})")
        assert d < gap / 100


def test_generate_returns_the_fixture_tokens_and_times():
    fx, ax = gold(), align_gold()
    model = model_gpu("a")
    wav = torch.from_numpy(fx["wave_f32"][:48000].copy()).cuda()[None]
    plain = model.generate(wav, None, "en")
    tokens, n, times = model.generate(wav, None, "en", return_token_timestamps=True)
    assert len(plain) == 2 and torch.equal(plain[0], tokens) and torch.equal(plain[1], n)
    k = int(n[0])
    assert tokens[0, :k].tolist() == fx["tokens_48000"].tolist() == ax["tokens_a3s"].tolist()
    assert np.array_equal(frames_of(times[0, :k]), ax["frames_a3s"]) and times.shape == tokens.shape
    again = model.token_timestamps(kv_gpu("a", 48000), tokens, n, 300, N0)
    assert torch.equal(again, times)


def test_a_ragged_batch_equals_its_single_runs():
    ax = align_gold()
    model = model_gpu("b")
    n = [len(ax["tokens_b3s"]), len(ax["tokens_b09"])]
    frames = [int(ax["nframes_b3s"]), int(ax["nframes_b09"])]
    wav = torch.full((2, 48000), 0.5, dtype=F32)                         # garbage beyond the short row's length
    wav[0] = torch.from_numpy(gold()["wave_f32"][:48000].copy())
    wav[1, :14400] = torch.from_numpy(gold()["wave_f32"][:14400].copy())
    kv = model.encode(wav.cuda(), [48000, 14400])
    tok = torch.full((2, max(n)), 140, dtype=I32)
    tok[0, :n[0]] = torch.from_numpy(ax["tokens_b3s"].copy())
    tok[1, :n[1]] = torch.from_numpy(ax["tokens_b09"].copy())
    both = model.token_timestamps(kv, tok.cuda(), n, frames, N0)
    for b, c in enumerate(("b3s", "b09")):
        _, kv1, tok1, n1, fr1 = case(c)
        single = model.token_timestamps(kv1, tok1, [n1], fr1, N0)
        print(f"row {b} ({c}): batch {frames_of(both[b, :n1]).tolist()}")
        assert torch.equal(both[b, :n1], single[0]) and (both[b, n1:] == 0).all()
        assert np.array_equal(frames_of(both[b, :n1]), ax[f"frames_{c}"])


def test_beam_search_times_are_those_of_its_winner():
    model = model_gpu("a")
    kv = kv_gpu("a", 14400)
    prompt = gold()["prompt"].tolist()
    plain = model.generate_from_kv(kv, prompt, max_new_tokens=12, beam_size=5, return_beams=True)
    res = model.generate_from_kv(kv, prompt, max_new_tokens=12, beam_size=5, return_beams=True, return_token_timestamps=True, frames=90)
    assert len(plain) == 3 and len(res) == 4                             # the times come last
    tokens, n, beams, times = res
    assert torch.equal(tokens, plain[0]) and torch.equal(n, plain[1]) and torch.equal(beams[0], plain[2][0])
    want = model.token_timestamps(kv, tokens, n, 90, len(prompt))
    k = int(n[0])
    print(f"beam 5: {k} tokens, frames {frames_of(times[0, :k]).tolist()}")
    assert torch.equal(times, want) and times.shape == tokens.shape
    assert (times[0, :len(prompt)] == 0).all() and times[0, k - 1] == times[0, k - 2] and (times[0, k:] == 0).all()
    three = model.generate_from_kv(kv, prompt, max_new_tokens=12, beam_size=5, return_token_timestamps=True, frames=90)
    assert len(three) == 3 and torch.equal(three[2], times)


def test_recognizer_word_spans_and_align():
    from f5e_tts_amd.eval.whisper import WhisperRecognizer
    rec = WhisperRecognizer.__new__(WhisperRecognizer)                   # no checkpoint directory: the fixture's model as it is
    rec.device, rec.language, rec.beam_size, rec.model, rec._warned = torch.device("cuda"), "en", 1, model_gpu("a"), set()
    wav = torch.from_numpy(gold()["wave_f32"][:48000].copy())
    spans = rec.transcribe_words(wav, 16000)
    print("words:", [(s.word, round(s.start_s, 2), round(s.end_s, 2)) for s in spans])
    assert len(spans) >= 5 and all(s.word and s.word == s.word.strip() for s in spans)
    assert all(0.0 <= s.start_s <= s.end_s <= 3.0 for s in spans)
    assert all(a.end_s <= b.start_s + 1e-6 for a, b in zip(spans, spans[1:]))            # a word ends where the next one starts
    from f5e_tts_amd.ppg.ctc_align import split_words
    said = [s for s in spans if any(ch.isalnum() for ch in s.word)]     # align compares what is left without punctuation
    text = " ".join(s.word.upper() for s in said)
    got = rec.align(wav, 16000, text)
    assert [g.word for g in got] == [w for w in split_words(text) if any(ch.isalnum() for ch in w)]
    assert (got[0].start_s, got[-1].end_s) == (said[0].start_s, said[-1].end_s)
    assert all(a.start_s <= a.end_s <= b.start_s + 1e-6 for a, b in zip(got, got[1:]))
    with pytest.raises(ValueError, match="differ at word 1"):
        rec.align(wav, 16000, " ".join([said[0].word, "zzz"] + [s.word for s in said[2:]]))


def test_include_last_changes_only_the_number_of_rows():
    ax = align_gold()
    which, kv, tok, n, frames = case("b3s")
    model = model_gpu(which)
    p0, r0, m0 = model.alignment_probs(kv, tok, [n], frames, N0)
    p1, r1, m1 = model.alignment_probs(kv, tok, [n], frames, N0, include_last=True)
    N, M = int(r0[0]), int(m0[0])
    assert (int(r1[0]), int(m1[0])) == (N + 1, M) and torch.equal(p1[:, :, :N], p0)     # the same rows and one more
    times = model.token_timestamps(kv, tok, [n], frames, N0, include_last=True)
    want = A.token_frames(p1[0, :, :, :M].cpu().numpy(), n, N0, 7, np.float32, include_last=True)
    got = frames_of(times[0])
    print(f"include_last: {got.tolist()}")
    assert np.array_equal(got, want) and (got[:N0] == 0).all()
    assert np.array_equal(want, A.token_frames(p1[0, :, :, :M].cpu().numpy(), n, N0, 7, np.float64, include_last=True))
