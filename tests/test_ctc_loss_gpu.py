"""CTC transcript scoring on the GPU (csrc/ctc.hip: f5e_ctc_loss through ops.ctc_loss), ``ConformerPPG.ctc_loss``,
``CTCAligner.score`` / ``score_batch`` and best-of-N synthesis (``infer_batch_process(best_of=N, scorer=...)``).

The reference of every value is -torch.nn.functional.ctc_loss(reduction="none") on the float64 log_softmax, computed on the
host (``ctc_loss_ref.torch_logp``), and the tolerance is |got - ref| <= (4 + T) * 2^-24 * max(1, |ref|): one fp32 rounding at
the magnitude of the running value per frame, plus the closing logaddexp and the normaliser (``ctc_loss_ref.tolerance``).

Kernel boundaries exercised: S = 2 L + 1 states in runs of 64 -> one wave with 1 / 2 / 4 slots up to S = 64 / 128 / 256
(L = 31 | 32, 63 | 64), several waves beyond (L = 127 | 128), two | three waves at L = 255 | 256; emissions are prefetched 8
rows ahead in a loop of 16 (T = 1, 7, 8, 9, 16, 17)."""
import math
import os
import threading

import numpy as np
import pytest
import torch

import ctc_loss_ref as LR
import ctc_ref as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
I32, F32 = torch.int32, torch.float32
SENTINEL = 123.0


@pytest.fixture(scope="module")
def ops():
    import f5e_tts_amd.ops as ops_mod
    ops_mod.require_device()
    return ops_mod


def i32(v):
    return torch.as_tensor(np.asarray(v), dtype=I32).cuda()


def pack(rows, width=None):
    width = max([len(r) for r in rows] + [0]) if width is None else width
    out = np.zeros((len(rows), width), np.int32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def rand_labels(L, V, seed, repeats=0):
    rng = np.random.default_rng(seed)
    lab = []
    for i in range(L):
        v = int(rng.integers(1, V))
        while i > 0 and v == lab[-1] and V > 2:
            v = int(rng.integers(1, V))
        lab.append(v)
    for k in range(repeats):
        if L > 1:
            i = 1 + (k * 5) % (L - 1)
            lab[i] = lab[i - 1]
    return lab


def need(lab):
    return len(lab) + sum(1 for i in range(1, len(lab)) if lab[i] == lab[i - 1])


def expected(host, labels, t_len, l_len):
    """float64 torch per row; -inf for a row without a path (torch would refuse or return +inf)."""
    B, T, V = host.shape
    L = labels.shape[1]
    out = np.full(B, -np.inf)
    for b in range(B):
        t, l = int(t_len[b]), int(l_len[b])
        if 0 <= l <= L and 1 <= t <= T and LR.has_path(labels[b, :l], t, V):
            out[b] = LR.torch_logp(host[b:b + 1, :t], labels[b:b + 1, :l].astype(np.int64), [t], [l])[0]
    return out


def close(got, want, t_len, what=""):
    for b, (g, w) in enumerate(zip(got, want)):
        if np.isneginf(w):
            assert np.isneginf(g), f"{what} row {b}: {g} where there is no path"
            continue
        tol = LR.tolerance(int(t_len[b]), w)
        print(f"{what} row {b}: T={int(t_len[b])} ref {w:.6f} got {float(g):.6f} error {abs(float(g) - w):.3e} = "
              f"{100 * abs(float(g) - w) / tol:.1f}% of the bound")
        assert abs(float(g) - w) <= tol, f"{what} row {b}: got {g}, want {w}, tolerance {tol}"


def check_loss(ops, scores_dev, host, labels, t_len, l_len, blank=0, softmax_too=True, what=""):
    """Kernel within the tolerance of float64 torch; the output pre-filled with a sentinel; scores bit-identical afterwards;
    raw logits and their log_softmax within the tolerance of each other."""
    B, T, V = scores_dev.shape
    before = scores_dev.clone()
    logp = torch.full((B,), SENTINEL, dtype=F32, device="cuda")
    out = ops.ctc_loss(scores_dev, i32(labels), i32(t_len), i32(l_len), blank, logp=logp)
    torch.cuda.synchronize()
    assert out is logp and torch.equal(scores_dev, before)
    got = logp.cpu().numpy()
    assert not (got == SENTINEL).any() and not np.isnan(got).any()
    want = expected(host, labels, t_len, l_len)
    close(got, want, t_len, what)
    if softmax_too:
        lp = torch.log_softmax(scores_dev, dim=-1).contiguous()
        got2 = ops.ctc_loss(lp, i32(labels), i32(t_len), i32(l_len), blank).cpu().numpy()
        for b in range(B):
            if np.isneginf(want[b]):
                assert np.isneginf(got2[b])
            else:
                assert abs(float(got2[b]) - float(got[b])) <= LR.tolerance(int(t_len[b]), want[b])
    return got


def logits(B, T, V, seed, scale=2.0):
    return (scale * np.random.default_rng(seed).standard_normal((B, T, V))).astype(np.float32)


# ------------------------------------------------------------------ the kernel

@pytest.mark.parametrize("L", [0, 1, 31, 32, 63, 64, 127, 128, 255, 256])
def test_state_count_crossing_a_run_a_slot_count_or_a_wave(ops, L):
    V, T = 20, L + 21
    rows = [rand_labels(L, V, 300 + L, repeats=2 if L >= 3 else 0), rand_labels(max(L - 1, 0), V, 400 + L)]
    host = logits(2, T, V, 500 + L)
    check_loss(ops, torch.from_numpy(host).cuda(), host, pack(rows, L), [T, T - 5], [len(r) for r in rows], what=f"L={L}")


@pytest.mark.parametrize("T", [1, 7, 8, 9, 16, 17])
def test_frame_counts_around_the_prefetch_depth(ops, T):
    V = 11
    rows = [rand_labels(min(3, T), V, 600 + T), [], rand_labels(1, V, 700 + T)]
    host = logits(3, T, V, 800 + T)
    check_loss(ops, torch.from_numpy(host).cuda(), host, pack(rows, 3), [T, T, T], [len(r) for r in rows], what=f"T={T}")


@pytest.mark.parametrize("V", [5, 218, 4233])
def test_vocabulary_sizes_in_a_strided_view(ops, V):
    """ld > V and a batch stride above T * ld: the view's strides reach the kernel, the guard cells around it stay."""
    B, T, ld = 2, 37, V + 3
    rows = [rand_labels(12, V, 900 + V, repeats=1), rand_labels(5, V, 950 + V)]
    host = logits(B, T, V, 1000 + V)
    buf = torch.full((B, T + 2, ld), -7.25, device="cuda")
    view = buf[:, :T, :V]
    view.copy_(torch.from_numpy(host))
    assert view.stride(0) > T * ld and view.stride(1) == ld
    keep = buf.clone()
    check_loss(ops, view, host, pack(rows), [T, 30], [12, 5], what=f"V={V}")
    assert torch.equal(buf, keep)


def test_kernel_against_the_fp32_restatement(ops):
    """The kernel and ``ctc_loss_ref`` (fp32) do the same operations in the same order, each rounded to fp32; what differs is
    the exp / log1p of the two maths libraries, a few ulp of a value of at most log 3 per frame and state, far below one
    rounding of the running value (|alpha| of tens to hundreds here).  So the two agree within the bound that each has
    against float64; bit-equality is not asked.  Two waves (S = 301), repeats, a ragged pair."""
    V, T, L = 50, 180, 150
    rows = [rand_labels(150, V, 41, repeats=3), rand_labels(37, V, 42)]
    t_len, l_len = [T, 95], [150, 37]
    host = logits(2, T, V, 43)
    got = check_loss(ops, torch.from_numpy(host).cuda(), host, pack(rows, L), t_len, l_len, what="restated")
    mine = LR.loss(host, pack(rows, L), t_len, l_len, dtype=np.float32)
    for b in range(2):
        tol = LR.tolerance(t_len[b], mine[b])
        print(f"kernel {got[b]:.6f} restatement {mine[b]:.6f}: {100 * abs(float(got[b]) - float(mine[b])) / tol:.1f}% of the bound")
        assert abs(float(got[b]) - float(mine[b])) <= tol


def test_ragged_batch_in_a_larger_buffer(ops):
    V, T, L = 33, 90, 40
    rows = [rand_labels(40, V, 1), rand_labels(7, V, 2, repeats=2), [], rand_labels(33, V, 3), [4, 4, 4, 4]]
    t_len = [90, 31, 12, need(rows[3]), 7]
    host = logits(5, T, V, 4)
    lab = pack(rows, L)
    lab[1, 7:] = -1                                                  # padding past a length is never read as a label
    check_loss(ops, torch.from_numpy(host).cuda(), host, lab, t_len, [len(r) for r in rows], what="ragged")


def test_rows_without_a_path_give_minus_infinity_and_leave_their_neighbours(ops):
    V, T, L = 9, 12, 6
    good = [1, 2, 3]
    rows = [good, [5, 5, 6, 6, 6, 2], good, [1, V, 2], good, good, good, good]
    t_len = [12, 8, 12, 12, 12, 12, 0, 13]                           # row 1: 6 labels + 3 repeats need 9 frames
    l_len = [3, 6, 3, 3, 3, 7, 3, 3]                                 # row 5: l_len > L; rows 6 / 7: t_len < 1 / > T
    host = logits(8, T, V, 5)
    got = check_loss(ops, torch.from_numpy(host).cuda(), host, pack(rows, L), t_len, l_len, what="no path")
    assert np.isneginf(got[[1, 3, 5, 6, 7]]).all() and np.isfinite(got[[0, 2, 4]]).all()
    alone = check_loss(ops, torch.from_numpy(host[:1]).cuda(), host[:1], pack([good], L), [12], [3])
    assert got[0] == alone[0] != got[2]                              # the neighbours of a dead row keep their own values
    neg = ops.ctc_loss(torch.from_numpy(host).cuda(), i32(pack(rows, L)), i32(t_len), i32([3, -1, 3, 3, 3, 3, 3, 3])).cpu().numpy()
    assert np.isneginf(neg[1]) and neg[0] == got[0]                  # l_len < 0


def test_true_minus_infinity_gives_a_finite_value_or_minus_infinity_never_nan(ops):
    T, V, lab = 30, 8, [1, 2, 2, 5]
    lp = torch.log_softmax(torch.from_numpy(logits(1, T, V, 6, 1.0)[0]).double(), -1).numpy().astype(np.float32)
    lp[::3, 3] = -np.inf                         # a class no label uses
    lp[:4, 5] = -np.inf                          # the last label cannot start early
    lp[10, 0] = -np.inf                          # one frame cannot be blank
    dead_label, dead_frame = lp.copy(), lp.copy()
    dead_label[:, 2] = -np.inf                   # a label that can never be emitted: torch says +inf
    dead_frame[12, :] = -np.inf                  # a frame nothing can pass (torch's log_softmax gives NaN there: no reference)
    host = np.stack([lp, dead_label, dead_frame])
    labels = pack([lab] * 3)
    out = ops.ctc_loss(torch.from_numpy(host).cuda(), i32(labels), i32([T] * 3), i32([4] * 3)).cpu().numpy()
    assert not np.isnan(out).any() and np.isfinite(out[0]) and np.isneginf(out[1]) and np.isneginf(out[2])
    close(out[:2], expected(host[:2], labels[:2], [T, T], [4, 4]), [T, T], "-inf entries")
    # an empty transcript through frames whose blank is -inf, and l = 0 when the blank is fine
    blank_dead = lp.copy()
    blank_dead[5, 0] = -np.inf
    host = np.stack([blank_dead, lp])
    out = ops.ctc_loss(torch.from_numpy(host).cuda(), torch.zeros(2, 0, dtype=I32, device="cuda"), i32([T, 9]),
                       i32([0, 0])).cpu().numpy()
    assert np.isneginf(out[0]) and np.isfinite(out[1])
    close(out, expected(host, np.zeros((2, 0), np.int32), [T, 9], [0, 0]), [T, 9], "empty transcript")


def test_planted_scores_rate_their_own_labels_above_a_permutation(ops):
    V, T = 30, 120
    lab = rand_labels(25, V, 7)
    perm = list(np.random.default_rng(8).permutation(lab))
    assert perm != lab
    host = np.stack([R.planted(T, lab, V, 9)] * 2)
    got = check_loss(ops, torch.from_numpy(host).cuda(), host, pack([lab, perm]), [T, T], [25, 25], what="planted")
    assert got[0] > got[1] + 10.0, got           # 25 labels boosted by 4.0 each against noise


def test_captured_once_and_replayed_to_the_same_bits(ops):
    B, T, L, V = 2, 200, 150, 40
    labs = ([rand_labels(150, V, 11), rand_labels(20, V, 12)], [rand_labels(60, V, 13, repeats=3), rand_labels(149, V, 14)])
    lens = ([200, 170], [111, 200])
    scores = torch.empty(B, T, V, device="cuda")
    labels = torch.zeros(B, L, dtype=I32, device="cuda")
    t_len, l_len = torch.zeros(B, dtype=I32, device="cuda"), torch.zeros(B, dtype=I32, device="cuda")
    logp = torch.full((B,), SENTINEL, device="cuda")
    ws = torch.empty(ops.ctc_loss_workspace_bytes(B, T), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = ops.Graph()
        g.begin()
        try:
            ops.ctc_loss(scores, labels, t_len, l_len, 0, logp=logp, workspace=ws)
        finally:
            g.end()
        for k in range(2):
            host = logits(B, T, V, 15 + k)
            lab = pack(list(labs[k]), L)
            ll = [len(r) for r in labs[k]]
            scores.copy_(torch.from_numpy(host))
            labels.copy_(torch.from_numpy(lab))
            t_len.copy_(torch.tensor(lens[k], dtype=I32))
            l_len.copy_(torch.tensor(ll, dtype=I32))
            g.launch()
            s.synchronize()
            first = logp.cpu().numpy().copy()
            close(first, expected(host, lab, lens[k], ll), lens[k], f"graph {k}")
            logp.fill_(SENTINEL)
            g.launch()
            s.synchronize()
            assert np.array_equal(logp.cpu().numpy().view(np.int32), first.view(np.int32))
            eager = ops.ctc_loss(scores, labels, t_len, l_len, 0)
            s.synchronize()
            assert np.array_equal(eager.cpu().numpy().view(np.int32), first.view(np.int32))
        g.destroy()


def test_wrapper_rejects_what_the_kernel_cannot_take(ops):
    from f5e_tts_amd import _C
    sc = torch.zeros(2, 8, 5, device="cuda")
    lab, t, l = torch.ones(2, 3, dtype=I32, device="cuda"), i32([8, 8]), i32([3, 3])
    for bad in (lambda: ops.ctc_loss(sc, lab.long(), t, l), lambda: ops.ctc_loss(sc, lab.cpu(), t, l),
                lambda: ops.ctc_loss(sc, lab[:1], t, l), lambda: ops.ctc_loss(sc, lab, t[:1], l),
                lambda: ops.ctc_loss(sc, lab, t, l, logp=torch.zeros(3, device="cuda")),
                lambda: ops.ctc_loss(sc, lab, t, l, blank=5),
                lambda: ops.ctc_loss(sc, lab, t, l, workspace=torch.empty(15, dtype=F32, device="cuda"))):
        # f5e_last_error is thread-local and nothing clears it: calls that are meant to fail run on a thread of their own
        seen = []

        def attempt(fn=bad):
            try:
                fn()
                seen.append(False)
            except _C.F5EError:
                seen.append(True)
        th = threading.Thread(target=attempt)
        th.start()
        th.join()
        assert seen == [True]
    assert ops.ctc_loss(sc, lab, t, l).shape == (2,)


# ------------------------------------------------------------------ the model

@pytest.fixture(scope="module")
def asr():
    """The tiny ASR model of tests/golden (ppg_conformer.npz + the CTC head of ctc_asr.npz), as in test_ctc_gpu.py."""
    from f5e_tts_amd.ppg import ConformerPPG
    base = np.load(os.path.join(GOLD, "ppg_conformer.npz"))
    z = np.load(os.path.join(GOLD, "ctc_asr.npz"))
    sd = {k[2:]: torch.from_numpy(base[k]) for k in base.files if k.startswith("w/")}
    sd.update({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")})
    m = ConformerPPG(80, 40, 64, 4, 128, 2, 15, global_cmvn=(sd["encoder.global_cmvn.mean"], sd["encoder.global_cmvn.istd"]),
                     ctc=True)
    full = m.state_dict()
    full.update(sd)
    m.load_state_dict(full)
    return m.cuda().eval()


@pytest.mark.parametrize("use_linear", [True, False])
def test_model_ctc_loss_equals_torch_on_its_own_logits(ops, asr, use_linear):
    g = torch.Generator().manual_seed(21)
    feats = 4.0 * torch.randn(3, 101, 80, generator=g) + 8.0
    lens = torch.tensor([101, 77, 60])
    rows = [rand_labels(17, 39, 22, repeats=2), [], rand_labels(9, 39, 23)]
    text = torch.full((3, 17), -1, dtype=I32)                       # the reference's padding
    for b, r in enumerate(rows):
        text[b, :len(r)] = torch.tensor(r, dtype=I32)
    l_len = [len(r) for r in rows]
    lg, _, frames = asr._ctc_scores(feats.cuda(), lens, use_linear)
    host = lg.cpu().numpy()
    want = -expected(host, text.numpy().clip(min=0), frames.tolist(), l_len)
    assert np.isfinite(want).all() and frames.tolist()[0] > frames.tolist()[2]
    nll = asr.ctc_loss(feats.cuda(), lens, text, l_len, use_linear=use_linear, reduce=False)
    assert nll.is_cuda and nll.shape == (3,)
    close(-nll.cpu().numpy(), -want, frames.tolist(), f"model use_linear={use_linear}")
    lists = asr.ctc_loss(feats.cuda(), lens, rows, use_linear=use_linear, reduce=False)         # lists of ids: the same call
    assert torch.equal(lists, nll)
    red = asr.ctc_loss(feats.cuda(), lens, text, l_len, use_linear=use_linear)
    assert red.ndim == 0 and red.is_cuda and abs(float(red) - float(nll.sum()) / 3) <= 2.0 ** -22 * float(red)
    if use_linear:
        assert torch.equal(asr.ctc_loss(feats.cuda(), lens, text, l_len), red)                   # the default applies `linear`
    else:
        assert not torch.equal(asr.ctc_loss(feats.cuda(), lens, text, l_len), red)


def test_golden_ctc_forward_through_gemm_and_kernel(ops):
    z = np.load(os.path.join(GOLD, "ctc_loss.npz"))
    W, bias = torch.from_numpy(z["ctc_lo_weight"]).cuda(), torch.from_numpy(z["ctc_lo_bias"]).cuda()
    for i in range(int(z["n_cases"])):
        hs, hl, ys, yl = z[f"hs_pad_{i}"], z[f"hlens_{i}"], z[f"ys_pad_{i}"], z[f"ys_lens_{i}"]
        B, T, D = hs.shape
        lg = torch.empty(B * T, W.shape[0], device="cuda")
        ops.gemm_f32(torch.from_numpy(hs).cuda().reshape(B * T, D), W, bias, out=lg)
        nll = -ops.ctc_loss(lg.view(B, T, -1), i32(ys), i32(hl), i32(yl)).cpu().numpy().astype(np.float64)
        per = z[f"per_utt_{i}"]
        tols = [LR.tolerance(int(t), v) + 2.0 ** -23 * abs(float(v)) for t, v in zip(hl, per)]   # + the fixture's own fp32
        for b in range(B):
            assert abs(nll[b] - per[b]) <= tols[b], (i, b, nll[b], per[b])
        assert abs(nll.sum() / B - float(z[f"loss_{i}"])) <= sum(tols) / B + 2.0 ** -23 * float(z[f"loss_{i}"])


# ------------------------------------------------------------------ the scorer

TABLE = {ch: 1 + k for k, ch in enumerate("abcdefghijklmnopqrstuvwxyz")}


@pytest.fixture(scope="module")
def aligner(asr):
    from f5e_tts_amd.ppg.ctc_align import CTCAligner
    return CTCAligner(model=asr, symbol_table=TABLE)


def speech_like(n, sr, seed, rows=1):
    """Band-limited noise well below 8 kHz with a slow envelope, at fbank-friendly amplitude."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / sr
    x = torch.zeros(rows, n, dtype=torch.float64)
    for _ in range(24):
        f = 80.0 + 3400.0 * torch.rand(rows, 1, generator=g, dtype=torch.float64)
        ph = 2 * math.pi * torch.rand(rows, 1, generator=g, dtype=torch.float64)
        x += torch.rand(rows, 1, generator=g, dtype=torch.float64) * torch.sin(2 * math.pi * f * t + ph)
    return (0.05 * x * (1.0 + 0.5 * torch.sin(2 * math.pi * 3.0 * t))).float()


def test_score_batch_equals_score_calls(ops, aligner):
    waves = speech_like(24000, 24000, 31, rows=3).cuda()
    text = "some words to say"
    batch = aligner.score_batch(waves, 24000, text)
    assert batch.is_cuda and batch.shape == (3,) and batch.dtype == F32
    single = [aligner.score(waves[b], 24000, text) for b in range(3)]
    frames = (1 + (16000 - 400) // 160 - 3) // 2 + 1
    assert all(math.isfinite(v) for v in single) and len(set(single)) == 3
    for b in range(3):
        assert abs(float(batch[b]) - single[b]) <= LR.tolerance(frames, single[b]), (b, float(batch[b]), single[b])
    assert aligner.score(waves[0], 24000, "words") != single[0]
    with pytest.raises(ValueError, match="symbol table"):
        aligner.score(waves[0], 24000, "1234 !?")
    with pytest.raises(ValueError, match="symbol table"):
        aligner.score_batch(waves, 24000, "...")
    from f5e_tts_amd import _C
    with pytest.raises(_C.F5EError, match="no CPU path"):
        aligner.score_batch(waves.cpu(), 24000, text)


def test_score_follows_the_sample_rate_route_as_far_as_the_resampler_does(ops, aligner):
    """The same audio given at 24 kHz and, resampled in float64 on the host with the resampler's own filter bank, at 16 kHz.
    The 24 kHz route differs from the 16 kHz one by the device resampler's fp32 error alone, which tests/test_resample_gpu.py
    bounds per sample by gamma_T * (|bank| * |x|), gamma_T = T u / (1 - T u), T = taps, u = 2^-24.  The tolerance on the score
    is what a perturbation of THAT size does to it: the largest change of ``score`` among 8 random-sign perturbations of the
    16 kHz input with every sample moved by its full bound (rounding errors reach the bound on few samples, if any), plus
    the kernel's own tolerance twice."""
    import torch.nn.functional as F

    from f5e_tts_amd.infer import audio as A
    text = "some words to say"
    x24 = speech_like(36000, 24000, 41)
    bank, width, orig, new = A.sinc_resample_kernel(24000, 16000)
    taps, n = bank.shape[-1], x24.shape[-1]
    n_out = -(-new * n // orig)
    xp = F.pad(x24.double(), (width, width + orig))[:, None]
    x16 = F.conv1d(xp, bank.double(), stride=orig).transpose(1, 2).reshape(1, -1)[:, :n_out]
    mag = F.conv1d(xp.abs(), bank.double().abs(), stride=orig).transpose(1, 2).reshape(1, -1)[:, :n_out]
    u = 2.0 ** -24
    bound = taps * u / (1 - taps * u) * mag
    base = aligner.score(x16.float(), 16000, text)
    g = torch.Generator().manual_seed(42)
    moved = 0.0
    for _ in range(8):
        sign = torch.randint(0, 2, bound.shape, generator=g).double() * 2 - 1
        moved = max(moved, abs(aligner.score((x16 + sign * bound).float(), 16000, text) - base))
    frames = (1 + (n_out - 400) // 160 - 3) // 2 + 1
    tol = moved + 2 * LR.tolerance(frames, base)
    via24 = aligner.score(x24, 24000, text)
    print(f"score at 16 kHz {base:.6f}, through the 24 kHz route {via24:.6f}; perturbation at the resampler's bound moves it "
          f"by {moved:.3e}; tolerance {tol:.3e}")
    assert math.isfinite(base) and abs(via24 - base) <= tol


# ------------------------------------------------------------------ best-of-N end to end

@pytest.fixture(scope="module")
def tts():
    """The smallest synthetic DiT (one block) with a character vocabulary, Vocos on synthetic weights, a 0.4 s prompt."""
    from f5e_tts_amd.model import CFM, DiT
    from f5e_tts_amd.vocoder import Vocos
    from tools import synth as SY
    arch = dict(dim=1024, depth=1, heads=16, ff_mult=2, text_dim=256, conv_layers=1, text_num_embeds=300)
    dit = DiT(**arch)
    dit.load_state_dict(SY.init_dit_state(SY.DiTConfig(**arch), 1234), strict=True)
    vocab = {chr(32 + k): k for k in range(95)}                                  # the text reaches the model as characters
    cfm = CFM(transformer=dit, vocab_char_map=vocab).cuda().eval()
    voc = Vocos()
    voc.load_state_dict(SY.init_vocos_state(), strict=False)
    return cfm, voc.cuda(), (SY.synthetic_ref_wave(40), 24000)


def synth(tts, texts, **more):
    from f5e_tts_amd.infer import utils_infer as U
    cfm, voc, ref = tts
    return next(U.infer_batch_process(ref, "Ref text. ", texts, cfm, voc, nfe_step=4, device="cuda", cross_fade_duration=0.0,
                                      **more))[0]


def test_best_of_three_keeps_the_candidate_the_scorer_prefers(ops, aligner, tts):
    text = "a few words here"
    runs = []
    for _ in range(2):
        report = []
        wave = synth(tts, [text], best_of=3, scorer=aligner, seed=100, report=report)
        runs.append((wave, report))
        assert len(report) == 1 and report[0]["seeds"] == [100, 101, 102] and len(report[0]["scores"]) == 3
    (wave, report), (wave2, report2) = runs
    assert np.array_equal(wave, wave2) and report == report2                     # a second run reproduces all of it
    scores, chosen = report[0]["scores"], report[0]["chosen"]
    assert all(math.isfinite(v) for v in scores) and len(set(scores)) == 3
    assert chosen == int(np.argmax(scores)) == scores.index(max(scores))
    alone = [synth(tts, [text], best_of=1, seed=100 + i) for i in range(3)]
    assert np.array_equal(wave, alone[chosen]) and not np.array_equal(alone[0], alone[1])
    n16 = -(-2 * len(wave) // 3)
    frames = (1 + (n16 - 400) // 160 - 3) // 2 + 1
    for i in range(3):
        one = aligner.score(torch.from_numpy(alone[i]), 24000, text)
        assert abs(one - scores[i]) <= LR.tolerance(frames, one), (i, one, scores[i])


def test_worker_threads_handle_whole_chunks_candidates_included(ops, aligner, tts, monkeypatch):
    """F5E_INFER_WORKERS=2: a worker runs a chunk's candidates and its scoring on its own stream; with seeds given, the
    waveform, the scores' choice and the report's order are those of the calling thread alone."""
    texts = ["a few words here", "and some more of them"]
    serial, threaded = [], []
    want = synth(tts, texts, best_of=2, scorer=aligner, seed=7, report=serial)
    monkeypatch.setenv("F5E_INFER_WORKERS", "2")
    got = synth(tts, texts, best_of=2, scorer=aligner, seed=7, report=threaded)
    assert [r["seeds"] for r in serial] == [r["seeds"] for r in threaded] == [[7, 8], [9, 10]]
    assert [r["chosen"] for r in serial] == [r["chosen"] for r in threaded]
    assert np.array_equal(want, got)
