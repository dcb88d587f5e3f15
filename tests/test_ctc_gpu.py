"""CTC forced alignment and best-path decoding on the GPU (csrc/ctc.hip through ops.ctc_align / ops.ctc_greedy) and the CTC
half of the ASR model (ConformerPPG(ctc=True)) against
  * the REFERENCE's own ``forced_align`` / ``ctc_greedy_search`` outputs (tests/golden/ctc_align.npz, ctc_asr.npz; the
    generator asserts that no stored decision is fragile), and
  * the NumPy restatement (tests/ctc_ref.py, pinned by the same fixtures) on shapes the reference's Python loop cannot cover
    and on unplanted scores, where the reference's negative index at state 0 makes IT the wrong yardstick.
Paths and hypotheses are discrete: every such comparison is exact, and the path score is compared bit for bit.

Kernel boundaries exercised (csrc/ctc.hip): S = 2 L + 1 states in runs of 64 -> one wave with 1 / 2 / 4 slots up to
S = 64 / 128 / 256 (L = 31 / 63 / 127), then waves of 256 states (L = 255 | 256 is the 2 | 3 wave boundary); emissions are
prefetched 8 rows ahead in a loop of 16; the backtrack resolves 64 rows per round; the collapse runs 1024 frames per round."""
import os
import threading

import numpy as np
import pytest
import torch

import ctc_ref as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
I32, F32 = torch.int32, torch.float32


@pytest.fixture(scope="module")
def ops():
    import f5e_tts_amd.ops as ops_mod
    ops_mod.require_device()
    return ops_mod


def i32(v):
    return torch.as_tensor(np.asarray(v), dtype=I32).cuda()


def expect_error(kind, fn):
    try:
        fn()
    except kind:
        return True
    return False


def pack(rows, width=None):
    width = width or max(len(r) for r in rows)
    out = np.zeros((len(rows), width), np.int32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def check_align(ops, scores_dev, scores_host, labels, t_len, l_len, blank=0):
    """Kernel == restatement, exactly (align, spans, score bits); sentinel-filled outputs show no stale element; scores
    untouched."""
    B, T, V = scores_dev.shape
    L = labels.shape[1]
    before = scores_dev.clone()
    al = torch.full((B, T), -7, dtype=I32, device="cuda")
    ts = torch.full((B, L), -7, dtype=I32, device="cuda")
    te = torch.full((B, L), -7, dtype=I32, device="cuda")
    sc = torch.full((B,), 123.0, dtype=F32, device="cuda")
    ops.ctc_align(scores_dev, i32(labels), i32(t_len), i32(l_len), blank, align=al, tok_start=ts, tok_end=te, score=sc)
    torch.cuda.synchronize()
    want = R.align(np.asarray(scores_host), labels, t_len, l_len, blank)
    got = [x.cpu().numpy() for x in (al, ts, te, sc)]
    assert np.array_equal(got[0], want[0]), f"align differs in {(got[0] != want[0]).sum()} frames"
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[3].view(np.int32), want[3].view(np.int32)), (got[3], want[3])
    assert torch.equal(scores_dev, before)
    return got


def planted_batch(shapes, V, seed, T_buf=None, plant=True):
    """shapes: [(T, labels)] -> (scores f32 [B, T_buf, V] host, labels [B, L], t_len, l_len)."""
    T_buf = T_buf or max(t for t, _ in shapes)
    rng = np.random.default_rng(seed)
    scores = rng.standard_normal((len(shapes), T_buf, V)).astype(np.float32)
    for b, (t, lab) in enumerate(shapes):
        if plant:
            scores[b, :t] = R.planted(t, lab, V, seed + 17 * b + 1)
    return scores, pack([lab for _, lab in shapes]), [t for t, _ in shapes], [len(lab) for _, lab in shapes]


def rand_labels(L, V, seed, distinct_neighbours=False):
    rng = np.random.default_rng(seed)
    lab = rng.integers(1, V, size=L)
    if distinct_neighbours:
        for i in range(1, L):
            while lab[i] == lab[i - 1]:
                lab[i] = rng.integers(1, V)
    return lab.astype(np.int64)


def need(lab):
    return len(lab) + int((np.asarray(lab)[1:] == np.asarray(lab)[:-1]).sum())


# ------------------------------------------------------------------ the kernel against the reference's alignments

def test_kernel_equals_the_reference_alignments(ops):
    z = np.load(os.path.join(GOLD, "ctc_align.npz"))
    for i in range(int(z["n_cases"])):
        logp, labels, want = z[f"logp_{i}"], z[f"labels_{i}"], z[f"align_{i}"]
        T = logp.shape[0]
        got = check_align(ops, torch.from_numpy(logp)[None].cuda(), logp[None], labels[None], [T], [len(labels)])
        assert np.array_equal(got[0][0], want)
        # defaults: outputs allocated by the wrapper; spans=False returns the path alone
        al, ts, te, sc = ops.ctc_align(torch.from_numpy(logp)[None].cuda(), i32(labels[None]), i32([T]), i32([len(labels)]))
        assert np.array_equal(al.cpu().numpy()[0], want) and ts.shape == te.shape == (1, len(labels)) and sc.shape == (1,)
        al2, ts2, te2, sc2 = ops.ctc_align(torch.from_numpy(logp)[None].cuda(), i32(labels[None]), i32([T]),
                                           i32([len(labels)]), spans=False)
        assert torch.equal(al2, al) and ts2 is None and te2 is None and sc2 is None


# ------------------------------------------------------------------ the kernel against the restatement at the mapping's edges

@pytest.mark.parametrize("L", [31, 32, 33, 63, 64, 127, 128, 129, 255, 256])
def test_state_count_crossing_a_run_a_slot_count_or_a_wave(ops, L):
    V = 37
    lab = rand_labels(L, V, 800 + L)
    for plant, T in ((True, need(lab) + 2 * L + 5), (False, need(lab) + L + 3)):      # T off the prefetch depth's grid
        scores, labels, t_len, l_len = planted_batch([(T, lab)], V, 900 + L, plant=plant)
        check_align(ops, torch.from_numpy(scores).cuda(), scores, labels, t_len, l_len)


def test_longest_sequence_2047_labels_4200_frames(ops):
    V, L, T = 64, 2047, 4200
    lab = rand_labels(L, V, 31, distinct_neighbours=True)
    scores, labels, t_len, l_len = planted_batch([(T, lab), (T, lab)], V, 32)
    scores[1] = np.random.default_rng(33).standard_normal((T, V)).astype(np.float32)          # unplanted
    got = check_align(ops, torch.from_numpy(scores).cuda(), scores, labels, t_len, l_len)
    assert R.is_ctc_path(got[0][0], lab) and R.is_ctc_path(got[0][1], lab)


@pytest.mark.parametrize("T", [1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129])
def test_frame_counts_around_the_prefetch_depth_and_the_backtrack_round(ops, T):
    V = 11
    lab = rand_labels(max(1, min(T // 2, 20)), V, 40 + T, distinct_neighbours=True)
    for plant in (True, False):
        scores, labels, t_len, l_len = planted_batch([(T, lab)], V, 50 + T, plant=plant)
        check_align(ops, torch.from_numpy(scores).cuda(), scores, labels, t_len, l_len)


def test_minimum_feasible_length_forces_the_path(ops):
    """t_len = labels + adjacent repeats: every label gets one frame, equal neighbours exactly one blank between them."""
    lab = np.array([3, 3, 5, 5, 5, 2, 7, 7, 1] * 9, np.int64)
    T = need(lab)
    scores, labels, t_len, l_len = planted_batch([(T, lab)], 9, 61, plant=False)
    got = check_align(ops, torch.from_numpy(scores).cuda(), scores, labels, t_len, l_len)
    want = []
    for i, y in enumerate(lab):
        want += ([0] if i and lab[i - 1] == y else []) + [int(y)]
    assert got[0][0].tolist() == want and (got[2][0] - got[1][0] == 1).all()
    t_short = [T - 1]                                             # one frame fewer: no path
    al, ts, te, sc = ops.ctc_align(torch.from_numpy(scores).cuda(), i32(labels), i32(t_short), i32(l_len))
    assert (al == -1).all() and (ts == 0).all() and (te == 0).all() and float(sc[0]) == -np.inf


def test_all_labels_equal_and_all_labels_distinct(ops):
    V = 200
    same = np.full(70, 9, np.int64)                               # no skip anywhere
    distinct = np.arange(1, 151, dtype=np.int64)                  # a skip at every label
    for plant in (True, False):
        scores, labels, t_len, l_len = planted_batch([(need(same) + 40, same), (331, distinct)], V, 70, plant=plant)
        check_align(ops, torch.from_numpy(scores).cuda(), scores, labels, t_len, l_len)


def test_ragged_batch_mixing_the_cases(ops):
    V = 50
    shapes = [(700, rand_labels(300, V, 1)), (need(rand_labels(120, 5, 2)), rand_labels(120, 5, 2)), (1, np.array([4])),
              (699, np.array([7])), (333, rand_labels(33, V, 3)), (64, rand_labels(31, V, 4, True)),
              (513, rand_labels(256, V, 5, True)), (257, rand_labels(128, V, 6, True))]
    for plant in (True, False):
        scores, labels, t_len, l_len = planted_batch(shapes, V, 80, T_buf=700, plant=plant)
        got = check_align(ops, torch.from_numpy(scores).cuda(), scores, labels, t_len, l_len)
        for b in (0, 4):                                          # a sequence of a batch gets what it gets alone
            solo = ops.ctc_align(torch.from_numpy(scores[b:b + 1]).cuda(), i32(labels[b:b + 1]), i32(t_len[b:b + 1]),
                                 i32(l_len[b:b + 1]))
            assert np.array_equal(solo[0].cpu().numpy()[0], got[0][b]) and float(solo[3][0]) == float(got[3][b])


def test_strided_view_with_ld_above_v_and_a_batch_stride_of_two_matrices(ops):
    big = torch.randn(4, 150, 80, generator=torch.Generator().manual_seed(90)).cuda()
    view = big[::2, :, 3:60]
    assert view.stride() == (2 * 150 * 80, 80, 1)
    host = view.cpu().contiguous().numpy()
    labels = pack([rand_labels(40, 57, 91), rand_labels(70, 57, 92)])
    check_align(ops, view, host, labels, [150, 149], [40, 70])
    lab_wide = torch.zeros(2, 90, dtype=I32)                      # labels as a view too (ld_labels > L)
    lab_wide[:, :70] = torch.from_numpy(labels)
    al, *_ = ops.ctc_align(view, lab_wide.cuda()[:, :70], i32([150, 149]), i32([40, 70]))
    assert np.array_equal(al.cpu().numpy(), R.align(host, labels, [150, 149], [40, 70])[0])


def test_constant_matrix_every_decision_is_a_tie(ops):
    """stay wins every tie and the end state is the last blank: the path runs through the labels as fast as the skips allow
    and then stays in the final blank."""
    scores = np.zeros((1, 300, 20), np.float32)
    lab = rand_labels(100, 20, 95, distinct_neighbours=True)
    got = check_align(ops, torch.from_numpy(scores).cuda(), scores, lab[None].astype(np.int32), [300], [100])
    assert got[0][0, :100].tolist() == lab.tolist() and (got[0][0, 100:] == 0).all() and got[3][0] == 0.0


def test_degenerate_device_lengths_give_defined_rows_and_leave_the_rest_alone(ops):
    V, T, L = 30, 120, 40
    rng = np.random.default_rng(96)
    scores = rng.standard_normal((7, T, V)).astype(np.float32)
    labels = np.stack([rand_labels(L, V, 97 + b, distinct_neighbours=True) for b in range(7)]).astype(np.int32)
    labels[5, :3] = 6                                             # two adjacent repeats: needs l + 2 frames
    labels[6, 10] = V                                             # a label that is no class
    t_len = [120, 0, 39, 121, 100, 41, 120]
    l_len = [40, 5, 40, 10, 41, 40, 40]
    got = check_align(ops, torch.from_numpy(scores).cuda(), scores, labels, t_len, l_len)
    for b in range(1, 7):
        assert (got[0][b] == -1).all() and (got[1][b] == 0).all() and (got[2][b] == 0).all() and got[3][b] == -np.inf
    solo = ops.ctc_align(torch.from_numpy(scores[:1]).cuda(), i32(labels[:1]), i32([120]), i32([40]))
    assert np.array_equal(solo[0].cpu().numpy()[0], got[0][0])
    labels[6, 10] = 1
    check_align(ops, torch.from_numpy(scores).cuda(), scores, labels, [120, 90, 60, 120, 100, 42, 77],
                [40, 5, 40, 10, 1, 40, 33])                       # all valid: every row changes, none is stale


def test_scores_of_minus_infinity_leave_no_stale_span(ops):
    """Log-probs from a hard mask: every alpha ends at -inf, the backtrack stays in the last blank and visits no label.  The
    spans of those labels are 0 / 0 (sentinel-filled buffers show that they are written), the score is -inf."""
    scores = np.full((2, 40, 9), -np.inf, np.float32)
    scores[1] = R.planted(40, [3, 4, 4, 1], 9, 77)            # a finite neighbour in the same batch
    labels = pack([[2, 5, 5, 7, 1, 3], [3, 4, 4, 1]])
    got = check_align(ops, torch.from_numpy(scores).cuda(), scores, labels, [40, 40], [6, 4])
    assert (got[0][0] == 0).all() and (got[1][0] == 0).all() and (got[2][0] == 0).all() and got[3][0] == -np.inf
    assert (got[2][1, :4] > got[1][1, :4]).all() and np.isfinite(got[3][1])


def test_wrapper_rejects_what_the_kernel_cannot_take(ops):
    from f5e_tts_amd import _C
    sc = torch.zeros(1, 8, 5, device="cuda")
    lab, t, l = i32([[1, 2]]), i32([8]), i32([2])
    for bad in (lambda: ops.ctc_align(sc.cpu(), lab, t, l), lambda: ops.ctc_align(sc, lab.cpu(), t, l),
                lambda: ops.ctc_align(sc, lab, t.cpu(), l), lambda: ops.ctc_align(sc, lab.long(), t, l),
                lambda: ops.ctc_align(sc, lab, t, l, blank=5),
                lambda: ops.ctc_align(sc, lab, t, l, align=torch.empty(1, 7, dtype=I32, device="cuda")),
                lambda: ops.ctc_align(sc, lab, t, l, workspace=torch.empty(7, dtype=torch.uint8, device="cuda")),
                lambda: ops.ctc_align(sc, torch.ones(1, 2048, dtype=I32, device="cuda"), t, l),
                lambda: ops.ctc_greedy(sc, t, blank=0, pad_id=5), lambda: ops.ctc_greedy(sc.cpu(), t),
                lambda: ops.ctc_greedy(sc, t, hyp=torch.empty(1, 7, dtype=I32, device="cuda"))):
        # f5e_last_error is thread-local and nothing clears it: calls that are meant to fail run on a thread of their own
        seen = []
        th = threading.Thread(target=lambda: seen.append(expect_error(_C.F5EError, bad)))
        th.start()
        th.join()
        assert seen == [True]


def test_align_captured_once_and_replayed_with_new_contents_and_lengths(ops):
    B, T, L, V = 2, 400, 150, 40
    labs = ([rand_labels(150, V, 101), rand_labels(20, V, 102)], [rand_labels(90, V, 103), rand_labels(149, V, 104, True)])
    lens = ([400, 300], [222, 400])
    scores = torch.empty(B, T, V, device="cuda")
    labels = torch.zeros(B, L, dtype=I32, device="cuda")
    t_len, l_len = torch.zeros(B, dtype=I32, device="cuda"), torch.zeros(B, dtype=I32, device="cuda")
    al, ts, te = (torch.zeros(B, n, dtype=I32, device="cuda") for n in (T, L, L))
    sc = torch.zeros(B, device="cuda")
    ws = torch.empty(ops.ctc_align_workspace_bytes(B, T, L), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = ops.Graph()
        g.begin()
        try:
            ops.ctc_align(scores, labels, t_len, l_len, 0, align=al, tok_start=ts, tok_end=te, score=sc, workspace=ws)
        finally:
            g.end()
        for k in range(2):
            host, lab, tl, ll = planted_batch(list(zip(lens[k], labs[k])), V, 110 + k, T_buf=T)
            lab = pack(list(labs[k]), L)
            scores.copy_(torch.from_numpy(host))
            labels.copy_(torch.from_numpy(lab))
            t_len.copy_(torch.tensor(tl, dtype=I32))
            l_len.copy_(torch.tensor(ll, dtype=I32))
            g.launch()
            s.synchronize()
            want = R.align(host, lab, tl, ll)
            for got, w in zip((al, ts, te), want):
                assert np.array_equal(got.cpu().numpy(), w)
            assert np.array_equal(sc.cpu().numpy().view(np.int32), want[3].view(np.int32))
        g.destroy()


# ------------------------------------------------------------------ greedy search

def distinct_scores(B, T, V, seed):
    """Every frame holds V distinct values (a random permutation of an arithmetic grid): no argmax tie by construction."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.rand(B, T, V, generator=g).argsort(-1).to(F32)
    scores = perm * (12.0 / V) - 6.0
    assert int((scores.sort(-1).values.diff(dim=-1) <= 0).sum()) == 0
    return scores


def check_greedy(ops, scores, t_len, blank, pad_id):
    B, T, V = scores.shape
    dev = scores.cuda()
    hyp = torch.full((B, T), -7, dtype=I32, device="cuda")
    hyp_len = torch.full((B,), -7, dtype=I32, device="cuda")
    logp = torch.full((B, T), 7.0, device="cuda")
    ops.ctc_greedy(dev, i32(t_len), blank, pad_id, hyp=hyp, hyp_len=hyp_len, frame_logp=logp)
    torch.cuda.synchronize()
    want, _ = R.greedy(scores.numpy(), t_len, blank, pad_id)
    hyp, hyp_len = hyp.cpu().numpy(), hyp_len.cpu().numpy()
    for b in range(B):
        n = len(want[b])
        assert hyp_len[b] == n and hyp[b, :n].tolist() == want[b] and (hyp[b, n:] == -1).all()
    ref = torch.log_softmax(scores.double(), -1).max(-1).values.float()
    torch.testing.assert_close(logp.cpu(), ref, rtol=1e-5, atol=3e-5)
    assert torch.equal(dev.cpu(), scores)
    return hyp, hyp_len


@pytest.mark.parametrize("V,T", [(2, 2500), (63, 1100), (64, 1024), (65, 1025), (5000, 300)])
def test_greedy_equals_the_restatement(ops, V, T):
    scores = distinct_scores(3, T, V, 200 + V)
    # long runs, so that the collapse has something to collapse: hold every frame's winner for a few frames
    hold = torch.arange(T) // 3 * 3
    scores = scores[:, hold]
    t_len = [T, T // 2 + 1, 1]
    for blank, pad_id in ((0, -1), (0, V - 1), (V - 1, 0)):
        check_greedy(ops, scores, t_len, blank, pad_id)
    h_a = ops.ctc_greedy(scores.cuda(), i32(t_len))                     # defaults: no log-probs unless asked for
    assert h_a[2] is None and h_a[0].shape == (3, T)
    assert ops.ctc_greedy(scores.cuda(), i32(t_len), want_logp=True)[2].shape == (3, T)


def test_greedy_all_blank_all_one_token_and_lengths_outside_the_buffer(ops):
    T, V = 1300, 10
    scores = distinct_scores(4, T, V, 300)
    scores[0, :, 0] = 50.0                                              # blank wins every frame
    scores[1, :, 4] = 50.0                                              # one token wins every frame
    scores[2, :, 0] = 50.0
    scores[2, 1029, 7] = 60.0                                           # a single token in the second collapse round
    hyp, hyp_len = check_greedy(ops, scores, [T, T, T, 0], 0, -1)
    assert hyp_len.tolist()[:3] == [0, 1, 1] and hyp[1, 0] == 4 and hyp[2, 0] == 7 and hyp_len[3] == 0
    hyp, hyp_len = check_greedy(ops, scores, [T, 700, T + 9, -3], 0, 9)  # eos tail; lengths clamped into the buffer
    assert hyp[1, :2].tolist() == [4, 9] and hyp_len[1] == 2 and hyp[3, 0] == 9 and hyp_len[3] == 1


def test_greedy_strided_view_and_graph_replay(ops):
    big = distinct_scores(4, 260, 90, 400).cuda()
    view = big[::2, :, 5:70]
    host = view.cpu().contiguous()
    hyp = torch.zeros(2, 260, dtype=I32, device="cuda")
    hyp_len = torch.zeros(2, dtype=I32, device="cuda")
    t_len = torch.zeros(2, dtype=I32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = ops.Graph()
        g.begin()
        try:
            ops.ctc_greedy(view, t_len, 0, 64, hyp=hyp, hyp_len=hyp_len)
        finally:
            g.end()
        for tl in ([260, 100], [3, 259]):
            t_len.copy_(torch.tensor(tl, dtype=I32))
            g.launch()
            s.synchronize()
            want, _ = R.greedy(host.numpy(), tl, 0, 64)
            for b in range(2):
                assert hyp[b, :int(hyp_len[b])].tolist() == want[b] and (hyp[b, int(hyp_len[b]):] == -1).all()
        g.destroy()


# ------------------------------------------------------------------ the model on the reference fixture

@pytest.fixture(scope="module")
def asr():
    from f5e_tts_amd.ppg import ConformerPPG
    base = np.load(os.path.join(GOLD, "ppg_conformer.npz"))
    z = np.load(os.path.join(GOLD, "ctc_asr.npz"))
    sd = {k[2:]: torch.from_numpy(base[k]) for k in base.files if k.startswith("w/")}
    sd.update({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")})
    m = ConformerPPG(80, 40, 64, 4, 128, 2, 15, global_cmvn=(sd["encoder.global_cmvn.mean"], sd["encoder.global_cmvn.istd"]),
                     ctc=True)
    full = m.state_dict()
    assert {"ctc.ctc_lo.weight", "ctc.ctc_lo.bias"} <= set(sd) and set(sd) <= set(full)
    full.update(sd)
    m.load_state_dict(full)
    return m.cuda().eval(), z


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def test_ctc_logits_and_greedy_search_equal_the_reference(ops, asr):
    m, z = asr
    feats, lens = torch.from_numpy(z["feats"]).cuda(), torch.from_numpy(z["lens"]).cuda()
    eng = m.engine()
    enc, frame_lens = eng.encode(feats, lens)
    assert frame_lens.tolist() == z["enc_len"].tolist() and frame_lens.dtype == I32 and frame_lens.is_cuda
    logits = eng.ctc_logits(enc)
    want = z["encoder_out"].astype(np.float64) @ z["w/ctc.ctc_lo.weight"].astype(np.float64).T + z["w/ctc.ctc_lo.bias"]
    e_enc, e_log = rel_l2(enc, z["encoder_out"]), rel_l2(logits, want)
    print(f"encoder_out rel L2 {e_enc:.3e}, ctc logits rel L2 {e_log:.3e}")
    assert e_log < 2e-4
    hyps, scores = m.ctc_greedy_search(feats, lens)
    want_hyps = [z["hyps"][b, :n].tolist() for b, n in enumerate(z["hyp_len"])]
    print("hyps", hyps, "scores", scores.flatten().tolist(), "reference", z["scores"].flatten().tolist())
    assert hyps == want_hyps and hyps[1][-1] == m.eos == 39                      # the trailing eos of the shorter utterance
    # the values are -8.4e-4 and -5.1e-4; the reference's own fp32 log_softmax is 1.97e-4 (relative L2) away from the fp64
    # value of its stored encoder output, so this gate is met only by a result that is right to the last bits
    print("scores rel L2 to the reference %.4e" % rel_l2(scores, z["scores"]))
    assert scores.shape == (2, 1) and rel_l2(scores, z["scores"]) < 2e-4
    # the same gate against the fp64 value of the stored encoder output, which has no rounding of its own
    true = torch.log_softmax(torch.from_numpy(want), -1).max(-1).values.max(1, keepdim=True).values
    print("scores rel L2 to the fp64 value %.4e" % rel_l2(scores, true))
    assert rel_l2(scores, true) < 2e-4
    # extract() is what it was: the encoder output through `linear` and `ce.fc`
    ppg, ce_logits = m.extract(feats, lens)
    ppg2, ce2 = eng.head(enc)
    assert torch.equal(ppg, ppg2) and torch.equal(ce_logits, ce2)
    # the head trained on linear(encoder_out): another input, the same machinery
    hyps_lin, _ = m.ctc_greedy_search(feats, lens, use_linear=True)
    lin = ppg.cpu().double().numpy() @ z["w/ctc.ctc_lo.weight"].astype(np.float64).T + z["w/ctc.ctc_lo.bias"]
    assert len(hyps_lin) == 2 and lin.shape == want.shape


def test_ctc_forced_align_of_the_greedy_hypotheses(ops, asr):
    """Each utterance's own greedy hypothesis (eos tail removed) as labels: the returned path is a valid CTC path, and its
    score, re-summed in fp64 over the REFERENCE's log-probs, is within 1e-3 of the optimum ctc_ref finds on those log-probs.

    The issue adds that "the logits' own error bound, 2e-4 x RMS x T, is below" 1e-3.  For this fixture that is false:
    RMS(logits) = 4.58, T = 50 / 38, so the figure is 0.046 / 0.035.  The 1e-3 gate therefore does not follow from the 2e-4
    parity gate; it holds because paths are discrete (the optimum's own difference is 0, and 1e-3 is far below the score
    difference between two different paths of this fixture).  What DOES follow from the error of the logits is asserted
    beside it: the device path p maximises the device scores s' up to the fp32 rounding of the alpha sums, so with
    e = max |device logits - reference logits| and A = sum over frames of max |logit|,
        s(optimum) - s(p) <= 2 T e + 2 T 2^-24 A
    (per-frame log-softmax constants cancel between two paths).  Measured on an MI355X: e and both sides are printed."""
    from f5e_tts_amd import _C
    m, z = asr
    feats, lens = torch.from_numpy(z["feats"]).cuda(), torch.from_numpy(z["lens"]).cuda()
    labels = [z["hyps"][0, :z["hyp_len"][0]].tolist(), z["hyps"][1, :z["hyp_len"][1] - 1].tolist()]
    al = m.ctc_forced_align(feats, lens, labels)
    assert al.frame_lens.tolist() == z["enc_len"].tolist()
    logp = z["logp"]
    eng = m.engine()
    mine_logits = eng.ctc_logits(eng.encode(feats, lens)[0]).double().cpu().numpy()
    ref_logits = z["encoder_out"].astype(np.float64) @ z["w/ctc.ctc_lo.weight"].astype(np.float64).T + z["w/ctc.ctc_lo.bias"]
    rms = float(np.sqrt((ref_logits ** 2).mean()))
    for b, lab in enumerate(labels):
        t = int(z["enc_len"][b])
        path = al.align[b, :t].cpu().numpy()
        assert R.is_ctc_path(path, lab) and (al.align[b, t:] == -1).all()
        ts, te = al.tok_start[b, :len(lab)].cpu().numpy(), al.tok_end[b, :len(lab)].cpu().numpy()
        assert (te > ts).all() and (ts[1:] >= te[:-1]).all() and te[-1] <= t
        assert all((path[s:e] == y).all() for s, e, y in zip(ts, te, lab))
        best = R.path_score(logp[b, :t], R.align_one(logp[b, :t], lab)[0])
        mine = R.path_score(logp[b, :t], path)
        e = float(np.abs(mine_logits[b, :t] - ref_logits[b, :t]).max())
        bound = 2 * t * e + 2 * t * 2.0 ** -24 * float(np.abs(ref_logits[b, :t]).max(-1).sum())
        print(f"utterance {b}: path score {mine:.6f}, optimum {best:.6f}, max logit error {e:.2e}, bound from it {bound:.2e}; "
              f"2e-4 x RMS(logits) x T = {2e-4 * rms * t:.3f} (RMS {rms:.2f})")
        assert mine <= best + 1e-9 and best - mine <= 1e-3
        assert best - mine <= bound
    with pytest.raises(_C.F5EError, match="no CTC path"):
        m.ctc_forced_align(feats, lens, [list(range(1, 39)) + [1] * 20, [1]])
    on_dev = torch.tensor(pack(labels)).cuda()
    for bad_len in ([0, 4], [7, 4], [6, 39]):                # ids on the device, lengths on the host: still validated there
        with pytest.raises(_C.F5EError, match="no CTC path"):
            m.ctc_forced_align(feats, lens, on_dev, bad_len)
    dev = m.ctc_forced_align(feats, lens, on_dev, torch.tensor([len(r) for r in labels]).cuda())
    assert torch.equal(dev.align, al.align) and torch.equal(dev.tok_end[0], al.tok_end[0])
