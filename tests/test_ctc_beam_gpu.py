"""CTC prefix beam search on the GPU (csrc/ctc_beam.hip through ops.ctc_beam_search), the rescoring kernels (ops.mha_f32,
ops.token_logp), the attention decoder of ``ConformerPPG`` and the two decoding modes built on them, against
  * the REFERENCE's own n-best lists, decoder outputs and rescoring winners (tests/golden/ctc_beam.npz, asr_decoder_*.npz;
    the generator asserts that no stored decision is fragile), and
  * the restatements (tests/ctc_beam_ref.py, tests/asr_decoder_ref.py, pinned by the same fixtures).
N-best lists are discrete: they are compared exactly, and only on cases that satisfy the margin rule of ctc_beam_ref (the
smallest decisive gap between candidate totals is at least 20 x the fp32 / fp64 score difference), which every test asserts
as a condition on the very scores it hands to the kernel."""
import os

import numpy as np
import pytest
import torch

import ctc_beam_ref as BR
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


def planted_case(T, L, V, boost, seed, blank=0):
    """``ctc_ref.planted`` logits times boost / 4 (the recipe of make_ctc_beam_golden.py), labels never the blank."""
    labels = np.random.default_rng(seed + 50).integers(1, V, size=L)
    if blank != 0:
        labels = np.where(labels == blank, 0, labels)
    return (R.planted(T, labels, V, seed, blank=blank, boost=boost) * np.float32(boost / 4.0)).astype(np.float32)


_memo = {}


def restated(scores, K, blank=0):
    """(hyps, E) of the restatement on ``scores``, computed once per array; asserts the margin rule (a condition)."""
    key = (scores.tobytes(), scores.shape, K, blank)
    if key not in _memo:
        hyps, delta, E, same = BR.margin(scores, K, blank)
        print(f"T={scores.shape[0]} V={scores.shape[1]} K={K}: delta {delta:.3e}, E {E:.3e}")
        assert same and BR.usable(delta, E), f"the case misses the margin rule: delta {delta:.3e}, E {E:.3e}"
        _memo[key] = (hyps, E)
    return _memo[key]


def run_beam(ops, scores_dev, t_len, K, blank=0, ld_hyp=None):
    """Sentinel-filled outputs -> host arrays (hyp, hyp_len, score); the scores are left untouched."""
    B, T, V = scores_dev.shape
    ld_hyp = ld_hyp or T
    before = scores_dev.clone()
    hyp = torch.full((B, K, ld_hyp), -7, dtype=I32, device="cuda")
    n = torch.full((B, K), -7, dtype=I32, device="cuda")
    sc = torch.full((B, K), 123.0, dtype=F32, device="cuda")
    ops.ctc_beam_search(scores_dev, i32(t_len), K, blank, hyp=hyp, hyp_len=n, score=sc)
    torch.cuda.synchronize()
    assert torch.equal(scores_dev, before)
    return hyp.cpu().numpy(), n.cpu().numpy(), sc.cpu().numpy()


def check_rows(got, b, hyps, E, K, T, ld_hyp):
    hyp, n, sc = got
    want_hyp, want_n, want_sc = BR.pack(hyps, K, ld_hyp)
    assert np.array_equal(n[b], want_n), (n[b], want_n)
    assert np.array_equal(hyp[b], want_hyp), f"lists differ in {(hyp[b] != want_hyp).any(1).sum()} of {K} rows"
    err = np.abs(sc[b].astype(np.float64) - want_sc).max()
    bound = 10 * max(E, 1e-6 * T)
    print(f"   score error {err:.3e} (bound {bound:.3e}), best {want_sc[0]:.5f}")
    assert err <= bound
    assert (np.diff(sc[b]) <= 0).all()                                       # best first


def check_single(ops, scores, K, blank=0):
    hyps, E = restated(scores, K, blank)
    T = scores.shape[0]
    got = run_beam(ops, torch.from_numpy(scores)[None].cuda(), [T], K, blank)
    check_rows(got, 0, hyps, E, K, T, T)
    return got, hyps


# ------------------------------------------------------------------ f5e_ctc_beam against the reference's lists

def test_kernel_equals_the_reference_nbest_lists(ops):
    z = np.load(os.path.join(GOLD, "ctc_beam.npz"))
    seen = set()
    for i in range(int(z["n_cases"])):
        logp, K = z[f"logp_{i}"], int(z[f"beam_{i}"])
        (hyp, n, sc), _ = check_single(ops, logp, K)
        ids, lens = z[f"ids_{i}"], z[f"len_{i}"]
        assert np.array_equal(n[0], lens) and np.array_equal(hyp[0][:, :ids.shape[1]], ids)
        assert (hyp[0][:, ids.shape[1]:] == -1).all()
        seen |= {"T1"} if len(logp) == 1 else set()
        seen |= {"K16"} if K == 16 else set()
        seen |= {"T1100"} if len(logp) == 1100 else set()
    assert seen == {"T1", "K16", "T1100"}
    # the defaults: outputs and workspace allocated by the wrapper
    logp = z["logp_0"]
    hyp, n, sc = ops.ctc_beam_search(torch.from_numpy(logp)[None].cuda(), i32([len(logp)]), int(z["beam_0"]))
    assert hyp.shape == (1, 4, 40) and np.array_equal(n.cpu().numpy()[0], z["len_0"]) and sc.shape == (1, 4)


# (T, L, V, K, boost, seed, blank): V = K (the first prune keeps every class), V around one wave's stride, V of the ASR
# head, and the blank as the LAST class
EDGE_CASES = [
    (30, 6, 8, 8, 6.0, 9201, 0),
    (50, 10, 63, 10, 8.0, 9202, 0),
    (50, 10, 65, 10, 8.0, 9203, 0),
    (60, 12, 218, 10, 8.0, 9204, 0),
    (40, 7, 12, 4, 6.0, 9205, 11),
    (45, 9, 2, 2, 6.0, 9206, 0),
]


@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: f"T{c[0]}-V{c[2]}-K{c[3]}-blank{c[6]}")
def test_kernel_equals_the_restatement_at_the_class_count_edges(ops, case):
    T, L, V, K, boost, seed, blank = case
    check_single(ops, planted_case(T, L, V, boost, seed, blank), K, blank)


def test_logits_and_their_log_softmax_give_the_same_lists(ops):
    T, L, V, K, boost, seed, _ = EDGE_CASES[1]
    logits = planted_case(T, L, V, boost, seed) + np.float32(3.0) * np.random.default_rng(5).standard_normal((T, 1)).astype(np.float32)
    (h0, n0, s0), _ = check_single(ops, logits, K)
    (h1, n1, s1), _ = check_single(ops, R.log_softmax(logits), K)
    assert np.array_equal(h0, h1) and np.array_equal(n0, n1)
    assert np.abs(s0 - s1).max() < 1e-4


def test_strided_view_with_ld_above_v_and_a_batch_stride_of_two_matrices(ops):
    T, V, K = 50, 41, 10
    big = torch.randn(4, T, 64, generator=torch.Generator().manual_seed(90))
    a, b = planted_case(T, 10, V, 8.0, 9301), planted_case(T - 4, 10, V, 8.0, 9302)
    big[0, :, 5:5 + V] = torch.from_numpy(a)
    big[2, :T - 4, 5:5 + V] = torch.from_numpy(b)
    view = big.cuda()[::2, :, 5:5 + V]
    assert view.stride() == (2 * T * 64, 64, 1)
    got = run_beam(ops, view, [T, T - 4], K)
    for i, s in enumerate((a, b)):
        hyps, E = restated(s, K)
        check_rows(got, i, hyps, E, K, T, T)


def test_ragged_batch_empty_and_overlong_lengths_and_solo_equality(ops):
    T, V, K = 90, 41, 10
    a = planted_case(T, 20, V, 8.0, 9401)
    c = planted_case(57, 11, V, 8.0, 9402)
    scores = np.random.default_rng(9403).standard_normal((5, T, V)).astype(np.float32)
    scores[0], scores[3, :57], scores[4] = a, c, a
    t_len = [T, 0, T + 1, 57, T]
    got = run_beam(ops, torch.from_numpy(scores).cuda(), t_len, K)
    hyp, n, sc = got
    assert (hyp != -7).all() and (n != -7).all() and (sc != 123.0).all()         # every owned element was written
    for b, s in ((0, a), (3, c), (4, a)):
        hyps, E = restated(s, K)
        check_rows(got, b, hyps, E, K, T, T)
        solo = run_beam(ops, torch.from_numpy(scores[b:b + 1]).cuda(), t_len[b:b + 1], K)
        for x, y in zip(solo, got):                                              # bit for bit what it gets alone
            assert np.array_equal(x[0].view(np.int32), y[b].view(np.int32))
    # t_len = 0: the empty prefix alone; t_len > T: nothing
    assert n[1].tolist() == [0] + [-1] * (K - 1) and sc[1, 0] == 0.0 and (sc[1, 1:] == -np.inf).all() and (hyp[1] == -1).all()
    assert (n[2] == -1).all() and (sc[2] == -np.inf).all() and (hyp[2] == -1).all()
    neg = run_beam(ops, torch.from_numpy(scores[:1]).cuda(), [-3], K)
    assert (neg[1] == -1).all() and (neg[2] == -np.inf).all() and (neg[0] == -1).all()


def test_ld_hyp_shorter_than_a_hypothesis_reports_the_true_length(ops):
    z = np.load(os.path.join(GOLD, "ctc_beam.npz"))
    logp, K, ids, lens = z["logp_0"], int(z["beam_0"]), z["ids_0"], z["len_0"]
    assert lens.max() > 3
    flat = torch.full((K * 3 + 64,), -7, dtype=I32, device="cuda")              # the rows, then a guard zone
    hyp = flat[:K * 3].view(1, K, 3)
    _, n, _ = ops.ctc_beam_search(torch.from_numpy(logp)[None].cuda(), i32([len(logp)]), K, hyp=hyp)
    torch.cuda.synchronize()
    assert np.array_equal(n.cpu().numpy()[0], lens)
    assert np.array_equal(hyp.cpu().numpy()[0], ids[:, :3]) and (flat[K * 3:] == -7).all()


# ------------------------------------------------------------------ f5e_mha_f32 against dense fp64 softmax attention

def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def dense_attention(q, k, v, B, H, kv_len, causal, scale):
    """fp64 on the same fp32 operands: q [B*Tq, D], k / v [B*Tk, D]; a query with no visible key gives zeros."""
    D = q.shape[1]
    dk = D // H
    q, k, v = (x.double().view(B, -1, H, dk).transpose(1, 2) for x in (q, k, v))
    Tq, Tk = q.shape[2], k.shape[2]
    vis = torch.ones(B, 1, Tq, Tk, dtype=torch.bool)
    if kv_len is not None:
        vis &= (torch.arange(Tk)[None, :] < torch.as_tensor(kv_len)[:, None])[:, None, None, :]
    if causal:
        vis &= torch.tril(torch.ones(Tq, Tk, dtype=torch.bool))[None, None]
    s = (q @ k.transpose(-2, -1) * scale).masked_fill(~vis, -float("inf"))
    p = torch.softmax(s, -1).masked_fill(~vis, 0.0)
    return (p @ v).transpose(1, 2).reshape(B * Tq, D)


@pytest.mark.parametrize("dk", [16, 64])
@pytest.mark.parametrize("shape", [(1, 1), (17, 15), (33, 50), (16, 16)], ids=lambda s: f"Tq{s[0]}-Tk{s[1]}")
def test_mha_equals_dense_attention_with_ragged_key_lengths_and_padded_strides(ops, shape, dk):
    Tq, Tk = shape
    B, H = 3, 4
    D = H * dk
    g = torch.Generator().manual_seed(100 * Tq + Tk + dk)
    # every operand a column slice of a wider buffer: four different row strides, all multiples of 4 floats
    wide = [torch.randn(B * n, D + pad, generator=g) for n, pad in ((Tq, 8), (Tk, 12), (Tk, 4))]
    q, k, v = (w[:, :D] for w in wide)
    kv_len = [Tk, 0, max(1, Tk // 2)]
    want = dense_attention(q, k, v, B, H, kv_len, False, dk ** -0.5)
    out_buf = torch.full((B * Tq, D + 16), -7.0).cuda()
    out = ops.mha_f32(wide[0].cuda()[:, :D], wide[1].cuda()[:, :D], wide[2].cuda()[:, :D], H, dk ** -0.5, B=B,
                      kv_len=i32(kv_len), out=out_buf[:, :D])
    torch.cuda.synchronize()
    assert out.stride(0) == D + 16 and (out_buf[:, D:] == -7.0).all()                # the gap of the row stride is untouched
    got = out.cpu()
    assert (got[Tq:2 * Tq] == 0).all()                                             # kv_len = 0: zeros, exactly
    err = rel_l2(got, want)
    print(f"Tq={Tq} Tk={Tk} dk={dk}: rel L2 {err:.3e}")
    assert err < 1e-5
    full = ops.mha_f32(wide[0].cuda()[:, :D], wide[1].cuda()[:, :D], wide[2].cuda()[:, :D], H, dk ** -0.5, B=B)   # no kv_len
    assert rel_l2(full, dense_attention(q, k, v, B, H, None, False, dk ** -0.5)) < 1e-5


@pytest.mark.parametrize("U", [1, 16, 17, 31])
def test_mha_causal_with_key_lengths(ops, U):
    B, H, dk = 4, 4, 16
    D = H * dk
    g = torch.Generator().manual_seed(300 + U)
    q, k, v = (torch.randn(B * U, D, generator=g) for _ in range(3))
    kv_len = [U, max(1, U // 2), 1, 0]
    want = dense_attention(q, k, v, B, H, kv_len, True, 0.25)
    got = ops.mha_f32(q.cuda(), k.cuda(), v.cuda(), H, 0.25, B=B, kv_len=i32(kv_len), causal=True).cpu()
    assert (got[3 * U:] == 0).all()
    err = rel_l2(got, want)
    print(f"causal U={U}: rel L2 {err:.3e}")
    assert err < 1e-5
    # query rows at or past the key length still attend the keys below it (kv_len limits keys, not queries)
    assert U == 1 or got[U + U // 2:2 * U].abs().sum() > 0


# ------------------------------------------------------------------ f5e_token_logp / f5e_log_softmax_rows against fp64

@pytest.mark.parametrize("V", [40, 63, 65, 5000])
def test_token_logp_and_log_softmax_rows_equal_fp64(ops, V):
    rows = 37
    g = torch.Generator().manual_seed(V)
    wide = 3.0 * torch.randn(rows, V + 3, generator=g)
    logits = wide[:, :V]
    target = torch.randint(0, V, (rows,), generator=g).to(I32)
    target[5], target[11] = -1, V - 1
    want_all = torch.log_softmax(logits.double(), -1)
    want = want_all[torch.arange(rows), target.long().clamp(min=0)]
    want[5] = 0.0
    got = ops.token_logp(wide.cuda()[:, :V], target.cuda()).cpu()
    assert got[5] == 0.0
    # fp32: the max-subtracted exponent sum carries ~V ulp/2 of relative error at worst, the subtraction one ulp of |x - max|
    tol = 2.0 ** -23 * (np.log(V) + 2 + float(logits.abs().max()) * 2)
    err = float((got.double() - want).abs().max())
    print(f"V={V}: token_logp max error {err:.3e} (tolerance {tol:.3e})")
    assert err < tol
    full = ops.log_softmax_rows(wide.cuda()[:, :V]).cpu()
    assert float((full.double() - want_all).abs().max()) < tol
    inplace = logits.contiguous().cuda()
    assert torch.equal(ops.log_softmax_rows(inplace, out=inplace).cpu(), full)


# ------------------------------------------------------------------ the attention decoder and the two decoding modes

def build_asr(kind):
    from f5e_tts_amd.ppg.ppg_model import ConformerPPG
    base = np.load(os.path.join(GOLD, "ppg_conformer.npz"))
    z = np.load(os.path.join(GOLD, f"asr_decoder_{kind}.npz"))
    sd = {k[2:]: torch.from_numpy(base[k]) for k in base.files if k.startswith("w/encoder.")}
    sd.update({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")})
    conf = dict(attention_heads=4, linear_units=64, num_blocks=1)
    if kind == "bitransformer":
        conf["r_num_blocks"] = 1
    m = ConformerPPG(80, 40, 64, 4, 128, 2, 15, global_cmvn=(sd["encoder.global_cmvn.mean"], sd["encoder.global_cmvn.istd"]),
                     ctc=True, decoder=kind, decoder_conf=conf)
    full = m.state_dict()
    assert set(sd) <= set(full) and any(k.startswith("decoder.") for k in sd)
    full.update(sd)
    m.load_state_dict(full)
    return m.cuda().eval(), z


@pytest.fixture(scope="module", params=["transformer", "bitransformer"])
def asr(request):
    return build_asr(request.param)


def stored_hyps(z):
    return [tuple(int(v) for v in z["ids"][i, :n]) for i, n in enumerate(z["len"])]


def test_decoder_forward_equals_the_reference_on_the_stored_encoder_output(ops, asr):
    import asr_decoder_ref as DR
    m, z = asr
    rw = float(z["reverse_weight"])
    hyps, V = stored_hyps(z), 40
    ys, r_ys, n = DR.inputs(hyps, V - 1, V - 1)
    enc = torch.from_numpy(z["encoder_out"])
    out, r_out = m.forward_attention_decoder(ys, n, enc.cuda(), rw)
    e = rel_l2(out, z["decoder_out"])
    worst = float((out.cpu().double() - torch.from_numpy(z["decoder_out"]).double()).abs().max())
    print(f"decoder_out rel L2 {e:.3e}, max abs {worst:.3e}")
    assert e < 2e-4
    if rw > 0:
        e_r = rel_l2(r_out, z["r_decoder_out"])
        worst = max(worst, float((r_out.cpu().double() - torch.from_numpy(z["r_decoder_out"]).double()).abs().max()))
        print(f"r_decoder_out rel L2 {e_r:.3e}")
        assert e_r < 2e-4
    else:
        assert r_out.ndim == 0 and float(r_out) == 0.0
    U = ys.shape[1] - 1
    for tag, cw in (("w0", 0.0), ("w5", 0.5)):
        got = DR.rescoring_scores(hyps, z["score"].tolist(), out.cpu().numpy(), r_out.cpu().numpy() if rw > 0 else None,
                                  V - 1, cw, rw)
        want = z[f"scores_{tag}"]
        print(f"ctc_weight {cw}: device {np.round(got, 4).tolist()}\n                reference {np.round(want, 4).tolist()}")
        assert np.abs(np.asarray(got) - want).max() <= 2 * (U + 2) * worst
        assert DR.winner(got) == int(z[f"winner_{tag}"])
    # the device decoder against the fp64 restatement (no fixture in between), hypotheses of unequal lengths included
    pre = "decoder." if rw == 0 else "decoder.left_decoder."
    mine = DR.decoder_forward({k[2:]: z[k] for k in z.files if k.startswith("w/")}, pre, enc, ys, n, 4)
    assert rel_l2(out, torch.log_softmax(mine, -1)) < 2e-4


def test_end_to_end_nbest_and_rescoring_equal_the_reference(ops, asr):
    m, z = asr
    rw = float(z["reverse_weight"])
    feats, lens = torch.from_numpy(z["feats"]).cuda(), torch.from_numpy(z["lens"]).cuda()
    K, want = 10, stored_hyps(z)
    # the restatement on the DEVICE's own logits: the margin rule is a condition on them
    logits, frame_lens, _ = m._ctc_scores(feats[:1], lens[:1], False)
    host = logits[0, :int(frame_lens[0])].cpu().numpy()
    mine, delta, E, same = BR.margin(host, K)
    print(f"device logits: delta {delta:.3e}, E {E:.3e}")
    assert same and BR.usable(delta, E)
    nbest = m.ctc_prefix_beam_search(feats[:1], lens[:1], K)
    assert len(nbest) == 1 and [h for h, _ in nbest[0]] == [h for h, _ in mine] == want
    assert np.abs(np.asarray([s for _, s in nbest[0]]) - [s for _, s in mine]).max() <= 10 * max(E, 1e-6 * len(host))
    solo = []
    for tag, cw in (("w0", 0.0), ("w5", 0.5)):
        (ids, score), = m.attention_rescoring(feats[:1], lens[:1], K, ctc_weight=cw, reverse_weight=rw)
        win = int(z[f"winner_{tag}"])
        print(f"ctc_weight {cw}: winner score {score:.4f}, reference {float(z[f'scores_{tag}'][win]):.4f}")
        assert ids == want[win]
        solo.append((ids, score))
    # a batch of two, the second shorter: per utterance what the utterance gets alone
    both = m.ctc_prefix_beam_search(feats, lens, K)
    alone = m.ctc_prefix_beam_search(feats[1:], lens[1:], K)
    assert [h for h, _ in both[0]] == want and [h for h, _ in both[1]] == [h for h, _ in alone[0]]
    assert np.allclose([s for _, s in both[1]], [s for _, s in alone[0]], rtol=0, atol=1e-4)
    res = m.attention_rescoring(feats, lens, K, ctc_weight=0.5, reverse_weight=rw)
    res1, = m.attention_rescoring(feats[1:], lens[1:], K, ctc_weight=0.5, reverse_weight=rw)
    assert res[0][0] == solo[1][0] and abs(res[0][1] - solo[1][1]) < 1e-3
    assert res[1][0] == res1[0] and abs(res[1][1] - res1[1]) < 1e-3


def test_transcribe_returns_a_string_in_all_three_modes(ops, asr):
    from f5e_tts_amd.ppg.ctc_align import CTCAligner, DECODE_MODES
    m, z = asr
    table = {"<blank>": 0, **{chr(96 + i): i for i in range(1, 27)}, **{f"<{i}>": i for i in range(27, 39)}, "<sos/eos>": 39}
    al = CTCAligner(model=m, symbol_table=table, device="cuda")
    wav = 0.1 * torch.randn(1, 16000, generator=torch.Generator().manual_seed(3))
    for mode in DECODE_MODES:
        text = al.transcribe(wav, 16000, mode=mode, beam_size=4, reverse_weight=float(z["reverse_weight"]))
        assert isinstance(text, str)
    assert al.transcribe(wav, 16000) == al.transcribe(wav, 16000, mode="ctc_greedy_search")
