"""Paraformer on the GPU (csrc/paraformer.hip through f5e_tts_amd.ops and eval/paraformer.py) against the float64 restatement
tests/paraformer_ref.py (fp32 where exactness is asked).  Conventions: every test prints its measured error before it asserts,
outputs are pre-filled with 7.0 and padding holds 1e4.

Bounds of the per-kernel comparisons: 10 * sqrt(K) * 2^-24 relative L2 with K the longest chain of fp32 additions behind one
output (the rule at the top of tests/test_ecapa_gpu.py), K stated per test; the LFR front and the CIF scan have no tolerance (bit
for bit).  The whole model and the full-size layer shapes use the project's chain gate 2e-4 relative L2 (tests/test_wavlm_gpu.py)
and its row gate 1e-5 for the rows of a ragged batch against their own B = 1 runs.

Measured on an MI355X: see DESIGN 4r."""
import math

import pytest
import torch

import paraformer_ref as PR
from test_paraformer_cpu import CLIP_SAMPLES, MARGIN, SEED, tiny_cfg, tiny_clips, tiny_cmvn, tiny_reference, tiny_tokens

pytestmark = pytest.mark.gpu

GATE, ROW_GATE = 2e-4, 1e-5
F32, F64, I32 = torch.float32, torch.float64, torch.int32
PAD, FILL = 1e4, 7.0


def bound(K: int) -> float:
    return 10 * math.sqrt(K) * 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    import f5e_tts_amd.ops as ops_mod
    ops_mod.require_device()
    return ops_mod


@pytest.fixture(scope="module")
def P():
    from f5e_tts_amd.eval import paraformer
    return paraformer


def rnd(seed, *shape, lo=-1.0, hi=1.0, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=F64) * (hi - lo) + lo).to(dtype)


def i32(v):
    return torch.tensor(list(v), dtype=I32).cuda()


def bits(t):
    return t.contiguous().view(I32)


# ------------------------------------------------------------------ f5e_lfr_cmvn_f32
LFR_T = (1, 3, 4, 6, 7, 12, 13, 100)


@pytest.mark.parametrize("n_mels", [8, 80])
def test_lfr_cmvn_is_the_fp32_restatement_bit_for_bit(ops, n_mels):
    """No reductions: exact.  Every T gives another count of repeated last frames (T < the 3-frame left pad included); a ragged
    B = 2 pairs each T with the next one in one buffer whose padding holds 1e4."""
    m, n, W = 7, 6, 7 * n_mels
    shift, scale = rnd(1, W, lo=-9, hi=-7), rnd(2, W, lo=0.1, hi=0.4)
    xscale = math.sqrt(512.0)
    for i, T in enumerate(LFR_T):
        counts = (T, LFR_T[(i + 3) % len(LFR_T)])
        Tb, Tp = max(counts), -(-max(counts) // n)
        pos = rnd(3 + i, Tp + 2, W)
        fb = torch.full((2, Tb, n_mels), PAD)
        for b, c in enumerate(counts):
            fb[b, :c] = rnd(10 * i + b, c, n_mels, lo=-3, hi=12)
        out, frames = torch.full((2, Tp, W), FILL).cuda(), torch.full((2,), 77, dtype=I32).cuda()
        ops.lfr_cmvn(fb.cuda(), i32(counts), shift.cuda(), scale.cuda(), pos.cuda(), out, frames, m, n, xscale=xscale)
        torch.cuda.synchronize()
        out = out.cpu()
        for b, c in enumerate(counts):
            want = PR.lfr_cmvn(fb[b, :c], shift, scale, pos, m, n, xscale, dtype=F32)
            tp = want.shape[0]
            same = torch.equal(bits(out[b, :tp]), bits(want))
            print(f"n_mels {n_mels} T {c} (buffer {Tb}): {tp} rows, bit-identical {same}, max |diff| {float((out[b, :tp] - want).abs().max()):.1e}")
            assert same and frames[b].item() == tp == -(-c // n)
            assert (out[b, tp:] == 0).all()


def test_lfr_cmvn_counts_samples_and_refuses_bad_shapes(ops):
    fb = rnd(1, 2, 13, 8).cuda()
    out, frames = torch.full((2, 3, 56), FILL).cuda(), torch.zeros(2, dtype=I32).cuda()
    z, o = torch.zeros(56).cuda(), torch.ones(56).cuda()
    # 400 + 160 * 12 samples are 13 frames -> 3 rows; 399 samples are none
    ops.lfr_cmvn(fb, i32([400 + 160 * 12 + 159, 399]), z, o, None, out, frames, 7, 6, win=400, hop=160)
    torch.cuda.synchronize()
    assert frames.tolist() == [3, 0] and (out[1] == 0).all() and torch.equal(out[0, 2, :8], fb[0, 9])
    with pytest.raises(Exception, match="rows"):
        ops.lfr_cmvn(fb, None, z, o, None, torch.zeros(2, 2, 56).cuda(), frames, 7, 6)
    with pytest.raises(Exception, match="position table"):
        ops.lfr_cmvn(fb, None, z, o, torch.zeros(2, 56).cuda(), out, frames, 7, 6)


# ------------------------------------------------------------------ f5e_fsmn_f32
@pytest.mark.parametrize("with_addend", [False, True])
@pytest.mark.parametrize("K,shift", [(11, 0), (4, 0), (11, 2)])
def test_fsmn_against_float64(ops, K, shift, with_addend):
    """K_chain = kernel width + 2: the taps, the input, the addend.  The input is the strided v third of a [M, 3C] buffer; ragged
    lengths make taps cross a row's end and the batch boundary, where the padding holds 1e4."""
    tol = bound(K + 2)
    left = (K - 1) // 2 + shift
    worst = 0.0
    for T in (1, 5, 10, 11, 12, 70):
        for C in (32, 512):
            lens = (T, (T + 1) // 2, max(T - 3, 0))
            B = len(lens)
            w = rnd(7 * T + C, C, 1, K)
            qkv = torch.full((B, T, 3 * C), PAD)
            for b, n in enumerate(lens):
                qkv[b, :n] = rnd(100 * T + b, n, 3 * C)
            add = rnd(5 * T + 1, B, T, C) if with_addend else None
            out = torch.full((B * T, C), FILL).cuda()
            dev = qkv.cuda().view(B * T, 3 * C)
            ops.fsmn(dev[:, 2 * C:], w[:, 0].t().contiguous().cuda(), i32(lens), out, B, left,
                     addend=None if add is None else add.cuda().view(B * T, C))
            torch.cuda.synchronize()
            out = out.cpu().view(B, T, C)
            for b, n in enumerate(lens):
                rest = add[b, n:] if with_addend else torch.zeros(T - n, C)
                assert torch.equal(out[b, n:], rest), (T, C, b)
                if n == 0:
                    continue
                want = PR.fsmn(qkv[b, :n, 2 * C:].double(), w.double(), shift)
                if with_addend:
                    want = want + add[b, :n].double()
                worst = max(worst, PR.rel_l2(out[b, :n], want))
    print(f"fsmn K {K} shift {shift} addend {with_addend}: worst relative L2 {worst:.2e} (bound {tol:.2e}, K_chain {K + 2})")
    assert worst < tol


def test_fsmn_refusals(ops):
    x, w = torch.zeros(8, 32).cuda(), torch.zeros(11, 32).cuda()
    with pytest.raises(Exception, match="in-place"):
        ops.fsmn(x, w, None, x, 1, 5)
    with pytest.raises(Exception, match="left"):
        ops.fsmn(x, w, None, torch.zeros(8, 32).cuda(), 1, 11)
    with pytest.raises(Exception, match="CPU"):
        ops.fsmn(torch.zeros(8, 32), torch.zeros(11, 32), None, torch.zeros(8, 32), 1, 5)


# ------------------------------------------------------------------ f5e_cif_alpha_f32
@pytest.mark.parametrize("T", [1, 65, 700])
def test_cif_alpha_against_float64(ops, T):
    lens = (T, (T + 1) // 2, 0)
    B = len(lens)
    smooth, noise, tail = 1.0, 0.0, 0.45
    logits = torch.full((B, T), PAD)
    for b, n in enumerate(lens):
        logits[b, :n] = rnd(3 * T + b, n, lo=-4, hi=4)
    alpha, n_out = torch.full((B, T + 1), FILL).cuda(), torch.full((B,), 77, dtype=I32).cuda()
    ops.cif_alpha(logits.cuda(), i32(lens), alpha, n_out, smooth, noise, tail)
    torch.cuda.synchronize()
    alpha = alpha.cpu()
    for b, n in enumerate(lens):
        want, n_ref = PR.cif_alpha(logits[b, :n].double(), smooth, noise, tail)
        frac = float(want.sum()) % 1.0
        err = float((alpha[b, :n + 1].double() - want).abs().max())
        print(f"cif_alpha T {T} len {n}: max |diff| {err:.2e} (bound 1e-6), n {n_out[b].item()} / {n_ref}, frac {frac:.4f}")
        assert 1e-3 <= frac <= 1 - 1e-3                    # the precondition, on the reference side
        assert err <= 1e-6 and n_out[b].item() == n_ref and (alpha[b, n + 1:] == 0).all()


def test_cif_alpha_smooth_and_noise(ops):
    logits = rnd(5, 2, 40, lo=-3, hi=3)
    alpha, n_out = torch.full((2, 41), FILL).cuda(), torch.zeros(2, dtype=I32).cuda()
    ops.cif_alpha(logits.cuda(), None, alpha, n_out, 1.3, 0.4, 0.2)
    torch.cuda.synchronize()
    for b in range(2):
        want, n_ref = PR.cif_alpha(logits[b].double(), 1.3, 0.4, 0.2)
        assert float((alpha[b].cpu().double() - want).abs().max()) <= 1e-6 and n_out[b].item() == n_ref
        assert 1e-3 <= float(want.sum()) % 1.0 <= 1 - 1e-3 and (want == 0).any()


# ------------------------------------------------------------------ f5e_cif_fire_f32
def run_fire(ops, rows, T, D, seed, n_limit=None):
    """rows: one f32 alpha vector of len_b + 1 values per batch row (the tail last).  -> the device result against the literal fp32
    loop, bit for bit: fire positions, counts, every emitted value, zeros beyond."""
    B, Lc = len(rows), T + 1
    lens = [r.numel() - 1 for r in rows]
    alpha, h = torch.full((B, T + 1), PAD), torch.full((B, T, D), PAD)
    for b, r in enumerate(rows):
        alpha[b, :r.numel()] = r
        h[b, :lens[b]] = rnd(seed + b, lens[b], D, lo=-2, hi=2)
    out, count = torch.full((B, Lc, D), FILL).cuda(), torch.full((B,), 77, dtype=I32).cuda()
    scratch = torch.full((ops.cif_fire_scratch(B, T, Lc),), FILL).cuda()
    ops.cif_fire(alpha.cuda(), h.cuda().view(B * T, D), i32(lens), out, count, scratch,
                 n_limit=None if n_limit is None else i32(n_limit))
    torch.cuda.synchronize()
    out, sc = out.cpu(), scratch.cpu()
    pos = sc[B * (T + 1): B * (T + 1) + B * Lc].view(I32).view(B, Lc)
    fired = []
    for b, r in enumerate(rows):
        want, wpos, _ = PR.cif(r, h[b, :lens[b]])
        k = len(wpos)
        assert count[b].item() == k and pos[b, :k].tolist() == wpos, (b, count[b].item(), k)
        keep = k if n_limit is None else min(k, n_limit[b])
        assert torch.equal(bits(out[b, :keep]), bits(want[:keep])), (b, float((out[b, :keep] - want[:keep]).abs().max()))
        assert (out[b, keep:] == 0).all()
        fired.append(k)
    return fired


def test_cif_fire_edge_cases_bit_for_bit(ops):
    f = lambda *v: torch.tensor(v, dtype=F32)
    tail = 0.45
    # all-zero alpha: nothing fires
    assert run_fire(ops, [torch.zeros(9), torch.zeros(4), torch.zeros(1)], 8, 32, 1) == [0, 0, 0]
    # 1.0 everywhere: a fire per frame, zero remainders (the tail adds 0.45 and does not fire)
    assert run_fire(ops, [torch.cat((torch.ones(n), f(tail))) for n in (8, 5, 1)], 8, 32, 2) == [8, 5, 1]
    # 0.5 + 0.5: fires at exactly the threshold; on the last valid frame for an even length
    assert run_fire(ops, [torch.cat((torch.full((n,), 0.5), f(tail))) for n in (8, 5, 2)], 8, 4, 3) == [4, 2, 1]
    # a carry of 0.6 into the tail fires it; 0.3 does not; 0.55 is the edge (0.55 + 0.45 in fp32)
    got = run_fire(ops, [f(0.7, 0.9, tail), f(0.7, 0.6, tail), f(0.55, tail)], 2, 32, 4)
    want = [len(PR.cif(r, torch.zeros(r.numel() - 1, 1))[1]) for r in (f(0.7, 0.9, tail), f(0.7, 0.6, tail), f(0.55, tail))]
    print(f"tail cases: fires {got}")
    assert got == want and got[0] == 2 and got[1] == 1
    # the limit of the predictor's own count cuts the emitted rows
    assert run_fire(ops, [torch.cat((torch.ones(n), f(tail))) for n in (8, 5, 1)], 8, 32, 5, n_limit=[3, 9, 0]) == [8, 5, 1]


@pytest.mark.parametrize("D", [4, 32, 512])
@pytest.mark.parametrize("T", [1, 2, 65, 700])
def test_cif_fire_random_alpha_bit_for_bit(ops, T, D):
    lens = (T, (T + 1) // 2, max(T - 1, 0) if T > 2 else 0)
    rows = [torch.cat((rnd(31 * T + D + b, n, lo=0.0, hi=1.0), torch.tensor([0.45]))) for b, n in enumerate(lens)]
    fired = run_fire(ops, rows, T, D, 1000 + T + D)
    print(f"cif_fire T {T} D {D} lens {lens}: fires {fired}, bit-identical")
    assert fired[0] >= (T >= 65) * T // 4


# ------------------------------------------------------------------ f5e_nar_pick
@pytest.mark.parametrize("V", [50, 8404])
def test_nar_pick(ops, V):
    """K = V: the sum of V exponentials behind each log-probability."""
    B, L, ld = 4, 6, V + 4
    n = [6, 0, 3, 4]
    buf = torch.full((B * L, ld), PAD)
    logits = rnd(V, B * L, V, lo=-6, hi=6)
    logits[2, 17], logits[2, 40] = 9.0, 9.0                 # a tie: the lowest index wins
    logits[4, 5] = 8.0
    for k, sid in enumerate((0, 1, 2, 1)):                  # utterance 3: only special ids
        logits[3 * L + k, sid] = 9.5
    logits[0, 2] = 9.25                                     # an eos among real tokens
    buf[:, :V] = logits
    for b in range(B):
        buf[b * L + n[b]: (b + 1) * L] = PAD                # rows beyond n hold padding
    dev = buf.cuda()
    arg, lp = torch.full((B * L,), 77, dtype=I32).cuda(), torch.full((B * L,), FILL).cuda()
    ids, length, score = torch.full((B, L), 77, dtype=I32).cuda(), torch.full((B,), 77, dtype=I32).cuda(), torch.full((B,), FILL).cuda()
    ops.nar_pick(dev[:, :V], i32(n), B, arg, lp, ids, length, score, sos=1, eos=2, blank=0, pad=-1)
    torch.cuda.synchronize()
    logp = torch.log_softmax(logits.double(), -1)
    worst = 0.0
    for b in range(B):
        rows = logp[b * L: b * L + n[b]]
        best = rows.max(-1).values if n[b] else torch.zeros(0, dtype=F64)
        want_arg = torch.where(rows == best[:, None], torch.arange(V)[None], V).min(-1).values     # the lowest index on ties
        keep = [int(v) for v in want_arg if int(v) not in (0, 1, 2)]
        assert arg[b * L: b * L + n[b]].tolist() == want_arg.tolist() and (arg[b * L + n[b]: (b + 1) * L] == -1).all()
        assert ids[b].tolist() == keep + [-1] * (L - len(keep)) and length[b].item() == len(keep)
        want = float(best.sum())
        if n[b]:
            worst = max(worst, abs(score[b].item() - want) / abs(want), PR.rel_l2(lp[b * L: b * L + n[b]].cpu(), best))
        else:
            assert score[b].item() == 0.0
    print(f"nar_pick V {V}: worst relative error of score / log-probabilities {worst:.2e} (bound {bound(V):.2e}, K = V)")
    assert worst < bound(V)
    assert arg[2].item() == 17 and length.tolist()[3] == 0 and length.tolist()[1] == 0 and 2 not in ids[0].tolist()


# ------------------------------------------------------------------ the whole model
@pytest.fixture(scope="module")
def tiny(P):
    cfg = tiny_cfg()
    model = P.Paraformer(cfg, cmvn=tiny_cmvn(cfg), tokens=tiny_tokens(cfg))
    model.load_funasr_state(P.seeded_state_dict(cfg, SEED))
    return model.cuda().eval()


def batch_of(clips):
    wav = torch.full((len(clips), max(c.numel() for c in clips)), PAD)
    for b, c in enumerate(clips):
        wav[b, :c.numel()] = c
    return wav.cuda(), i32([c.numel() for c in clips])


def stages(model, wav, lens):
    """Every stage of one pass as CPU tensors: feats, frames, enc, embeds, n, alpha, and the log-probabilities."""
    feats, frames, enc, embeds, n, alpha = model.encode_predict(wav, lens)
    L = max(int(n.max()), 1)
    logp = model.decode(enc, frames, embeds[:, :L], n)
    torch.cuda.synchronize()
    return dict(feats=feats.cpu(), frames=frames.tolist(), enc=enc.cpu(), embeds=embeds.cpu(), n=n.tolist(), alpha=alpha.cpu(),
                logp=logp.cpu())


def test_whole_model_ragged_batch_against_float64(tiny):
    ref = tiny_reference()
    for r in ref:                                                                  # the two margins, on the reference, for all clips
        assert r["fire_margin"] >= MARGIN and MARGIN <= r["frac"] <= 1 - MARGIN and r["fires"] == r["n"]
    assert max(r["n"] for r in ref) >= 3
    wav, lens = batch_of(tiny_clips())
    got = stages(tiny, wav, lens)
    tokens, length, score = tiny.generate(wav, lens)
    torch.cuda.synchronize()
    worst = 0.0
    for b, r in enumerate(ref):
        tp, n = r["feats"].shape[0], r["n"]
        assert got["frames"][b] == tp and got["n"][b] == n
        errs = dict(feats=PR.rel_l2(got["feats"][b, :tp], r["feats"]), enc=PR.rel_l2(got["enc"][b, :tp], r["enc"]),
                    alpha=PR.rel_l2(got["alpha"][b, :tp + 1], r["alpha"]), embeds=PR.rel_l2(got["embeds"][b, :n], r["embeds"]),
                    logp=PR.rel_l2(got["logp"][b, :n], r["logp"]))
        ids = [int(v) for v in tokens[b].tolist() if v >= 0]
        text, want_text = tiny.decode_ids(ids), PR.join_tokens([tiny_tokens(tiny.cfg)[i] for i in r["ids"]])
        print(f"clip {CLIP_SAMPLES[b]}: T' {tp}, n {n}, " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) +
              f" (gate {GATE:.0e}); ids equal {ids == r['ids']}, score {score[b].item():.4f} / {r['score']:.4f}, text {text!r}")
        assert (got["feats"][b, tp:] == 0).all() and (got["enc"][b, tp:] == 0).all() and (got["embeds"][b, n:] == 0).all()
        assert max(errs.values()) < GATE
        assert ids == r["ids"] and length[b].item() == len(ids) and text == want_text
        assert abs(score[b].item() - r["score"]) <= GATE * abs(r["score"])
        worst = max(worst, *errs.values())
    print(f"whole model: worst relative L2 {worst:.2e}")


def test_rows_of_a_ragged_batch_equal_their_own_b1_runs(tiny):
    clips = tiny_clips()
    wav, lens = batch_of(clips)
    got = stages(tiny, wav, lens)
    for b, c in enumerate(clips):
        one = stages(tiny, *batch_of([c]))
        tp, n = one["frames"][0], one["n"][0]
        assert got["frames"][b] == tp and got["n"][b] == n
        errs = [PR.rel_l2(got[k][b, :m], one[k][0, :m]) for k, m in (("feats", tp), ("enc", tp), ("alpha", tp + 1), ("embeds", n),
                                                                     ("logp", n))]
        print(f"row {b} against its B = 1 run: " + " ".join(f"{e:.2e}" for e in errs) + f" (gate {ROW_GATE:.0e})")
        assert max(errs) < ROW_GATE


def test_encode_predict_allocates_nothing_and_replays_from_a_graph(tiny):
    wav, lens = batch_of(tiny_clips())
    B, S = wav.shape
    ws = torch.empty(tiny.workspace_bytes(B, S), dtype=torch.uint8).cuda()
    eager = [t.clone() for t in tiny.encode_predict(wav, lens)]            # folds the weights
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    outs = tiny.encode_predict(wav, lens, workspace=ws)
    assert torch.cuda.memory_allocated() == before
    assert all(torch.equal(a, b) for a, b in zip(outs, eager))
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    ws.zero_()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        outs = tiny.encode_predict(wav, lens, workspace=ws)
    ws.zero_()
    graph.replay()
    torch.cuda.synchronize()
    same = [torch.equal(a, b) for a, b in zip(outs, eager)]
    print(f"graph replay of front-end + encoder + predictor equals the eager run bit for bit: {same}")
    assert all(same)
    with pytest.raises(Exception, match="workspace"):
        tiny.encode_predict(wav, lens, workspace=ws[:1024])
    with pytest.raises(Exception, match="workspace"):
        tiny.generate(wav, lens, workspace=ws[: ws.numel() // 2])
    tokens, _, _ = tiny.generate(wav, lens, workspace=ws)
    assert torch.equal(tokens, tiny.generate(wav, lens)[0])


def test_recognizer_transcribes_a_directory_written_here(tiny, P, tmp_path):
    from test_paraformer_cpu import write_dir
    rec = P.ParaformerRecognizer(write_dir(tmp_path, P.seeded_state_dict(tiny.cfg, SEED)))
    ref = tiny_reference()
    texts = rec.transcribe([c for c in tiny_clips()], 16000)
    want = [PR.join_tokens([tiny_tokens(tiny.cfg)[i] for i in r["ids"]]) for r in ref]
    print(f"transcripts: {texts}")
    assert texts == want and rec.transcribe(tiny_clips()[1], 16000, mode="ctc_greedy_search", beam_size=10) == want[1]


# ------------------------------------------------------------------ full-size layer shapes
def test_full_size_layer_shapes(P):
    """D 512, the 560-wide first layer and one 512-wide layer, the predictor, one decoder layer + decoders3, V 8404, T' = 170 (and a
    ragged second row): width-dependent indexing.  Seeded weights; the chain gate."""
    cfg = P.ParaformerConfig(enc_layers=2, dec_layers=1)
    sd = P.seeded_state_dict(cfg, SEED + 7)
    model = P.Paraformer(cfg)
    model.load_funasr_state(sd)
    model = model.cuda().eval()
    lens = (170, 101)
    feats = torch.zeros(2, 170, 560)
    for b, n in enumerate(lens):
        feats[b, :n] = rnd(50 + b, n, 560, lo=-3, hi=3)
    frames = i32(lens)
    enc = model.encode(feats.cuda(), frames)
    embeds, n, alpha = model.predict(enc, frames)
    L = int(n.max())
    logp = model.decode(enc, frames, embeds[:, :L], n)
    torch.cuda.synchronize()
    sd = PR.sd64(sd)
    for b, t in enumerate(lens):
        want_enc = PR.encoder(sd, cfg, feats[b, :t].double())
        want_alpha, want_n = PR.predictor_alpha(sd, cfg, want_enc)
        want_frames, _, seen = PR.cif(want_alpha, want_enc)
        frac = float(want_alpha.sum()) % 1.0
        assert min(abs(v - 1.0) for v in seen) >= 1e-4 and 1e-3 <= frac <= 1 - 1e-3       # the comparison's precondition
        want_logp = PR.decoder(sd, cfg, want_frames[:want_n], want_enc)
        errs = dict(enc=PR.rel_l2(enc[b, :t].cpu(), want_enc), alpha=PR.rel_l2(alpha[b, :t + 1].cpu(), want_alpha),
                    embeds=PR.rel_l2(embeds[b, :want_n].cpu(), want_frames[:want_n]), logp=PR.rel_l2(logp[b, :want_n].cpu(), want_logp))
        print(f"full-size shapes, row {b} (T' {t}, n {want_n}): " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (gate {GATE:.0e})")
        assert n[b].item() == want_n and max(errs.values()) < GATE
