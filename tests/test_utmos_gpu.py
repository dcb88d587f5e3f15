"""UTMOS predictor on the GPU (csrc/utmos.hip, eval/wav2vec2.py, eval/utmos.py) against
  * the fixture made from ``transformers.Wav2Vec2Model`` and ``torch.nn.LSTM`` (tests/golden/utmos.npz): last hidden state, BiLSTM
    output and per-frame scores of every case, relative L2 < 2e-4, the project's gate for fp32 chains against reference fixtures
    (tests/test_wavlm_gpu.py); the utterance score within 2e-4 * max(1, |want|);
  * the CPU restatement (tests/utmos_ref.py, pinned by the same fixture) in float64, kernel by kernel, on the smallest shapes at
    which each can go wrong.  Bound: 10 * sqrt(K) * 2^-24 relative L2 with K the longest chain of fp32 additions behind one output
    of that kernel (the rule at the top of tests/test_ecapa_gpu.py).  conv0_gn: K = max(10, T0) (10 taps, statistics over T0
    frames); lstm: K = T (H + 4) (a dot product of H terms and the four-term cell update per step, T steps); score_mean: K = F for
    a frame, F + T for the mean;
  * its own B = 1 runs for the rows of a ragged batch (1e-5, the figure tests/test_wavlm_gpu.py uses for the same property).

Every test prints its measured error before it asserts.  Output buffers are pre-filled with 7.0, padding holds 1e4.

Measured on an MI355X (relative L2): fixture hidden state 6.9e-7 .. 8.8e-7, BiLSTM output 5.5e-7 .. 9.1e-7, frame
scores 1.7e-7 .. 5.4e-7, the three scores equal the fixture's; per kernel conv0_gn 3.8e-8 .. 4.5e-7, lstm 7.9e-8 .. 1.05e-7 (CPU fp32
torch.nn.LSTM on the same inputs: 8.0e-8 .. 1.19e-7), score_mean 3.8e-8 .. 1.8e-7; full-size configuration 1.5e-6 (hidden state),
1.3e-6 (BiLSTM), 2.4e-6 (frame scores); the rows of a ragged batch equal their own B = 1 run bit for bit; a graph replay of
``predict`` equals the eager result bit for bit."""
import json
import math

import numpy as np
import pytest
import torch

import utmos_ref as UR
from test_utmos_cpu import CASES, FRAMES, gold, tiny_cfg, tiny_model

pytestmark = pytest.mark.gpu

GATE, ROW_GATE = 2e-4, 1e-5
F64, I32 = torch.float64, torch.int32


def tol(K):
    return 10.0 * math.sqrt(K) * 2.0 ** -24


def rnd(*shape, seed=0, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def dev32(t):
    return t.to(torch.float32).cuda().contiguous()


def f64(t):
    return dev32(t).cpu().double()          # the float32 values the device sees, in float64


def check(name, got, want, bound):
    err = UR.rel_l2(got.detach().cpu(), want)
    print(f"{name}: rel L2 {err:.3e} (bound {bound:.3e})")
    assert torch.isfinite(got).all() and err < bound, name


@pytest.fixture(scope="module")
def ops():
    import f5e_tts_amd.ops as ops_mod
    ops_mod.require_device()
    return ops_mod


@pytest.fixture(scope="module")
def model(ops):
    return tiny_model().cuda()


@pytest.fixture(scope="module")
def singles(model):
    """``parts`` of every fixture case alone (B = 1), computed once and shared."""
    z, _ = gold()
    return {S: {k: v.clone() for k, v in model.parts(torch.from_numpy(z[f"wav_{S}"]).cuda()[None]).items()} for S in CASES}


# ---- kernel by kernel against the float64 restatement ----

@pytest.mark.parametrize("C", (32, 512))
def test_conv0_group_norm_gelu(ops, C):
    cfg = tiny_cfg()
    w, g, beta, bias = rnd(C, 1, 10, seed=C, scale=0.3), 1 + 0.1 * rnd(C, seed=1), 0.1 * rnd(C, seed=2), 0.2 * rnd(C, seed=9)
    for S in (10, 14, 15, 400, 1290, 4007):              # T0 = 1, 1, 2, 79, 257 (a second chunk of one frame), 800 (four chunks)
        lens = [S, S - 137] if S - 137 >= 10 else [S]
        B, T0 = len(lens), (S - 10) // 5 + 1
        wav = 0.5 * rnd(B, S, seed=S) + 0.2
        x = dev32(wav)
        for b, n in enumerate(lens):
            x[b, n:] = 1e4
        T = UR.frame_counts(S, cfg)[-1]
        want_frames = [UR.frame_counts(n, cfg)[-1] for n in lens]
        for use_bias in (False, True):
            out = torch.full((B, T0 + 1, C), 7.0).cuda()
            frames, mask = torch.full((B,), -1, dtype=I32).cuda(), (torch.full((B, T), 7.0).cuda() if T else None)
            partials = torch.full((ops.w2v_conv0_gn_partials(B, S, C),), float("nan")).cuda()
            ops.w2v_conv0_gn(x, dev32(w[:, 0]), dev32(bias) if use_bias else None, dev32(g), dev32(beta),
                             torch.tensor(lens, dtype=I32).cuda(), out, partials, frames, mask, cfg.conv_kernel, cfg.conv_stride)
            want = UR.conv0_gn(f64(wav), f64(w), f64(bias) if use_bias else None, f64(g), f64(beta), lens)
            assert want.shape == (B, T0, C) and float((out[:, T0] - 7.0).abs().max()) == 0.0      # the pad frame is not touched
            for b, n in enumerate(lens):
                assert float(out[b, (n - 10) // 5 + 1:T0].abs().max() if (n - 10) // 5 + 1 < T0 else 0.0) == 0.0
            assert frames.tolist() == want_frames
            if T:
                assert torch.equal(mask.cpu(), (torch.arange(T)[None] < torch.tensor(want_frames)[:, None]).float())
            check(f"conv0_gn C={C} S={S} bias={use_bias}", out[:, :T0], want, tol(max(10, T0)))
        if T0 == 1:          # one frame: the normalised term vanishes EXACTLY, whatever the wave: GELU(beta), the bits of a silent row
            silent = torch.full((1, 2, C), 7.0).cuda()
            ops.w2v_conv0_gn(torch.zeros(1, S).cuda(), dev32(w[:, 0]), None, dev32(g), dev32(beta), None, silent, partials)
            same = torch.equal(out[0, 0], silent[0, 0])
            print(f"conv0_gn C={C} S={S}: one frame equals GELU(beta) bit for bit: {same}")
            assert same
            check(f"conv0_gn C={C} S={S} GELU(beta)", silent[0, 0], UR.gelu(f64(beta)), tol(10))


@pytest.mark.parametrize("T", (1, 2, 17, 130))
@pytest.mark.parametrize("ND", (1, 2))
@pytest.mark.parametrize("H", (64, 512))
def test_lstm_recurrence(ops, H, ND, T):
    B, lens = 3, [T, max(1, T - 5), 1]
    xg, w_hh = rnd(B, T, ND * 4 * H, seed=H + T, scale=H ** -0.5), rnd(ND, 4 * H, H, seed=H + ND, scale=H ** -0.5)
    xd = dev32(xg)
    for b, n in enumerate(lens):
        xd[b, n:] = 1e4                                                        # padding rows of xg are never read
    packed = ops.pack_lstm_weight(w_hh)
    guarded = torch.full((packed.numel() + 8,), float("nan"))
    guarded[4:-4] = packed.reshape(-1)                                         # NaN on both sides: an index off by one shows
    wp = guarded.cuda()[4:-4].view(packed.shape)
    out, cell = torch.full((B, T, ND * H), 7.0).cuda(), torch.full((ND, B, H), float("nan")).cuda()
    ops.lstm_f32(xd.view(B * T, -1), wp, torch.tensor(lens, dtype=I32).cuda(), out, cell)
    want = UR.lstm_recurrence(f64(xg), f64(w_hh), lens)
    for b, n in enumerate(lens):
        assert float(out[b, n:].abs().max() if n < T else 0.0) == 0.0          # rows t >= len are zero
    # the same recurrence by torch.nn.LSTM in fp32 on the CPU, as a yardstick for the device's error (printed, not asserted)
    ref = torch.nn.LSTM(ND * 4 * H, H, batch_first=True, bidirectional=ND == 2)
    with torch.no_grad():
        for d, sfx in enumerate(("", "_reverse")[:ND]):
            sel = torch.zeros(4 * H, ND * 4 * H)
            sel[:, d * 4 * H:(d + 1) * 4 * H] = torch.eye(4 * H)               # W_ih picks this direction's columns of xg, exactly
            getattr(ref, "weight_ih_l0" + sfx).copy_(sel)
            getattr(ref, "weight_hh_l0" + sfx).copy_(w_hh[d].float())
            getattr(ref, "bias_ih_l0" + sfx).zero_(), getattr(ref, "bias_hh_l0" + sfx).zero_()
        pk = torch.nn.utils.rnn.pack_padded_sequence(xg.float(), lens, batch_first=True)
        cpu, _ = torch.nn.utils.rnn.pad_packed_sequence(ref(pk)[0], batch_first=True, total_length=T)
    print(f"lstm H={H} ND={ND} T={T}: CPU fp32 torch.nn.LSTM rel L2 {UR.rel_l2(cpu, want):.3e}")
    check(f"lstm H={H} ND={ND} T={T}", out, want, tol(T * (H + 4)))


@pytest.mark.parametrize("B", (1, 2, 6, 16))
def test_lstm_without_lengths_and_other_batch_sizes(ops, B):
    """The kernel takes 1, 2 or 4 rows per pass over its weights: one row, two rows, and more rows than one pass (6 = 4 + 2 with
    two idle slots, 16 = the limit)."""
    H, T = 128, 9
    xg, w_hh = rnd(B, T, 8 * H, seed=B, scale=H ** -0.5), rnd(2, 4 * H, H, seed=2, scale=H ** -0.5)
    out = torch.full((B, T, 2 * H), 7.0).cuda()
    ops.lstm_f32(dev32(xg).view(B * T, -1), ops.pack_lstm_weight(w_hh).cuda(), None, out, torch.empty(2 * B * H).cuda())
    check(f"lstm H=128 B={B} without lengths", out, UR.lstm_recurrence(f64(xg), f64(w_hh)), tol(T * (H + 4)))


@pytest.mark.parametrize("T", (1, 17))
@pytest.mark.parametrize("F", (64, 2048))
def test_score_mean(ops, F, T):
    B, frames = 3, [T, max(1, T - 5), 1]
    hid, w2, b2 = rnd(B, T, F, seed=F + T), rnd(F, seed=3, scale=F ** -0.5), rnd(1, seed=4)
    hd = dev32(hid)
    for b, n in enumerate(frames):
        hd[b, n:] = 1e4
    out, fs = torch.full((B,), 7.0).cuda(), torch.full((B, T), 7.0).cuda()
    ops.score_mean(hd.view(B * T, F), dev32(w2), dev32(b2), torch.tensor(frames, dtype=I32).cuda(), out, B, scale=2.0, offset=3.0,
                   frame_scores=fs)
    keep = (torch.arange(T)[None] < torch.tensor(frames)[:, None]).double()
    want_fs = (f64(hid) @ f64(w2) + f64(b2)) * keep
    want = want_fs.sum(1) / torch.tensor(frames).double() * 2.0 + 3.0
    assert float((fs.cpu() * (1 - keep)).abs().max()) == 0.0
    check(f"score_mean F={F} T={T} frame scores", fs, want_fs, tol(F))
    check(f"score_mean F={F} T={T} mean", out, want, tol(F + T))
    again = torch.full((B,), 7.0).cuda()
    ops.score_mean(hd.view(B * T, F), dev32(w2), dev32(b2), torch.tensor(frames, dtype=I32).cuda(), again, B, scale=2.0, offset=3.0)
    assert torch.equal(again, out)                                             # the per-frame output is optional


# ---- the module ----

@pytest.mark.parametrize("S", CASES)
def test_fixture(singles, S):
    z, _ = gold()
    r = singles[S]
    assert r["frames"].tolist() == [FRAMES[S]]
    check(f"S={S} last hidden state", r["hidden"][0], z[f"hidden_{S}"], GATE)
    check(f"S={S} BiLSTM output", r["blstm"][0], z[f"blstm_{S}"], GATE)
    check(f"S={S} frame scores", r["frame_scores"][0], z[f"frame_{S}"], GATE)
    got, want = float(r["scores"][0]), float(z[f"score_{S}"])
    print(f"S={S} score {got:.6f} against {want:.6f}: |diff| {abs(got - want):.3e} (bound {GATE * max(1, abs(want)):.3e})")
    assert abs(got - want) < GATE * max(1.0, abs(want))


def test_ragged_rows_equal_their_own_batch_of_one(model, singles):
    z, _ = gold()
    lens = [40000, 23457, 400]
    wav = torch.full((3, 40000), 1e4)
    for b, n in enumerate(lens):
        wav[b, :n] = torch.from_numpy(z[f"wav_{n}"])
    r = model.parts(wav.cuda(), torch.tensor(lens, dtype=I32).cuda())
    assert r["frames"].tolist() == [124, 73, 1] and all(torch.isfinite(r[k]).all() for k in ("hidden", "blstm", "frame_scores", "scores"))
    for b, n in enumerate(lens):
        one, f = singles[n], FRAMES[n]
        for key in ("hidden", "blstm", "frame_scores"):
            same = torch.equal(r[key][b, :f], one[key][0])
            err = UR.rel_l2(r[key][b, :f].cpu(), one[key][0].cpu())
            print(f"row {b} ({n} samples) {key} against its B = 1 run: rel L2 {err:.3e}, bit-identical: {same}")
            assert err < ROW_GATE
        assert float(r["blstm"][b, f:].abs().max() if f < 124 else 0.0) == 0.0 == float(r["frame_scores"][b, f:].abs().max() if f < 124 else 0.0)
        d = abs(float(r["scores"][b]) - float(one["scores"][0]))
        print(f"row {b} score against its B = 1 run: |diff| {d:.3e}, bit-identical: {d == 0.0}")
        assert d < ROW_GATE * max(1.0, abs(float(one["scores"][0])))


def test_predict_allocates_nothing_and_replays_from_a_graph(model):
    z, _ = gold()
    wav = torch.zeros(2, 23457)
    wav[0], wav[1, :20000] = torch.from_numpy(z["wav_23457"]), torch.from_numpy(z["wav_23457"][:20000])
    wav, lens = wav.cuda(), torch.tensor([23457, 20000], dtype=I32).cuda()
    ws = torch.empty(model.workspace_bytes(2, 23457), dtype=torch.uint8).cuda()
    out, fs = torch.empty(2).cuda(), torch.empty(2, 73).cuda()
    eager_fs = torch.empty(2, 73).cuda()
    eager = model.predict(wav, lens, frame_scores=eager_fs).clone()             # folds the weights
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    got = model.predict(wav, lens, out=out, workspace=ws, frame_scores=fs)
    assert torch.cuda.memory_allocated() == before and got.data_ptr() == out.data_ptr()
    assert torch.equal(out, eager) and torch.equal(fs, eager_fs)
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    out.zero_(), fs.zero_()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        model.predict(wav, lens, out=out, workspace=ws, frame_scores=fs)
    out.zero_(), fs.zero_()
    graph.replay()
    torch.cuda.synchronize()
    same = torch.equal(out, eager) and torch.equal(fs, eager_fs)
    print(f"graph replay equals the eager result bit for bit: {same}")
    assert same


def test_full_size_configuration(ops):
    """utmos22_strong's sizes (wav2vec2-base, BiLSTM 1024 -> 2 x 512, 1024 -> 2048 -> 1), seeded synthetic weights, one second of
    audio (49 frames) against the float64 restatement.  Measured on an MI355X: see DESIGN 4p."""
    from f5e_tts_amd.eval.utmos import UTMOS22Strong
    torch.manual_seed(4243)
    big = UTMOS22Strong()
    wav = (0.1 * torch.randn(1, 16000) + 0.2 * torch.sin(torch.arange(16000) * (2 * math.pi * 180 / 16000)))
    sd = {k: v.detach().double() for k, v in big.state_dict().items()}
    want = UR.predict(sd, big.wav2vec2.cfg, wav.double())
    del sd
    r = big.cuda().parts(wav.cuda())
    assert want["frames"] == [49] == r["frames"].tolist() and r["hidden"].shape == (1, 49, 768) and r["blstm"].shape == (1, 49, 1024)
    print(f"full size: frame-score std {float(want['frame_scores'].std()):.3e}, score {float(want['scores'][0]):.5f}")
    for key in ("hidden", "blstm", "frame_scores"):
        check(f"full size {key}", r[key], want[key], GATE)
    d = abs(float(r["scores"][0]) - float(want["scores"][0]))
    print(f"full size score: |diff| {d:.3e}")
    assert d < GATE * max(1.0, abs(float(want["scores"][0])))


def test_run_utmos_on_files(model, tmp_path):
    from f5e_tts_amd.eval import eval_utmos
    from f5e_tts_amd.infer.utils_infer import load_wav, save_wav
    z, _ = gold()
    save_wav(str(tmp_path / "a.wav"), z["wav_23457"], 16000)
    save_wav(str(tmp_path / "b.wav"), z["wav_40000"][:30000], 24000)
    mean = eval_utmos.run_utmos(str(tmp_path), "wav", model, "cuda")
    lines = (tmp_path / "_utmos_results.jsonl").read_text().split("\n")
    rows = [json.loads(l) for l in lines[:2]]
    assert [r["wav"] for r in rows] == ["a", "b"]
    for r, sr in zip(rows, (16000, 24000)):
        wav, got_sr = load_wav(str(tmp_path / (r["wav"] + ".wav")))
        want = float(model(wav.mean(0).cuda()[None], got_sr)[0])
        print(f"{r['wav']}.wav at {sr} Hz: jsonl {r['utmos']:.6f}, forward {want:.6f}")
        assert got_sr == sr and abs(r["utmos"] - want) < 1e-6
    assert lines[2] == "" and lines[3] == f"UTMOS: {mean:.4f}" and abs(mean - (rows[0]["utmos"] + rows[1]["utmos"]) / 2) < 1e-9
