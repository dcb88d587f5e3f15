"""WavLM upstream on the GPU (csrc/wavlm.hip, f5e_relbias_attn_f32, eval/wavlm.py) against
  * the fixture made from ``transformers.WavLMModel`` (tests/golden/wavlm.npz): every hidden state of every case, relative
    L2 < 2e-4, the project's gate for fp32 chains against reference fixtures (tests/test_ppg_gpu.py, tests/test_ecapa_gpu.py);
  * the CPU restatement (tests/wavlm_ref.py, pinned by the same fixture) in float64, kernel by kernel, on the smallest shapes at
    which each can go wrong.  Bound: 10 * sqrt(K) * 2^-24 relative L2 with K the longest chain of fp32 additions behind one
    output of that kernel -- one rounding of 2^-24 per operation grows like sqrt(K) as a root mean square, which is what a
    relative L2 measures; ten times that (the rule at the top of tests/test_ecapa_gpu.py);
  * its own B = 1 runs for the rows of a ragged batch (1e-5, the figure tests/test_ecapa_gpu.py uses for the same property).

Every test prints its measured error before it asserts.

Measured on an MI355X (relative L2): fixture hidden states 7.7e-7 .. 9.4e-7; per kernel wav_norm 5e-8, conv0 1.3e-7,
strided-view conv + LayerNorm + GELU at most 8e-7, posconv 3.1e-7, gate 3.3e-8, relbias_attn 3.7e-7; full-size configuration
2.3e-6 (hidden state 0) falling to 1.6e-6 (hidden state 24); the rows of a ragged batch equal their own B = 1 run bit for bit;
a graph replay of ``extract`` equals the eager result bit for bit."""
import math

import numpy as np
import pytest
import torch

import wavlm_ref as WR
from test_wavlm_cpu import CASES, gold, tiny_cfg, tiny_model

pytestmark = pytest.mark.gpu

GATE, ROW_GATE = 2e-4, 1e-5
F64, I32 = torch.float64, torch.int32


def tol(K):
    return 10.0 * math.sqrt(K) * 2.0 ** -24


def rnd(*shape, seed=0, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def dev32(t):
    return t.to(torch.float32).cuda().contiguous()


def check(name, got, want, bound):
    err = WR.rel_l2(got.detach().cpu(), want)
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


# ---- end to end against the fixture ----

@pytest.mark.parametrize("S", CASES)
def test_fixture_hidden_states(model, S):
    z, _ = gold()
    hs, frames = model.extract(torch.from_numpy(z[f"wav_{S}"]).cuda()[None])
    want = z[f"hs_{S}"]
    assert hs.shape == (4, 1) + want.shape[1:] and frames.tolist() == [want.shape[1]]
    for l in range(4):
        check(f"S={S} hidden state {l}", hs[l, 0], want[l], GATE)


def test_fixture_padded_pair(model):
    z, _ = gold()
    wav = torch.zeros(2, 40000)
    wav[0], wav[1, :23457] = torch.from_numpy(z["wav_40000"]), torch.from_numpy(z["wav_23457"])
    wav[1, 23457:] = 1e4                                     # whatever the padding holds
    hs, frames = model.extract(wav.cuda(), torch.tensor([40000, 23457], dtype=I32).cuda())
    assert frames.tolist() == [124, 73] and torch.isfinite(hs).all()
    for row in range(2):
        for l in range(4):
            check(f"pair row {row} hidden state {l}", hs[l, row, :int(frames[row])], z[f"hs_pair_{row}"][l], GATE)


# ---- kernel by kernel against the float64 restatement ----

@pytest.mark.parametrize("S", (400, 40001))
def test_wav_norm(ops, S):
    cfg = tiny_cfg()
    lens = [S, S - 137]
    wav = rnd(2, S, seed=S) * 0.1 + 0.05
    x = wav.clone()
    x[1, lens[1]:] = 1e4
    T = WR.frame_counts(S, cfg)[-1]
    out, frames, mask = torch.full((2, S), 7.0).cuda(), torch.zeros(2, dtype=I32).cuda(), torch.full((2, T), 7.0).cuda()
    partials = torch.empty(ops.wav_norm_partials(2, S)).cuda()
    ops.wav_norm(dev32(x), torch.tensor(lens, dtype=I32).cuda(), out, partials, frames, mask, cfg.conv_kernel, cfg.conv_stride)
    want_frames = [WR.frame_counts(n, cfg)[-1] for n in lens]
    assert frames.tolist() == want_frames
    assert float(out[1, lens[1]:].abs().max()) == 0.0
    assert torch.equal(mask.cpu(), (torch.arange(T)[None] < torch.tensor(want_frames)[:, None]).float())
    check(f"wav_norm S={S}", out, WR.wav_norm(dev32(wav).cpu().double(), lens), tol(S))


@pytest.mark.parametrize("C", (32, 512))
def test_conv0_layernorm_gelu(ops, C):
    for S in (10, 14, 15, 400, 4007):
        w, g, beta = rnd(C, 1, 10, seed=C + S, scale=0.3), 1 + 0.1 * rnd(C, seed=1), 0.1 * rnd(C, seed=2)
        wav = rnd(2, S, seed=S)
        T0 = (S - 10) // 5 + 1
        out = torch.full((2, T0 + 1, C), 7.0).cuda()
        ops.wavlm_conv0(dev32(wav), dev32(w[:, 0]), None, dev32(g), dev32(beta), out)
        want = WR.conv_ln_gelu(dev32(wav).cpu().double()[:, :, None], dev32(w).cpu().double(), None, dev32(g).cpu().double(),
                               dev32(beta).cpu().double(), 5)
        assert want.shape == (2, T0, C) and float((out[:, T0] - 7.0).abs().max()) == 0.0      # the pad frame is not touched
        check(f"conv0 C={C} S={S}", out[:, :T0], want, tol(max(10, C)))
    bias = 0.2 * rnd(C, seed=9)
    ops.wavlm_conv0(dev32(wav), dev32(w[:, 0]), dev32(bias), dev32(g), dev32(beta), out)
    want = WR.conv_ln_gelu(dev32(wav).cpu().double()[:, :, None], dev32(w).cpu().double(), dev32(bias).cpu().double(),
                           dev32(g).cpu().double(), dev32(beta).cpu().double(), 5)
    check(f"conv0 C={C} with conv_bias", out[:, :T0], want, tol(max(10, C)))


@pytest.mark.parametrize("C", (32, 512))
def test_strided_view_conv_and_layernorm_gelu(ops, C):
    """Layers 1-6 as the module runs them: ONE f5e_gemm_f32 over both batch rows on an overlapping view (lda = stride * C,
    K = k * C, the batch pitch of the input twice that of the output), then f5e_layernorm_gelu in place."""
    for k, s in ((3, 2), (2, 2)):
        for T_in in (2, 3, 64, 65, 127):
            if T_in < k:
                continue
            T_out = (T_in - k) // s + 1
            P_out = T_out + 1
            P_in = s * P_out
            assert P_in >= (T_out - 1) * s + k
            w, g, beta = rnd(C, C, k, seed=T_in + k, scale=C ** -0.5), 1 + 0.1 * rnd(C, seed=1), 0.1 * rnd(C, seed=2)
            x = rnd(2, P_in, C, seed=T_in)
            flat = torch.cat([dev32(x).view(-1), torch.full((k * C,), float("nan")).cuda()])
            rows = 2 * P_out
            y = torch.empty(rows, C).cuda()
            ops.gemm_f32(torch.as_strided(flat, (rows, k * C), (s * C, 1)), dev32(w.permute(0, 2, 1).reshape(C, k * C)), None, out=y)
            ops.layernorm_gelu(y, y, dev32(g), dev32(beta))
            n_in = (T_out - 1) * s + k
            want = WR.conv_ln_gelu(dev32(x).cpu().double()[:, :n_in], dev32(w).cpu().double(), None, dev32(g).cpu().double(),
                                   dev32(beta).cpu().double(), s)
            check(f"conv C={C} k={k} T_in={T_in}", y.view(2, P_out, C)[:, :T_out], want, tol(k * C))


@pytest.mark.parametrize("D", (64, 1024))
def test_posconv(ops, D):
    G, taps = 16, 128
    cg = D // G
    v, gw, bias = rnd(D, cg, taps, seed=D, scale=(cg * taps) ** -0.5), 1 + 0.2 * rnd(1, 1, taps, seed=3).abs(), 0.1 * rnd(D, seed=4)
    w = WR.fold_wn(gw, v)
    wp = ops.pack_wavlm_posconv_weight(w, G).cuda()
    for T in (1, 63, 64, 65, 130):
        frames = [T, max(1, T - 7)]
        x = rnd(2, T, D, seed=T)
        xd = dev32(x)
        xd[1, frames[1]:] = 1e4
        out = torch.full((2, T, D), 7.0).cuda()
        ops.wavlm_posconv(xd, wp, dev32(bias), torch.tensor(frames, dtype=I32).cuda(), out)
        want = WR.posconv(dev32(x).cpu().double(), wp.cpu().double().permute(0, 2, 3, 1).reshape(D, cg, taps), dev32(bias).cpu().double(),
                          G, frames)
        assert float(out[1, frames[1]:].abs().max()) == 0.0 if frames[1] < T else True
        check(f"posconv D={D} T={T}", out, want, tol(taps * cg))
    full = torch.empty(2, 65, D).cuda()
    ops.wavlm_posconv(dev32(rnd(2, 65, D, seed=65)), wp, dev32(bias), None, full)          # no lengths: every row is full
    want = WR.posconv(dev32(rnd(2, 65, D, seed=65)).cpu().double(), wp.cpu().double().permute(0, 2, 3, 1).reshape(D, cg, taps),
                      dev32(bias).cpu().double(), G)
    check(f"posconv D={D} without lengths", full, want, tol(taps * cg))


@pytest.mark.parametrize("dk", (16, 64))
def test_gate(ops, dk):
    for H in (4, 16):
        for T in (1, 17):
            D = H * dk
            xn, wg, bg, const = rnd(2, T, D, seed=T + H), rnd(8, dk, seed=5, scale=dk ** -0.5), rnd(8, seed=6), 1 + 0.5 * rnd(H, seed=7)
            gate = torch.empty(2, H, T).cuda()
            ops.wavlm_gate(dev32(xn).view(2 * T, D), dev32(wg), dev32(bg), dev32(const), gate)
            want = WR.gate(dev32(xn).cpu().double(), dev32(wg).cpu().double(), dev32(bg).cpu().double(), dev32(const).cpu().double(), H)
            check(f"gate dk={dk} H={H} T={T}", gate, want, tol(dk))


@pytest.mark.parametrize("dk", (16, 64))
def test_relbias_attn(ops, dk):
    from f5e_tts_amd.eval.wavlm import bias_table
    H, B = 4, 2
    D = H * dk
    emb = rnd(320, H, seed=dk).float()
    for T, Tt in ((1, 1), (15, 15), (16, 16), (17, 17), (17, 24), (81, 81), (124, 124), (200, 200)):
        kv = [T, max(1, T - 5)]
        qkv = rnd(B, T, 3 * D, seed=T)
        g = 1 + 0.5 * rnd(B, H, T, seed=T + 1)
        qd = dev32(qkv)
        qd[1, kv[1]:, D:] = 1e4                               # keys and values beyond kv_len
        table = bias_table(emb, Tt)
        guarded = torch.full((H * (2 * Tt - 1) + 8,), float("nan"))
        guarded[4:-4] = table.reshape(-1)                    # NaN on both sides: an index off by one shows
        tab = guarded.cuda()[4:-4].view(H, 2 * Tt - 1)
        flat = qd.view(B * T, 3 * D)
        out = torch.full((B * T, D), 7.0).cuda()
        ops.relbias_attn(flat[:, :D], flat[:, D:2 * D], flat[:, 2 * D:], dev32(g), tab, H, dk ** -0.5,
                         kv_len=torch.tensor(kv, dtype=I32).cuda(), out=out)
        q64 = dev32(qkv).cpu().double()
        want = WR.relbias_attention(q64[..., :D], q64[..., D:2 * D], q64[..., 2 * D:], dev32(g).cpu().double(),
                                    WR.compute_bias(emb, T).double(), H, dk ** -0.5, kv)
        out = out.view(B, T, D)
        if kv[1] < T:
            assert float(out[1, kv[1]:].abs().max()) == 0.0      # a query at or beyond kv_len yields zeros
        check(f"relbias_attn dk={dk} T={T} Tt={Tt}", out, want, tol(dk + T))


# ---- the module ----

def test_ragged_rows_equal_their_own_batch_of_one(model):
    z, _ = gold()
    lens = [40000, 23457, 400]
    wav = torch.full((3, 40000), 1e4)
    for b, n in enumerate(lens):
        wav[b, :n] = torch.from_numpy(z[f"wav_{n}"])
    hs, frames = model.extract(wav.cuda(), torch.tensor(lens, dtype=I32).cuda())
    hs, frames = hs.clone(), frames.tolist()
    assert frames == [124, 73, 1] and torch.isfinite(hs).all()
    for b, n in enumerate(lens):
        one, f1 = model.extract(wav[b:b + 1, :n].cuda())
        assert f1.tolist() == [frames[b]]
        same = torch.equal(hs[:, b, :frames[b]], one[:, 0])
        err = max(WR.rel_l2(hs[l, b, :frames[b]].cpu(), one[l, 0].cpu()) for l in range(4))
        print(f"row {b} ({n} samples) against its B = 1 run: max rel L2 {err:.3e}, bit-identical: {same}")
        assert err < ROW_GATE


def test_extract_allocates_nothing_and_replays_from_a_graph(model):
    z, _ = gold()
    wav = torch.zeros(2, 23457)
    wav[0], wav[1, :20000] = torch.from_numpy(z["wav_23457"]), torch.from_numpy(z["wav_23457"][:20000])
    wav, lens = wav.cuda(), torch.tensor([23457, 20000], dtype=I32).cuda()
    ws = torch.empty(model.workspace_bytes(2, 23457), dtype=torch.uint8).cuda()
    out = torch.empty(4, 2, 73, 64).cuda()
    eager, _ = model.extract(wav, lens)                       # folds the weights and builds the table of T = 73
    eager = eager.clone()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    hs, frames = model.extract(wav, lens, out=out, workspace=ws)
    assert torch.cuda.memory_allocated() == before and hs.data_ptr() == out.data_ptr()
    assert torch.equal(out, eager) and frames.tolist() == [73, 62]
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    out.zero_()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        model.extract(wav, lens, out=out, workspace=ws)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    same = torch.equal(out, eager)
    print(f"graph replay equals the eager result bit for bit: {same}")
    assert same


def test_full_size_configuration(ops):
    """WavLM-large defaults, seeded synthetic weights, one second of audio (49 frames): all 25 hidden states against the
    float64 restatement.  Measured on an MI355X: see DESIGN 4m."""
    from f5e_tts_amd.eval.wavlm import WavLM
    torch.manual_seed(4242)
    big = WavLM()
    wav = (0.1 * torch.randn(1, 16000) + 0.2 * torch.sin(torch.arange(16000) * (2 * math.pi * 180 / 16000)))
    sd = {k: v.detach().double() for k, v in big.state_dict().items()}
    want, frames = WR.forward(sd, big.cfg, wav.double())
    del sd
    hs, fr = big.cuda().extract(wav.cuda())
    assert frames == [49] == fr.tolist() and hs.shape == (25, 1, 49, 1024) and torch.isfinite(hs).all()
    errs = [WR.rel_l2(hs[l].cpu(), want[l]) for l in range(25)]
    print("full size, rel L2 per hidden state: " + " ".join(f"{e:.2e}" for e in errs))
    print(f"full size: max rel L2 {max(errs):.3e} (gate {GATE:.1e})")
    assert max(errs) < GATE


def test_embed_wavs_and_run_sim_from_audio(model, tmp_path):
    from f5e_tts_amd.eval import eval_sim
    from f5e_tts_amd.eval.ecapa_tdnn import ECAPA_TDNN
    from f5e_tts_amd.infer.utils_infer import save_wav
    z, _ = gold()
    torch.manual_seed(7)
    head = ECAPA_TDNN(feat_dim=64, channels=64, emb_dim=16, feat_num=4).cuda()
    wavs = [torch.from_numpy(z["wav_40000"]).cuda(), torch.from_numpy(z["wav_23457"]).cuda()]
    lengths = [model.frame_count(40000), model.frame_count(23457)]
    emb = head.embed_wavs(wavs, feature_extract=model, lengths=lengths)
    pair = torch.zeros(4, 2, 124, 64)
    pair[:, 0], pair[:, 1, :73] = torch.from_numpy(z["hs_pair_0"]), torch.from_numpy(z["hs_pair_1"])
    want = head(pair.cuda(), lengths)
    check("embed_wavs against forward on the fixture's hidden states", emb, want.cpu(), GATE)
    gen, prompts, feats = tmp_path / "gen", tmp_path / "prompts", tmp_path / "feats"
    gen.mkdir(), prompts.mkdir()
    save_wav(str(gen / "utt0.wav"), z["wav_23457"][:12000], 24000)
    save_wav(str(prompts / "p0.wav"), z["wav_40000"][:6000], 16000)
    (tmp_path / "meta.lst").write_text("utt0|prompt text|prompts/p0.wav|truth\n")
    test_set = eval_sim.get_test_set(str(tmp_path / "meta.lst"), str(gen))
    audio = eval_sim.run_sim(test_set, None, None, "cuda", model=head, upstream=model, dump_feats=str(feats))
    stored = eval_sim.run_sim(test_set, None, str(feats), "cuda", model=head)
    print(f"SIM from audio {audio[0]['sim']:.7f}, from the dumped features {stored[0]['sim']:.7f}")
    assert np.load(feats / "utt0.npy").shape == (4, model.frame_count(8000), 64)
    assert abs(audio[0]["sim"] - stored[0]["sim"]) < 1e-6
