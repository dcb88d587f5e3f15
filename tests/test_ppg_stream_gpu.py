"""Streaming (chunk-by-chunk) PPG extraction on the GPU: ConformerPPG.extract(stream=True) / forward_encoder_chunk ->
f5e_relpos_attn + f5e_dwconv_stream (libf5e_hip.so) against
  * the REFERENCE's outputs directly (tests/golden/ppg_stream_*.npz: ASRModel.extract(stream=True) and two forward_chunk calls
    of the reference's own classes, tests/golden/make_ppg_stream_golden.py), and
  * the CPU restatement of the cached loop (tests/ppg_stream_ref.py, pinned by the same fixtures) at the default encoder size,
plus the two kernels on their own against dense torch formulations.  fp32 on both sides; the encoder gates are those of
tests/test_ppg_gpu.py for the same encoder sizes."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import ppg_stream_ref as R
from oracle import f5e_ppg_oracle as P

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def fixture_model(causal):
    from f5e_tts_amd.ppg import ConformerPPG
    sd, g = R.load_stream_fixture(causal)
    m = ConformerPPG(80, 40, 64, 4, 128, 2, 15, global_cmvn=(sd["encoder.global_cmvn.mean"], sd["encoder.global_cmvn.istd"]),
                     causal=causal, use_dynamic_chunk=True)
    full = m.state_dict()
    full.update({k: v for k, v in sd.items() if k in full})
    m.load_state_dict(full)
    return m.cuda().eval(), sd, g


# ------------------------------------------------------------------ the extractor against the reference fixtures

@pytest.mark.parametrize("causal", [False, True])
def test_stream_extract_matches_the_reference_fixture(causal):
    """extract(stream=True) on the reference's weights and features: 322 frames (20 chunks + 2: the limit of 17 left chunks is
    reached) and 37 frames (a short last chunk); gate of test_conformer_matches_the_reference_fixture (same encoder size)."""
    m, _, g = fixture_model(causal)
    for tag in ("long", "short"):
        feats = g["feats_" + tag]
        ppg, logits = m.extract(feats.cuda(), torch.tensor([feats.shape[1]]), stream=True)
        assert ppg.shape == g["ppg_" + tag].shape and logits.shape == g["logits_" + tag].shape       # the loop's frame count
        e, el = rel_l2(ppg, g["ppg_" + tag]), rel_l2(logits, g["logits_" + tag])
        print("causal=%d %s: ppg rel L2 %.2e, logits %.2e" % (causal, tag, e, el))
        assert e < 2e-4 and el < 2e-4
    # speech_lengths is not used in this mode (as in the reference)
    again, _ = m.extract(g["feats_short"].cuda(), torch.tensor([40]), stream=True)
    assert torch.equal(again, ppg)


def test_full_context_extract_of_a_causal_model_matches_the_reference_fixture():
    """extract(stream=False) with causal: true (the causal depthwise convolution with its GLU(bias) left fill is the same in
    both modes): one utterance, and a ragged batch of two."""
    m, _, g = fixture_model(True)
    ppg, logits = m.extract(g["feats_long"].cuda(), torch.tensor([645]))
    e, el = rel_l2(ppg, g["full_ppg_long"]), rel_l2(logits, g["full_logits_long"])
    print("causal full context: ppg rel L2 %.2e, logits %.2e" % (e, el))
    assert ppg.shape == g["full_ppg_long"].shape and e < 2e-4 and el < 2e-4
    ppg, logits = m.extract(g["feats_pair"].cuda(), g["lens_pair"])
    valid = torch.arange(50)[None, :] < torch.tensor([50, 37])[:, None]
    e = rel_l2(ppg.cpu()[valid], g["full_ppg_pair"][valid])
    print("causal full context, ragged pair: ppg rel L2 %.2e" % e)
    assert e < 2e-4 and rel_l2(logits.view(2, 50, -1).cpu()[valid], g["full_logits_pair"].view(2, 50, -1)[valid]) < 2e-4


@pytest.mark.parametrize("T,causal", [(1001, False), (501, False), (501, True)])
def test_default_size_stream_vs_restatement(T, causal, monkeypatch):
    """The encoder at its constructor defaults (256-d, 4 heads of 64, 2048 units, 6 blocks) on 10 s / 5 s of features, gate of
    test_default_size_conformer_vs_oracle.  One attention launch per layer whatever the number of chunks (31 / 16 here), and
    the result is NOT the full-context one (on the CPU the restatement's two modes differ by 5.7e-2 for this model / input)."""
    from f5e_tts_amd import ops
    from f5e_tts_amd.ppg import ConformerPPG
    m = ConformerPPG(80, 218, global_cmvn=(torch.zeros(80), torch.ones(80)), causal=causal, use_dynamic_chunk=True)
    sd = R.seeded_state(m, 11)
    m.load_state_dict(sd)
    m = m.cuda().eval()
    feats = 3.0 * torch.randn(1, T, 80, generator=torch.Generator().manual_seed(7)) + 6.0
    ref, ref_logits = R.asr_extract_stream(sd, feats, heads=4, causal=causal)
    calls, real = [], ops.relpos_attn
    monkeypatch.setattr(ops, "relpos_attn", lambda *a, **kw: (calls.append(kw.get("chunk")), real(*a, **kw))[1])
    ppg, logits = m.extract(feats.cuda(), torch.tensor([T]), stream=True)
    monkeypatch.undo()
    e, el = rel_l2(ppg, ref), rel_l2(logits, ref_logits)
    print("T=%d causal=%d: ppg rel L2 %.2e, logits %.2e, %d attention launches" % (T, causal, e, el, len(calls)))
    assert calls == [16] * 6
    assert ppg.shape == ref.shape == (1, (T - 3) // 2 + 1, 256) and e < 5e-4 and el < 5e-4
    if T == 1001:
        full, _ = m.extract(feats.cuda(), torch.tensor([T]), stream=False)
        d = rel_l2(ppg, full)
        print("stream vs full context rel L2 %.2e" % d)
        assert d > 1e-3


@pytest.mark.parametrize("causal", [False, True])
def test_one_chunk_stream_equals_full_context(causal):
    """With ONE chunk covering the utterance (101 feature frames -> 50 encoder frames, chunk 64, all left chunks) the
    streaming pass and the full-context pass are the same function up to the attention's summation order (f5e_relpos_attn
    against the per-head GEMM + softmax_rows sequence): nothing mode-specific hides in the shared conformer layer.  Gate
    2e-4 relative L2, the gate each mode has against the reference fixture at this encoder size (two results within 2e-4
    of one reference are within 4e-4 of each other: the tighter of the two).  Measured on one MI355X: 1.21e-07 (not
    causal), 1.25e-07 (causal)."""
    from f5e_tts_amd.ppg.ppg_model import ConformerEngine
    m, _, g = fixture_model(causal)
    feats = g["feats_long"][:, :101].cuda()
    eng = m.engine()
    assert ConformerEngine.stream_frames(101, 64) == 50
    stream = eng.forward_chunk_by_chunk(feats, 64, -1)
    full = eng.encode(feats, torch.tensor([101]))[0]
    e = rel_l2(stream, full)
    print("causal=%d: one-chunk stream vs full context rel L2 %.2e" % (causal, e))
    assert stream.shape == full.shape == (1, 50, 64) and e < 2e-4


# ------------------------------------------------------------------ the kernels on their own

def attn_operands(B, T, H, dk, seed):
    g = torch.Generator().manual_seed(seed)
    D = H * dk
    return (torch.randn(B * T, 2 * D, generator=g), torch.randn(B * T, D, generator=g), torch.randn(T, D, generator=g),
            torch.randn(B * T, D, generator=g))


def dense_attention(qu, k, pos, v, B, T, H, dk, lens, chunk, left):
    """Dense masked softmax in fp64 on the CPU from the same fp32 operands; rows at or beyond a sequence's length are zero."""
    D = H * dk
    qu, k, pos, v = qu.double(), k.double(), pos.double(), v.double()
    out = torch.zeros(B * T, D, dtype=torch.float64)
    t = torch.arange(T)
    for b in range(B):
        n = T if lens is None else int(lens[b])
        mask = (t[None, :] < n).expand(T, T).clone()
        if chunk > 0:
            c = t // chunk
            mask &= c[None, :] <= c[:, None]
            if left >= 0:
                mask &= c[None, :] >= c[:, None] - left
        r = slice(b * T, (b + 1) * T)
        for h in range(H):
            cs = slice(h * dk, (h + 1) * dk)
            s = (qu[r, cs] @ k[r, cs].T + qu[r, D + h * dk:D + (h + 1) * dk] @ pos[:T, cs].T) / math.sqrt(dk)
            a = torch.softmax(s.masked_fill(~mask, -float("inf")), dim=-1)
            out[r, cs] = a @ v[r, cs]
        out[b * T + n:(b + 1) * T] = 0.0
    return out


def existing_sequence(qu, k, pos, v, B, T, H, dk, lens):
    """The full-context launch sequence of ConformerEngine.forward on the same operands, by the engine's own method
    (ConformerEngine._full_attn: per sequence and head (q+u) k^T, + (q+v) p^T, softmax_rows, P.V on the fp32 GEMM).  The
    method projects its value rows with the layer's weight and adds the bias after P.V: an identity and zeros hand it v."""
    from f5e_tts_amd.ppg.ppg_model import ConformerEngine
    D, dv = H * dk, qu.device
    eng = object.__new__(ConformerEngine)
    eng.device, eng.dim, eng.heads, eng.dk = dv, D, H, dk
    layer = dict(wv=torch.eye(D, device=dv), bv=torch.zeros(D, device=dv))
    kv = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dv)
    return eng._full_attn(layer, qu, k, pos[:T], v, torch.empty(B * T, D, device=dv), B=B, T=T, kv_len=kv,
                          ws=eng._full_attn_scratch(T))


@pytest.mark.parametrize("dk", [16, 64])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 250, 500])
def test_relpos_attn_kernel(T, dk):
    """f5e_relpos_attn against a dense masked softmax (fp64 on the CPU, same fp32 operands): full context (chunk <= 0), where
    it must also agree with the existing per-head GEMM + softmax_rows sequence, and the bands (16, 17), (16, 2), (8, -1),
    (4, 0).  fp32 summation-order differences only: gate 1e-5 relative L2.  The existing sequence against the same dense
    result is printed beside it (it is the yardstick for that gate; measured on one MI355X over these sizes: existing
    sequence 1.5e-7 ... 5.5e-7, fused kernel 1.5e-7 ... 5.6e-7, so the 1e-5 gate stands)."""
    from f5e_tts_amd import ops
    H = 4
    qu, k, pos, v = attn_operands(1, T, H, dk, 100 + T + dk)
    dev = [t.cuda() for t in (qu, k, pos, v)]
    scale = 1.0 / math.sqrt(dk)
    dense = dense_attention(qu, k, pos, v, 1, T, H, dk, None, 0, -1)
    old = existing_sequence(*dev, 1, T, H, dk, None)
    out = ops.relpos_attn(*dev, torch.full((T, H * dk), float("nan"), device="cuda"), H, scale)
    e_old, e_new = rel_l2(old, dense), rel_l2(out, dense)
    print("T=%d dk=%d full: existing sequence vs dense %.2e, fused vs dense %.2e, fused vs existing %.2e"
          % (T, dk, e_old, e_new, rel_l2(out, old)))
    assert e_new < 1e-5 and rel_l2(out, old) < 1e-5
    for chunk, left in ((16, 17), (16, 2), (8, -1), (4, 0)):
        out = ops.relpos_attn(*dev, torch.full((T, H * dk), float("nan"), device="cuda"), H, scale, chunk=chunk,
                              left_chunks=left)
        e = rel_l2(out, dense_attention(qu, k, pos, v, 1, T, H, dk, None, chunk, left))
        print("T=%d dk=%d band (%d, %d): fused vs dense %.2e" % (T, dk, chunk, left, e))
        assert e < 1e-5


@pytest.mark.parametrize("dk", [16, 64])
def test_relpos_attn_ragged_batch_and_query_offset(dk):
    """A ragged batch of two (keys past a sequence's length unseen, its rows past the length zero) in full context against the
    existing sequence and the dense result, and banded; q_begin: only the rows from q_begin on are written."""
    from f5e_tts_amd import ops
    B, T, H, lens = 2, 77, 4, [77, 45]
    qu, k, pos, v = attn_operands(B, T, H, dk, 7 + dk)
    pos = torch.cat([pos, torch.randn(9, H * dk)])                  # a table longer than the sequences
    dev = [t.cuda() for t in (qu, k, pos, v)]
    kv = torch.tensor(lens, dtype=torch.int32, device="cuda")
    scale = 1.0 / math.sqrt(dk)
    valid = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).reshape(-1)
    old = existing_sequence(*dev, B, T, H, dk, lens)
    for chunk, left in ((0, -1), (16, 2), (8, -1)):
        dense = dense_attention(qu, k, pos, v, B, T, H, dk, lens, chunk, left)
        out = ops.relpos_attn(*dev, torch.full((B * T, H * dk), float("nan"), device="cuda"), H, scale, B=B, kv_len=kv,
                              chunk=chunk, left_chunks=left)
        e = rel_l2(out, dense)
        print("ragged dk=%d band (%d, %d): fused vs dense %.2e" % (dk, chunk, left, e))
        assert e < 1e-5 and float(out.cpu()[~valid].abs().max()) == 0.0
        if chunk == 0:
            print("ragged dk=%d: existing vs dense %.2e" % (dk, rel_l2(old.cpu()[valid], dense[valid])))
            assert rel_l2(out.cpu()[valid], old.cpu()[valid]) < 1e-5
    dense = dense_attention(qu, k, pos, v, B, T, H, dk, None, 0, -1)
    out = torch.full((B * T, H * dk), 7.0, device="cuda")
    ops.relpos_attn(*dev, out, H, scale, B=B, q_begin=61)
    out = out.view(B, T, -1).cpu()
    assert float((out[:, :61] - 7.0).abs().max()) == 0.0
    assert rel_l2(out[:, 61:], dense.view(B, T, -1)[:, 61:]) < 1e-5


def test_relpos_attn_argument_checks():
    from f5e_tts_amd import _C, ops
    z = lambda *s: torch.zeros(*s, device="cuda")   # noqa: E731
    with pytest.raises(_C.F5EError, match="head dim 36"):
        ops.relpos_attn(z(8, 288), z(8, 144), z(8, 144), z(8, 144), z(8, 144), 4, 1.0)
    with pytest.raises(_C.F5EError, match="inconsistent shapes"):
        ops.relpos_attn(z(8, 128), z(8, 64), z(7, 64), z(8, 64), z(8, 64), 4, 1.0)
    with pytest.raises(_C.F5EError, match="q_begin"):
        ops.relpos_attn(z(8, 128), z(8, 64), z(8, 64), z(8, 64), z(8, 64), 4, 1.0, q_begin=8)


@pytest.mark.parametrize("K,causal,chunk", [(15, False, 16), (15, False, 4), (7, False, 0), (15, True, 0), (8, True, 0), (2, True, 0)])
def test_dwconv_stream_kernel(K, causal, chunk):
    """f5e_dwconv_stream against torch.nn.functional.conv1d: chunk-isolated (every chunk convolved on its own with zero
    padding), whole-sequence (equal to f5e_dwconv), and causal with the per-channel left fill, even K included.  At most 15
    fp32 products per output in a different order: gate 1e-6 relative L2."""
    from f5e_tts_amd import ops
    g = torch.Generator().manual_seed(K + chunk)
    B, T, C = 2, 53, 64
    x, w, b = torch.randn(B, T, C, generator=g), torch.randn(C, 1, K, generator=g), torch.randn(C, generator=g)
    fill = torch.randn(C, generator=g)
    xt = x.transpose(1, 2).double()
    if causal:
        left = fill.double()[None, :, None].expand(B, C, K - 1)
        ref = F.conv1d(torch.cat([left, xt], 2), w.double(), b.double(), groups=C)
    elif chunk > 0:
        ref = torch.cat([F.conv1d(p, w.double(), b.double(), padding=(K - 1) // 2, groups=C) for p in xt.split(chunk, 2)], 2)
    else:
        ref = F.conv1d(xt, w.double(), b.double(), padding=(K - 1) // 2, groups=C)
    w_t = w[:, 0, :].t().contiguous().cuda()
    out = ops.dwconv_stream(x.cuda(), w_t, b.cuda(), torch.empty(B, T, C, device="cuda"), causal=causal, chunk=chunk,
                            fill=fill.cuda() if causal else None)
    e = rel_l2(out, ref.transpose(1, 2))
    print("dwconv_stream K=%d causal=%d chunk=%d: rel L2 %.2e" % (K, causal, chunk, e))
    assert e < 1e-6
    if not causal and chunk == 0:
        assert torch.equal(out, ops.dwconv(x.cuda(), w_t, b.cuda(), torch.empty(B, T, C, device="cuda")))
    if causal:          # without a fill the left context is zero
        out0 = ops.dwconv_stream(x.cuda(), w_t, b.cuda(), torch.empty(B, T, C, device="cuda"), causal=True)
        assert rel_l2(out0, F.conv1d(F.pad(xt, (K - 1, 0)), w.double(), b.double(), groups=C).transpose(1, 2)) < 1e-6


# ------------------------------------------------------------------ incremental interface

@pytest.mark.parametrize("causal", [False, True])
def test_forward_encoder_chunk_window_by_window(causal):
    """Feeding the fixture utterance through forward_encoder_chunk, one window of 33 feature frames at stride 32 at a time
    with the caches handed back in, reproduces forward_chunk_by_chunk (1e-5: the same kernels on [cache ; chunk], in another
    summation order), and the first two steps reproduce the reference's outputs and caches (fixture gate, 2e-4)."""
    m, _, g = fixture_model(causal)
    feats = g["feats_long"].cuda()
    whole = m.engine().forward_chunk_by_chunk(feats, 16, 17)
    cache, outs, offset = (None, None, None), [], 0
    for step, (cur, end) in enumerate(R.stream_windows(feats.shape[1], 16)):
        y, sub, att, cnn = m.forward_encoder_chunk(feats[:, cur:end], offset, 16 * 17, *cache)
        cache = (sub, att, cnn)
        outs.append(y)
        offset += y.shape[1]
        assert sub.shape[1] == min(offset, 16 * 17) and all(a.shape == sub.shape for a in att)
        if step < 2:
            assert rel_l2(y, g[f"step{step}_y"]) < 2e-4 and rel_l2(sub, g[f"step{step}_sub"]) < 2e-4
            for i in range(2):
                assert rel_l2(att[i], g[f"step{step}_att{i}"]) < 2e-4
                assert cnn[i].shape == g[f"step{step}_cnn{i}"].shape
                if causal:
                    assert rel_l2(cnn[i], g[f"step{step}_cnn{i}"]) < 2e-4
    ys = torch.cat(outs, 1)
    e = rel_l2(ys, whole)
    print("causal=%d: %d windows, incremental vs one pass rel L2 %.2e" % (causal, len(outs), e))
    assert ys.shape == whole.shape == (1, 322, 64) and len(outs) == 21 and e < 1e-5
    ppg, _ = m.engine().head(ys)
    assert rel_l2(ppg, g["ppg_long"]) < 2e-4


# ------------------------------------------------------------------ wrapper and eval driver

def test_wrapper_and_eval_driver_stream_mode(tmp_path):
    """PPGModelWapper(..., stream=True).audio_to_ppg and eval_infer_batch --mode vc --ppg_stream on the synthetic set-up of
    test_eval_driver_vc_mode_extracts_ppg_on_the_gpu: the written audio equals a direct extract(stream=True) -> sample_vc ->
    decode on the same inputs (int16 file round trip), and the streaming PPGs are not the full-context ones."""
    import yaml
    from safetensors.torch import save_file

    import f5e_tts_amd
    from f5e_tts_amd.eval import eval_infer_batch as E
    from f5e_tts_amd.infer import audio as A
    from f5e_tts_amd.infer import utils_infer as U
    from f5e_tts_amd.model import CFM, DiT
    from f5e_tts_amd.ppg import ConformerPPG, PPGModelWapper
    from f5e_tts_amd.train.parse_cfg import parse_model_yaml
    from f5e_tts_amd.vocoder import Vocos
    from tools import synth as SY
    pkg = os.path.dirname(os.path.abspath(f5e_tts_amd.__file__))
    cfg = yaml.safe_load(open(os.path.join(pkg, "configs", "F5TTS_Small_PPG.yaml")))
    cfg["model"]["arch"].update(depth=2, conv_layers=2)
    cfg["model"]["ppg_config"].update(model_path=str(tmp_path / "33.pt"), config=str(tmp_path / "train.yaml"))
    (tmp_path / "model.yaml").write_text(yaml.safe_dump(cfg))
    mc = parse_model_yaml(cfg)
    torch.manual_seed(77)
    dit = DiT(**mc["arch"], text_num_embeds=2545, mel_dim=100, ppg_config=mc["transformer_ppg_config"],
              cb_config=mc["transformer_codebook_config"])
    for p_ in dit.parameters():
        if float(p_.detach().abs().max()) == 0:
            torch.nn.init.normal_(p_, std=0.02)
    cfm = CFM(transformer=dit, ppg_config=mc["cfm_ppg_config"], cb_config=mc["cfm_codebook_config"])
    save_file({"ema_model." + k: v.contiguous() for k, v in cfm.state_dict().items()}, str(tmp_path / "model.safetensors"))
    cfm = cfm.cuda().eval()
    ppg_cfg = dict(cmvn_file=None, is_json_cmvn=True, input_dim=80, output_dim=218, encoder="conformer",
                   encoder_conf=dict(output_size=256, attention_heads=4, linear_units=512, num_blocks=2, causal=True,
                                     use_dynamic_chunk=True))
    (tmp_path / "train.yaml").write_text(yaml.safe_dump(ppg_cfg))
    pm = ConformerPPG.from_config(ppg_cfg)
    torch.save(R.seeded_state(pm, 5), str(tmp_path / "33.pt"))
    vdir = tmp_path / "vocos"
    vdir.mkdir()
    (vdir / "config.yaml").write_text(yaml.safe_dump({
        "backbone": {"init_args": dict(input_channels=100, dim=512, intermediate_dim=1536, num_layers=8)},
        "head": {"init_args": dict(dim=512, n_fft=1024, hop_length=256, padding="center")}}))
    voc = Vocos()
    voc.load_state_dict(SY.init_vocos_state(), strict=False)
    torch.save(voc.state_dict(), str(vdir / "pytorch_model.bin"))
    voc = voc.cuda().eval()
    audio = tmp_path / "wavs"
    audio.mkdir()
    ref = SY.synthetic_ref_wave(96, seed=1)[0] * 3.0          # ~1 s prompt
    src = SY.synthetic_ref_wave(190, seed=2)[0] * 3.0         # ~2 s source utterance
    U.save_wav(str(audio / "ref0.wav"), ref.numpy(), 24000)
    U.save_wav(str(audio / "gen0.wav"), src.numpy(), 24000)
    (tmp_path / "test.lst").write_text("\t".join(["ref0", "1.0", "some prompt text.", "gen0", "2.0", "converted content."]) + "\n")
    out_dir = tmp_path / "out"
    E.main(["-n", "F5TTS_Small_PPG", "-t", str(tmp_path / "test.lst"), "-nfe", "4", "-s", "0", "--mode", "vc", "--ckpt",
            str(tmp_path / "model.safetensors"), "--audio_root", str(audio), "--vocoder_path", str(vdir), "--output_dir",
            str(out_dir), "-mc", str(tmp_path / "model.yaml"), "--ppg_stream"])
    got, sr = U.load_wav(str(out_dir / "gen0.wav"))
    a, _ = U.load_wav(str(audio / "ref0.wav"))
    s, _ = U.load_wav(str(audio / "gen0.wav"))
    ref_len = a.shape[-1] // 256
    tot = ref_len + int(s.shape[-1] / 256)
    assert sr == 24000 and got.shape == (1, 256 * (tot - ref_len - 1))
    w = PPGModelWapper(str(tmp_path / "33.pt"), str(tmp_path / "train.yaml"), "cuda", stream=True)
    full16 = torch.cat([A.resample(a, 24000, 16000), A.resample(s, 24000, 16000)], dim=1)
    ppg, _ = w.audio_to_ppg(full16.cuda(), 16000)
    feats, flen = w.audio_to_mel(full16.cuda(), 16000)
    direct_ppg, _ = w.ppg_model.extract(feats, flen, stream=True)
    assert ppg.shape == direct_ppg.shape and ppg.shape[2] == 256 and abs(ppg.shape[1] - round(0.533 * tot)) <= 3
    true_len = int(flen) // 2
    assert rel_l2(ppg[:, :true_len], direct_ppg[:, :true_len]) < 1e-6       # ppg_to_target only zeroes the padded frames
    plain, _ = PPGModelWapper(str(tmp_path / "33.pt"), str(tmp_path / "train.yaml"), "cuda").audio_to_ppg(full16.cuda(), 16000)
    assert rel_l2(ppg, plain) > 1e-3
    mel_in = cfm.mel_spec(a.cuda()).permute(0, 2, 1)[:, :ref_len]
    mel, _ = cfm.sample_vc(mel_in, ppg, duration=torch.tensor([tot]), steps=4, alpha_spk=2.5, alpha_ppg=3.0,
                           sway_sampling_coef=-1.0, seed=0)
    direct = voc.decode(mel[:, ref_len:tot].permute(0, 2, 1)).cpu()
    assert float((got - direct.clamp(-1, 1)).abs().max()) <= 2.0 / 32768
