"""The recogniser on the reference's 4x / 6x / 8x subsampling fronts, on the GPU: f5e_conv2d_sub_f32 (csrc/subsample.hip) on
its own against torch's conv2d, and ConformerPPG.from_asr_config / build_asr_model / CTCAligner(asr=True) against the
REFERENCE's outputs (tests/golden/asr_subsample_{4,6,8}.npz, made by the reference's own classes) and the CPU restatement's
decodes of them.  fp32 on both sides; the encoder gate is the one tests/test_ppg_gpu.py holds this path to."""
import json
import math

import pytest
import torch
import torch.nn.functional as F

import asr_subsample_ref as R
import ctc_beam_ref

pytestmark = pytest.mark.gpu

GATE = 5e-4      # rel L2, fp32 on both sides: test_ppg_gpu.py's gate of this encoder path


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------ the kernel on its own

@pytest.mark.parametrize("ksize,stride,C,t_ins", [
    (3, 2, 64, (3, 4, 37)),
    (3, 2, 80, (3, 4, 37, 215)),   # C no multiple of the 64-wide tile; T_in 215 x F_in 39 crosses the 32-row / 64-row tile switch
    (5, 3, 48, (5, 6, 37)),        # a 5 x 5 kernel needs 5 rows: 5 and 6 are its single-row inputs (3 and 4 must raise)
])
def test_conv2d_sub_matches_torch_conv2d(ksize, stride, C, t_ins):
    """B = 2; T_in gives single-row outputs and a T tail, F_in in {39, 19} an F tail; K = 9 C or 25 C is never a multiple of
    the 64-float K-step except at C = 64.  Bound: the one of test_ops_gpu.py::test_gemm_f32 with an activation (rtol 1e-5, atol
    3e-5 on unit-variance outputs) -- its K reaches 1536, these reach 25 * 48 = 1200.  Measured on one MI355X: largest error
    5.2e-6 over all cases (torch's fp32 conv2d against a float64 one on the same inputs: 0.7e-6 .. 2.3e-6)."""
    from f5e_tts_amd import _C, ops
    ops.require_device()
    gen = torch.Generator().manual_seed(100 * ksize + C)
    K = ksize * ksize * C
    w = torch.randn(C, C, ksize, ksize, generator=gen) / math.sqrt(K)
    b = torch.randn(C, generator=gen)
    wp = ops.pack_conv2d_sub_weight(w.cuda())
    assert wp.shape == (C, ksize, ksize, C)
    for T_in in t_ins:
        for F_in in (39, 19):
            x = torch.randn(2, C, T_in, F_in, generator=gen)                      # torch layout; the kernel gets channels-last
            ref = F.relu(F.conv2d(x, w, b, stride=stride)).permute(0, 2, 3, 1)
            ref64 = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=stride)).permute(0, 2, 3, 1)
            out = ops.conv2d_sub(x.permute(0, 2, 3, 1).contiguous().cuda(), wp, b.cuda(), stride)
            assert out.shape == ref.shape == (2, (T_in - ksize) // stride + 1, (F_in - ksize) // stride + 1, C)
            err, lim = (out.cpu() - ref).abs(), 3e-5 + 1e-5 * ref.abs()
            print("k%d s%d C=%d T_in=%d F_in=%d: max err %.3e (torch fp32 against fp64: %.3e)"
                  % (ksize, stride, C, T_in, F_in, float(err.max()), float((ref - ref64).abs().max())))
            assert not (err > lim).any(), f"T_in={T_in} F_in={F_in}: max err {float(err.max()):.3e}"
            assert float(out.min()) >= 0.0                                        # the ReLU is in the epilogue
    no_act = ops.conv2d_sub(x.permute(0, 2, 3, 1).contiguous().cuda(), wp, None, stride, act=ops.ACT_NONE)
    plain = F.conv2d(x, w, None, stride=stride).permute(0, 2, 3, 1)
    assert not ((no_act.cpu() - plain).abs() > 3e-5 + 1e-5 * plain.abs()).any() and float(no_act.min()) < 0.0
    # refused before any launch
    for bad in (torch.zeros(2, ksize - 1, 19, C), torch.zeros(2, 19, ksize - 1, C)):
        with pytest.raises(_C.F5EError, match="smaller than the kernel"):
            ops.conv2d_sub(bad.cuda(), wp, None, stride)
    with pytest.raises(_C.F5EError, match="multiple of 16"):
        ops.conv2d_sub(torch.zeros(1, 9, 9, 24).cuda(), torch.zeros(24, 3, 3, 24).cuda(), None, 2)


# ------------------------------------------------------------------ the encoder against the reference fixtures

_models = {}


def fixture_model(rate):
    """ConformerPPG.from_asr_config on the fixture's config and weights, on the GPU; built once per rate."""
    if rate not in _models:
        from f5e_tts_amd.ppg import ConformerPPG
        from f5e_tts_amd.ppg.ppg_model import _GlobalCMVN
        sd, g = R.load_fixture(rate)
        m = ConformerPPG.from_asr_config(R.fixture_config(rate))
        m.encoder.global_cmvn = _GlobalCMVN(sd["encoder.global_cmvn.mean"], sd["encoder.global_cmvn.istd"])
        full = m.state_dict()
        assert all(k in full for k in sd)
        full.update(sd)
        m.load_state_dict(full)
        _models[rate] = (m.cuda().eval(), sd, g)
    return _models[rate]


@pytest.mark.parametrize("rate", R.RATES)
def test_encoder_and_ctc_match_the_reference_fixture(rate, monkeypatch):
    """One utterance (101 frames, no multiple of the rate) and a ragged pair whose second row has the minimum length:
    subsampling output, encoder output and CTC log-probabilities over the frames the reference's mask calls valid.
    Measured on one MI355X: 1.0e-7 .. 6.8e-7 relative L2 at every rate."""
    from f5e_tts_amd import ops
    m, sd, g = fixture_model(rate)
    eng = m.engine()
    assert (eng.rate, eng.context, m.subsampling_rate) == (rate, R.RIGHT_CONTEXT[rate] + 1, rate)
    calls, real = [], ops.conv2d_sub
    monkeypatch.setattr(ops, "conv2d_sub", lambda *a, **kw: (calls.append(a[0].shape), real(*a, **kw))[1])
    emb = eng._subsample(g["feats_one"].cuda())
    assert len(calls) == len(R.CONVS[rate]) - 1                    # the C -> C convolutions run on the new kernel
    e = rel_l2(emb.view(1, -1, 64), g["embed_one"])
    enc, lens = eng.encode(g["feats_one"].cuda(), torch.tensor([101]))
    logp = torch.log_softmax(eng.ctc_logits(enc), -1)
    e2, e3 = rel_l2(enc, g["enc_one"]), rel_l2(logp, g["logp_one"])
    print("rate %d, one utterance: embed rel L2 %.2e, encoder %.2e, CTC log-probs %.2e" % (rate, e, e2, e3))
    assert enc.shape == g["enc_one"].shape and lens.tolist() == [g["enc_one"].shape[1]]
    assert max(e, e2, e3) < GATE
    # ragged pair; the conv module's output rows of padded frames are exactly zero, as on the 2x front
    padded = []
    real_axpby = ops.axpby
    valid = g["mask_pair"]

    def axpby(x, y, out, a, b, *rest):
        if y is not None and x.shape[0] == valid.numel():
            padded.append(float(y.view(2, -1, 64).cpu()[~valid].abs().max()))
        return real_axpby(x, y, out, a, b, *rest)
    monkeypatch.setattr(ops, "axpby", axpby)
    enc, lens = eng.encode(g["feats_pair"].cuda(), g["lens_pair"])
    monkeypatch.undo()
    assert lens.tolist() == valid.sum(1).tolist() and enc.shape == g["enc_pair"].shape
    assert len(padded) == 2 and max(padded) == 0.0                 # one conv module per block
    logp = torch.log_softmax(eng.ctc_logits(enc), -1)
    e2, e3 = rel_l2(enc.cpu()[valid], g["enc_pair"][valid]), rel_l2(logp.cpu()[valid], g["logp_pair"][valid])
    e = rel_l2(eng._subsample(g["feats_pair"].cuda()).view(2, -1, 64), g["embed_pair"])     # padded frames convolved as they are
    print("rate %d, ragged pair: embed rel L2 %.2e, encoder %.2e, CTC log-probs %.2e" % (rate, e, e2, e3))
    assert max(e, e2, e3) < GATE
    # the public extract on this model: ppg = linear(encoder output)
    ppg, _ = m.extract(g["feats_one"].cuda(), torch.tensor([101]))
    want = F.linear(g["enc_one"], m.linear.weight.detach().cpu(), m.linear.bias.detach().cpu())
    assert rel_l2(ppg, want) < GATE
    with pytest.raises(Exception, match=f"at least {R.RIGHT_CONTEXT[rate] + 1} feature frames"):
        eng.encode(g["feats_one"][:, :R.RIGHT_CONTEXT[rate]].cuda(), torch.tensor([R.RIGHT_CONTEXT[rate]]))


@pytest.mark.parametrize("rate", R.RATES)
def test_streaming_encoder_matches_the_reference_fixture(rate):
    """forward_chunk_by_chunk(chunk 4, 2 left chunks) and two consecutive forward_chunk calls with every returned cache."""
    m, sd, g = fixture_model(rate)
    causal = rate == 8
    cbc = m.engine().forward_chunk_by_chunk(g["feats_one"].cuda(), 4, 2)
    e = rel_l2(cbc, g["cbc"])
    print("rate %d: forward_chunk_by_chunk rel L2 %.2e" % (rate, e))
    assert cbc.shape == g["cbc"].shape and e < GATE
    window, stride = 3 * rate + R.RIGHT_CONTEXT[rate] + 1, 4 * rate
    cache = (None, None, None)
    for step, (cur, offset) in enumerate(((0, 0), (stride, 4))):
        y, sub, att, cnn = m.forward_encoder_chunk(g["feats_one"][:, cur:cur + window].cuda(), offset, 8, *cache)
        cache = (sub, att, cnn)
        errs = [rel_l2(y, g[f"step{step}_y"]), rel_l2(sub, g[f"step{step}_sub"])]
        assert y.shape == g[f"step{step}_y"].shape and sub.shape == g[f"step{step}_sub"].shape
        for i in range(2):
            assert att[i].shape == g[f"step{step}_att{i}"].shape and cnn[i].shape == g[f"step{step}_cnn{i}"].shape
            errs.append(rel_l2(att[i], g[f"step{step}_att{i}"]))
            if causal:
                errs.append(rel_l2(cnn[i], g[f"step{step}_cnn{i}"]))
            else:
                assert float(cnn[i].abs().max()) == 0.0            # the reference's dummy
        print("rate %d step %d: worst rel L2 %.2e" % (rate, step, max(errs)))
        assert max(errs) < GATE


def test_streaming_recognizer_on_the_4x_model_does_not_depend_on_the_feeding():
    m, sd, g = fixture_model(4)
    feats = g["feats_one"][0]
    whole = m.streaming_recognizer(beam_size=4, decoding_chunk_size=4, num_decoding_left_chunks=2, max_seconds=2.0)
    assert (whole.rate, whole.context) == (4, 7)
    assert whole.accept_features(feats) == 24                      # six complete windows of 19 frames at stride 16
    want = whole.finish()
    assert whole.offset == 24 and rel_l2(whole.encoder_out(), g["cbc"]) < GATE
    pieces = m.streaming_recognizer(beam_size=4, decoding_chunk_size=4, num_decoding_left_chunks=2, max_seconds=2.0)
    at, added = 0, []
    for n in (5, 1, 13, 30, 0, 17, 35):
        added.append(pieces.accept_features(feats[at:at + n]))
        at += n
    assert at == 101 and sum(added) == 24 and added[:2] == [0, 0] and added[2] == 4      # 19 frames make the first window
    got = pieces.finish()
    assert [ids for ids, _ in got] == [ids for ids, _ in want] and len(want) >= 1
    for (_, a), (_, b) in zip(got, want):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b))


# ------------------------------------------------------------------ the public path

CHARS = "abcdefghijklmnopqrstuvwxyz0123"          # one character per id: text <-> ids is a bijection (id 0 is the blank)


def test_ctc_aligner_asr_on_the_4x_fixture_model(tmp_path, monkeypatch):
    import yaml

    from f5e_tts_amd.ppg.ctc_align import CTCAligner
    sd, g = R.load_fixture(4)
    cfg = R.fixture_config(4)
    cmvn = tmp_path / "global_cmvn"
    cmvn.write_text(json.dumps(dict(mean_stat=[0.0] * 80, var_stat=[1.0] * 80, frame_num=1)))   # the checkpoint's values replace it
    cfg.update(cmvn_file=str(cmvn), is_json_cmvn=True)
    (tmp_path / "train.yaml").write_text(yaml.safe_dump(cfg))
    torch.save(sd, tmp_path / "final.pt")
    (tmp_path / "units.txt").write_text("".join(f"{c} {i}\n" for i, c in enumerate(CHARS)))
    al = CTCAligner(str(tmp_path / "final.pt"), str(tmp_path / "train.yaml"), str(tmp_path / "units.txt"), "cuda", asr=True)
    assert al.model.subsampling_rate == 4 and al.frame_s == pytest.approx(0.04)
    feats = g["feats_one"].cuda()
    monkeypatch.setattr(al, "_feats", lambda audio, sr: (feats, torch.tensor([101], device="cuda"), 1.025))
    logp = g["logp_one"][0]
    greedy = R.greedy_ids(logp)
    hyps, delta = R.beam_nbest(logp, 4)
    _, _, E, same = ctc_beam_ref.margin(logp.numpy(), 4)
    assert len(greedy) >= 1 and same and ctc_beam_ref.usable(delta, E)            # the fixture decides its n-best with a margin
    assert al.transcribe(None, 16000) == "".join(CHARS[i] for i in greedy)
    assert al.transcribe(None, 16000, mode="ctc_prefix_beam_search", beam_size=4) == "".join(CHARS[i] for i in hyps[0][0])
    text = " ".join(CHARS[i] for i in greedy)                     # every token its own word
    spans = al.align(None, 16000, text)
    assert [s.word for s in spans] == text.split() and spans[0].start_s == 0.0
    assert spans[-1].end_s == pytest.approx(g["enc_one"].shape[1] * 0.04)
    for s in spans:
        for t in (s.start_s, s.end_s):
            assert abs(t / 0.04 - round(t / 0.04)) < 1e-9
        assert s.end_s > s.start_s
    assert math.isfinite(al.score(None, 16000, text))
