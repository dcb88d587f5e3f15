"""The recogniser's 4x / 6x / 8x subsampling fronts and the layer-norm convolution module, CPU side: the fp32 restatement
(tests/asr_subsample_ref.py) against the reference-generated fixtures (tests/golden/make_asr_subsample_golden.py), the
length / mask / window arithmetic of every rate against a literal transcription of the reference loop's bounds, and the
front door (``from_asr_config`` / ``build_asr_model``).  No kernel is launched here."""
import pytest
import torch

import asr_subsample_ref as R

TOL = dict(rtol=1e-4, atol=5e-5)   # fp32 vs fp32, same operation order: the gate of test_ppg_stream_cpu.py
ALL_RATES = (2, 4, 6, 8)


@pytest.mark.parametrize("rate", R.RATES)
def test_restatement_reproduces_the_reference_fixtures(rate):
    sd, g = R.load_fixture(rate)
    causal = rate == 8
    assert R.rate_of(sd) == rate
    assert ("encoder.encoders.0.conv_module.norm.running_mean" in sd) == (R.CNN_NORM[rate] == "batch_norm")
    for tag, lens in (("one", torch.tensor([101])), ("pair", g["lens_pair"])):
        feats = g["feats_" + tag]
        emb, mask = R.embed(sd, feats, lens)
        enc, mask2 = R.encoder(sd, feats, lens, heads=4, causal=causal)
        assert emb.shape == g["embed_" + tag].shape == (feats.shape[0], R.out_frames(feats.shape[1], rate), 64)
        torch.testing.assert_close(emb, g["embed_" + tag], **TOL)
        torch.testing.assert_close(enc, g["enc_" + tag], **TOL)
        torch.testing.assert_close(R.ctc_log_probs(sd, enc), g["logp_" + tag], **TOL)
    # the sliced mask counts MORE frames for the minimum-length row than the convolutions give it alone (one): the
    # reference's rule, kept
    short = int(R.sub_mask((torch.arange(77) < int(g["lens_pair"][1]))[None, None], rate).sum())
    assert torch.equal(mask2[:, 0], g["mask_pair"]) and g["mask_pair"].sum(1).tolist() == [R.out_frames(77, rate), short]
    assert short >= 1 and R.out_frames(int(g["lens_pair"][1]), rate) == 1
    torch.testing.assert_close(R.forward_chunk_by_chunk(sd, g["feats_one"], 4, 2, heads=4, causal=causal), g["cbc"], **TOL)
    window, stride = 3 * rate + R.RIGHT_CONTEXT[rate] + 1, 4 * rate
    assert R.loop_bounds(101, 4, rate)[:2] == [(0, window), (stride, stride + window)]
    cache = (None, None, None)
    for step, (cur, offset) in enumerate(((0, 0), (stride, 4))):
        y, sub, att, cnn = R.forward_chunk(sd, g["feats_one"][:, cur:cur + window], offset, 8, *cache, heads=4, causal=causal)
        cache = (sub, att, cnn)
        assert y.shape == (1, 4, 64) and sub.shape == (1, 4 * (step + 1), 64)
        torch.testing.assert_close(y, g[f"step{step}_y"], **TOL)
        torch.testing.assert_close(sub, g[f"step{step}_sub"], **TOL)
        for i in range(2):
            assert cnn[i].shape == g[f"step{step}_cnn{i}"].shape == ((1, 64, 6) if causal else (1,))
            torch.testing.assert_close(att[i], g[f"step{step}_att{i}"], **TOL)
            torch.testing.assert_close(cnn[i], g[f"step{step}_cnn{i}"], **TOL)


@pytest.mark.parametrize("rate", ALL_RATES)
def test_length_mask_and_window_arithmetic_follow_the_rate(rate):
    from f5e_tts_amd.ppg import ppg_model as M
    from f5e_tts_amd.ppg.streaming_asr import ready_windows
    context = R.RIGHT_CONTEXT[rate] + 1
    assert M.right_context(rate) == R.RIGHT_CONTEXT[rate] and M.INPUT_LAYERS[R.INPUT_LAYER[rate]] == rate
    for T in list(range(context, context + 30)) + [101, 645]:
        # the frames a convolution stack leaves = the length of the sliced mask, and per length the mask's count
        mask = R.sub_mask(torch.ones(1, 1, T, dtype=torch.bool), rate)
        assert M.subsampled_frames(T, rate) == R.out_frames(T, rate) == mask.shape[2] >= 1
        for n in (0, 1, context - 1, context, T // 2, T - 1, T):
            want = int(R.sub_mask((torch.arange(T) < n)[None, None], rate).sum())
            assert M.subsampled_len(n, T, rate) == want
    assert M.subsampled_frames(context - 1, rate) == 0
    for total in list(range(0, 4 * context)) + [101, 333]:
        for chunk in (1, 3, 4, 16):
            want = R.loop_bounds(total, chunk, rate)
            assert ready_windows(total, 0, chunk, True, rate, context) == want
            assert M.ConformerEngine.stream_frames(total, chunk, rate, context) == sum(R.out_frames(e - c, rate) for c, e in want)
            # fed in pieces: only complete windows before the end, the rest at the end
            got, cur = [], 0
            for fed in range(0, total + 1, 5):
                now = ready_windows(fed, cur, chunk, False, rate, context)
                got += now
                cur = now[-1][0] + rate * chunk if now else cur
            got += ready_windows(total, cur, chunk, True, rate, context)
            assert got == want


def test_default_arguments_are_the_2x_front():
    from f5e_tts_amd.ppg import ppg_model as M
    from f5e_tts_amd.ppg.ctc_align import word_spans
    from f5e_tts_amd.ppg.streaming_asr import ready_windows
    for total in (0, 2, 3, 4, 37, 101):
        for chunk in (1, 4, 16):
            want = [(c, min(c + 2 * (chunk - 1) + 3, total)) for c in range(0, total - 3 + 1, 2 * chunk)]
            assert ready_windows(total, 0, chunk, True) == want
            assert M.ConformerEngine.stream_frames(total, chunk) == sum((e - c - 3) // 2 + 1 for c, e in want)
        assert M.subsampled_len(total, 101) == int((torch.arange(0, 101 - 2, 2) < total).sum())
    assert M.right_context() == 2 and M.subsampled_frames(101) == 50
    assert word_spans(["a"], [[1]], [5], 10)[0].end_s == pytest.approx(10 * 0.02)
    assert word_spans(["a"], [[1]], [5], 10, frame_s=0.04)[0].end_s == pytest.approx(10 * 0.04)


@pytest.mark.parametrize("rate", R.RATES)
def test_from_asr_config_builds_the_reference_key_set(rate):
    from f5e_tts_amd import _C
    from f5e_tts_amd.ppg import ConformerPPG
    sd, _ = R.load_fixture(rate)
    cfg = R.fixture_config(rate)
    m = ConformerPPG.from_asr_config(cfg)
    assert m.has_ctc and m.subsampling_rate == rate and m.right_context == R.RIGHT_CONTEXT[rate]
    assert m.input_layer == R.INPUT_LAYER[rate] and m.cnn_module_norm == R.CNN_NORM[rate] and m.causal == (rate == 8)
    own = {k: tuple(v.shape) for k, v in m.state_dict().items()
           if k.startswith(("encoder.", "ctc.")) and "concat_linear" not in k and "num_batches_tracked" not in k}
    want = {k: tuple(v.shape) for k, v in sd.items() if "global_cmvn" not in k}       # the config names no cmvn file
    assert own == want
    lin = "encoder.embed.out.0.weight" if rate == 4 else "encoder.embed.linear.weight"
    assert lin in own and ("encoder.embed.conv.4.weight" in own) == (rate == 8)
    # the extractor's door stays strict: the DiT needs 20 ms PPGs
    with pytest.raises(_C.F5EError, match="input_layer"):
        ConformerPPG.from_config(cfg)
    for key, bad in (("input_layer", "linear"), ("cnn_module_norm", "group_norm"), ("pos_enc_layer_type", "abs_pos"),
                     ("use_emb", True)):
        with pytest.raises(_C.F5EError, match=key):
            ConformerPPG.from_asr_config(dict(cfg, encoder_conf=dict(cfg["encoder_conf"], **{key: bad})))
    with pytest.raises(_C.F5EError):
        ConformerPPG.from_asr_config(dict(cfg, encoder="transformer"))


def test_from_config_refuses_layer_norm_and_from_asr_config_of_a_2x_model_is_from_config():
    from f5e_tts_amd import _C
    from f5e_tts_amd.ppg import ConformerPPG
    cfg = R.fixture_config(4)
    enc2 = dict(cfg["encoder_conf"], input_layer="conv2d", cnn_module_norm="batch_norm")
    with pytest.raises(_C.F5EError, match="cnn_module_norm"):
        ConformerPPG.from_config(dict(cfg, encoder_conf=dict(enc2, cnn_module_norm="layer_norm")))
    a = ConformerPPG.from_config(dict(cfg, encoder_conf=enc2), ctc=True)
    b = ConformerPPG.from_asr_config(dict(cfg, encoder_conf=enc2))
    assert {k: v.shape for k, v in a.state_dict().items()} == {k: v.shape for k, v in b.state_dict().items()}
    assert b.subsampling_rate == 2 and "encoder.embed.out.0.weight" in b.state_dict()


def test_upstream_conv2d_over_a_4x_checkpoint_names_conv2d4(tmp_path):
    import yaml

    from f5e_tts_amd import _C
    from f5e_tts_amd.ppg import build_asr_model, build_ppg_model
    sd, _ = R.load_fixture(4)
    cfg = R.fixture_config(4)
    ckpt = tmp_path / "final.pt"
    torch.save({k: v for k, v in sd.items() if "global_cmvn" not in k}, ckpt)
    good, upstream = tmp_path / "train.yaml", tmp_path / "upstream.yaml"
    good.write_text(yaml.safe_dump(cfg))
    upstream.write_text(yaml.safe_dump(dict(cfg, encoder_conf=dict(cfg["encoder_conf"], input_layer="conv2d"))))
    with pytest.raises(_C.F5EError, match="input_layer: conv2d4"):
        build_asr_model(str(ckpt), str(upstream))
    m = build_asr_model(str(ckpt), str(good))
    assert m.subsampling_rate == 4 and torch.equal(m.state_dict()["encoder.embed.conv.2.weight"], sd["encoder.embed.conv.2.weight"])
    with pytest.raises(_C.F5EError, match="input_layer"):
        build_ppg_model(str(ckpt), str(good))
