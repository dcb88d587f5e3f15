"""BigVGAN vocoder host side (no GPU): construction, checkpoint loading and weight-norm folding, the anti-alias filter,
the slaney filterbank, the polyphase repack of the transposed convs, and the CLI / eval wiring."""
import json
import math

import pytest
import torch
import torch.nn.functional as F

from tools import synth as SY


def test_melspec_bigvgan_constructs_and_needs_a_gpu():
    from f5e_tts_amd._C import F5EError
    from f5e_tts_amd.model import MelSpec
    ms = MelSpec(mel_spec_type="bigvgan")
    assert ms.mel_spec_type == "bigvgan"
    if not torch.cuda.is_available():
        with pytest.raises(F5EError):
            ms(torch.zeros(1, 4096))


def _write_ckpt(tmp_path, cfg, form):
    d = tmp_path / form
    d.mkdir()
    (d / "config.json").write_text(json.dumps(cfg))
    sd = SY.init_bigvgan_state(cfg, 5, weight_norm_form=form)
    torch.save({"generator": sd}, d / "bigvgan_generator.pt")
    return d, sd


def test_load_vocoder_bigvgan_both_weight_norm_forms(tmp_path):
    from f5e_tts_amd.infer import utils_infer as U
    from f5e_tts_amd.vocoder_bigvgan import BigVGAN
    cfg = SY.bigvgan_config(256)
    d1, sd1 = _write_ckpt(tmp_path, cfg, "weight_g")
    d2, sd2 = _write_ckpt(tmp_path, cfg, "parametrizations")
    v1 = U.load_vocoder("bigvgan", is_local=True, local_path=str(d1), device="cpu")
    v2 = U.load_vocoder("bigvgan", is_local=True, local_path=str(d2), device="cpu")
    assert isinstance(v1, BigVGAN) and isinstance(v2, BigVGAN)
    assert v1.w("conv_pre.weight").shape == (256, 100, 7)
    assert v1.w("ups.0.0.weight").shape == (256, 128, 8)
    assert v1.w("conv_post.bias") is None          # use_bias_at_final: false
    for name in v1._names:
        torch.testing.assert_close(v1.w(name), v2.w(name), rtol=0, atol=0)
    with pytest.raises(FileNotFoundError):
        U.load_vocoder("bigvgan", is_local=True, local_path=str(tmp_path / "nope"))
    with pytest.raises(RuntimeError):
        U.load_vocoder("bigvgan", is_local=False)


def test_folded_weights_equal_torch_weight_norm():
    from f5e_tts_amd.vocoder_bigvgan import fold_weight_norm
    torch.manual_seed(0)
    conv = torch.nn.utils.weight_norm(torch.nn.Conv1d(12, 20, 7))
    convt = torch.nn.utils.weight_norm(torch.nn.ConvTranspose1d(16, 8, 4, stride=2))
    for m in (conv, convt):
        with torch.no_grad():
            m.weight_g.mul_(torch.rand_like(m.weight_g) + 0.5)
        m(torch.randn(1, m.weight_v.shape[0] if m is convt else 12, 9))  # recompute .weight from g, v
        folded = fold_weight_norm(m.weight_g, m.weight_v)
        torch.testing.assert_close(folded, m.weight.detach(), rtol=1e-6, atol=1e-7)
    assert convt.weight_g.shape == (16, 1, 1)    # dim 0 of a ConvTranspose1d weight is the INPUT channel


def test_missing_extra_keys_and_unsupported_configs_raise():
    from f5e_tts_amd._C import F5EError
    from f5e_tts_amd.vocoder_bigvgan import fold_state
    cfg = SY.bigvgan_config(256)
    sd = SY.init_bigvgan_state(cfg, 1)
    fold_state(sd, cfg)
    missing = dict(sd)
    missing.pop("resblocks.4.convs2.1.weight_v")
    with pytest.raises(F5EError, match="missing"):
        fold_state(missing, cfg)
    extra = dict(sd)
    extra["resblocks.99.convs1.0.bias"] = torch.zeros(3)
    with pytest.raises(F5EError, match="unexpected"):
        fold_state(extra, cfg)
    with_bias = dict(sd)
    with_bias["conv_post.bias"] = torch.zeros(1)       # use_bias_at_final is false: a bias is an extra key
    with pytest.raises(F5EError, match="unexpected"):
        fold_state(with_bias, cfg)
    with pytest.raises(F5EError, match="resblock"):
        fold_state(sd, dict(cfg, resblock="2"))
    with pytest.raises(F5EError, match="activation"):
        fold_state(sd, dict(cfg, activation="relu"))


def test_anti_alias_filter_matches_scipy_firwin():
    signal = pytest.importorskip("scipy.signal")
    from f5e_tts_amd.vocoder_bigvgan import kaiser_sinc_filter1d
    A = 2.285 * (6 - 1) * math.pi * (4 * 0.3) + 7.95
    beta = 0.1102 * (A - 8.7)
    assert abs(beta - 4.6638) < 2e-3
    ref = torch.from_numpy(signal.firwin(12, 0.25, window=("kaiser", beta), fs=1.0)).float()
    f = kaiser_sinc_filter1d()
    assert f.shape == (12,) and abs(float(f.sum()) - 1.0) < 1e-6
    assert float((f - ref).abs().max()) < 1e-7


def _slaney_independent(sr, n_fft, n_mels):
    """librosa.filters.mel(htk=False, norm="slaney"), written out per filter with Python floats."""
    def hz2mel(f):
        return f * 3.0 / 200.0 if f < 1000.0 else 15.0 + math.log(f / 1000.0) * 27.0 / math.log(6.4)

    def mel2hz(m):
        return m * 200.0 / 3.0 if m < 15.0 else 1000.0 * math.exp((m - 15.0) * math.log(6.4) / 27.0)

    top = hz2mel(sr / 2.0)
    pts = [mel2hz(top * i / (n_mels + 1)) for i in range(n_mels + 2)]
    freqs = [sr / 2.0 * k / (n_fft // 2) for k in range(n_fft // 2 + 1)]
    fb = torch.zeros(n_fft // 2 + 1, n_mels, dtype=torch.float64)
    for m in range(n_mels):
        lo, c, hi = pts[m], pts[m + 1], pts[m + 2]
        for k, f in enumerate(freqs):
            w = max(0.0, min((f - lo) / (c - lo), (hi - f) / (hi - c)))
            fb[k, m] = w * 2.0 / (hi - lo)
    return fb


def test_slaney_filterbank():
    from f5e_tts_amd import ops
    from f5e_tts_amd.engine import slaney_mel_filterbank
    fb = slaney_mel_filterbank(1024, 100, 24000)
    assert fb.shape == (513, 100) and fb.dtype == torch.float32
    ref = _slaney_independent(24000, 1024, 100)
    assert float((fb.double() - ref).abs().max()) < 1e-7 * float(ref.abs().max()) + 1e-12
    # hand-worked: below 1 kHz the mel points are 200/3 Hz * 44.26.../101 apart, each filter's area is 1 (slaney norm)
    top_mel = 15.0 + math.log(12.0) * 27.0 / math.log(6.4)
    step_hz = top_mel / 101 * 200.0 / 3.0
    assert abs(float(fb[:, 0].sum()) * 23.4375 - 1.0) < 0.15              # bin width 24000 / 1024 Hz
    assert int(fb[:, 0].argmax()) == round(step_hz / 23.4375)             # peak at the first centre frequency
    enorm0 = 2.0 / (2 * step_hz)
    assert abs(float(fb[:, 0].max()) - enorm0 * (1 - abs(round(step_hz / 23.4375) * 23.4375 - step_hz) / step_hz)) < 1e-6
    assert int(fb[:, 99].argmax()) > 400                                 # the last filters sit near Nyquist
    banded = ops.band_filterbank(fb)
    assert banded is not None                                            # fits the banded STFT kernel
    assert banded[0].numel() == int((fb != 0).sum()) <= 2048


def test_transposed_conv_polyphase_repack():
    """ConvTranspose1d(stride u) == 3-tap conv with N = u * C_out whose [L][u C_out] output is [L u][C_out]."""
    from f5e_tts_amd.vocoder_bigvgan import pack_conv_weight, transposed_as_conv3
    torch.manual_seed(1)
    for u, k in ((4, 8), (2, 4)):
        Cin, Cout, L = 12, 8, 10
        w, b = torch.randn(Cin, Cout, k, dtype=torch.float64), torch.randn(Cout, dtype=torch.float64)
        x = torch.randn(2, Cin, L, dtype=torch.float64)
        ref = F.conv_transpose1d(x, w, b, stride=u, padding=(k - u) // 2)
        w3, b3 = transposed_as_conv3(w, b, u)
        y = F.conv1d(x, w3.double(), b3.double(), padding=1)                 # [2, u Cout, L]
        y = y.permute(0, 2, 1).reshape(2, L * u, Cout).permute(0, 2, 1)
        torch.testing.assert_close(y, ref)
        p = pack_conv_weight(w3)
        assert p.dtype == torch.bfloat16 and p.shape == (64, 3 * 32)
        torch.testing.assert_close(p.view(64, 3, 32)[:u * Cout, :, :Cin].float(),
                                   w3.permute(0, 2, 1).to(torch.bfloat16).float())
        assert float(p.view(64, 3, 32)[u * Cout:].float().abs().sum()) == 0.0


def test_infer_cli_resolves_bigvgan():
    from f5e_tts_amd.infer import infer_cli
    args = infer_cli.build_parser().parse_args(["--vocoder_name", "bigvgan", "--load_vocoder_from_local"]) \
        if hasattr(infer_cli, "build_parser") else None
    if args is None:
        import argparse
        args = argparse.Namespace(**{k: None for k in (
            "model", "model_cfg", "ckpt_file", "vocab_file", "ref_audio", "ref_text", "gen_text", "gen_file",
            "output_dir", "output_file", "save_chunk", "remove_silence", "target_rms", "cross_fade_duration",
            "nfe_step", "cfg_strength", "sway_sampling_coef", "speed", "fix_duration", "device")},
            vocoder_name="bigvgan", load_vocoder_from_local=True)
    s = infer_cli.resolve_settings(args, {})
    assert s["vocoder_name"] == "bigvgan" and s["load_vocoder_from_local"]
    assert "bigvgan" in infer_cli.DEFAULT_VOCODER_PATH[s["vocoder_name"]]
    assert infer_cli.resolve_settings(args, {"vocoder_name": "vocos"})["vocoder_name"] == "bigvgan"   # flag > toml


def test_eval_reads_mel_spec_type_from_yaml(tmp_path):
    import yaml
    from f5e_tts_amd.eval.eval_infer_batch import yaml_mel_spec_type
    from f5e_tts_amd.train.parse_cfg import parse_model_yaml
    import os
    import f5e_tts_amd
    base = os.path.join(os.path.dirname(f5e_tts_amd.__file__), "configs", "F5TTS_v1_Base.yaml")
    with open(base) as f:
        cfg = yaml.safe_load(f)
    assert yaml_mel_spec_type(parse_model_yaml(cfg)) == "vocos"
    cfg["model"]["mel_spec"]["mel_spec_type"] = "bigvgan"
    p = tmp_path / "m.yaml"
    p.write_text(yaml.safe_dump(cfg))
    with open(p) as f:
        assert yaml_mel_spec_type(parse_model_yaml(yaml.safe_load(f))) == "bigvgan"
