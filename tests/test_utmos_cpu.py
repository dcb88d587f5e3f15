"""UTMOS predictor, the parts that need no GPU: the plain-torch restatement (tests/utmos_ref.py) against the fixture made from
``transformers.Wav2Vec2Model`` and ``torch.nn.LSTM`` (tests/golden/utmos.npz, tests/golden/make_utmos_golden.py), the hand-loop
LSTM against ``torch.nn.LSTM``, the name converter, the refusals, the bias fold, the C ABI entries and the ``eval_utmos`` driver on
a stub predictor.

Restatement gate: float64 against the fp32 fixture, |got - want| <= 2e-5 + 1e-4 |want| element by element (the project's
rtol 1e-4 / atol 2e-5 for fp32 fixtures)."""
import json
import os
import re

import numpy as np
import pytest
import torch

import utmos_ref as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "utmos.npz")
CASES = (400, 23457, 40000)
FRAMES = {400: 1, 23457: 73, 40000: 124}
RTOL, ATOL = 1e-4, 2e-5
ENTRIES = (("f5e_w2v_conv0_gn", 21), ("f5e_w2v_conv0_gn_partials", 4), ("f5e_lstm_f32", 11), ("f5e_score_mean", 13))
F64 = torch.float64


def tiny_cfg():
    from f5e_tts_amd.eval.wav2vec2 import Wav2Vec2Config
    return Wav2Vec2Config(conv_dim=(32,) * 7, encoder_embed_dim=64, encoder_layers=3, encoder_attention_heads=4,
                          encoder_ffn_embed_dim=128)


_gold = {}


def gold():
    """(fixture arrays, float32 state dict in the module's own names), loaded once and shared."""
    if not _gold:
        from f5e_tts_amd.eval.wav2vec2 import convert_hf_state_dict
        z = np.load(GOLD)
        _gold["z"] = {k: z[k] for k in z.files}
        w = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}
        sd = {k: v for k, v in w.items() if not k.startswith("wav2vec2.")}
        sd.update({"wav2vec2." + k: v for k, v in convert_hf_state_dict({k: v for k, v in w.items() if k.startswith("wav2vec2.")}).items()})
        _gold["sd"] = sd
    return _gold["z"], _gold["sd"]


def tiny_model():
    from f5e_tts_amd.eval.utmos import UTMOS22Strong
    z, _ = gold()
    raw = {k[2:]: torch.from_numpy(z[k]) for k in z if k.startswith("w/")}            # HF names: from_checkpoint converts them
    return UTMOS22Strong.from_checkpoint(raw, cfg=tiny_cfg(), emb_dim=16, lstm_hidden=32, proj_hidden=128)


def close(name, got, want):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    over = float(((got - want).abs() - (ATOL + RTOL * want.abs())).max())
    print(f"{name}: max |diff| {float((got - want).abs().max()):.3e}, rel L2 {UR.rel_l2(got, want):.3e}")
    assert got.shape == want.shape and over <= 0.0, name


# ---- restatement against the fixture ----

@pytest.mark.parametrize("S", CASES)
def test_restatement_matches_the_fixture(S):
    z, sd = gold()
    r = UR.predict(UR.cast(sd, F64), tiny_cfg(), torch.from_numpy(z[f"wav_{S}"]).double()[None])
    assert r["frames"] == [FRAMES[S]]
    close(f"S={S} last hidden state", r["hidden"][0], z[f"hidden_{S}"])
    close(f"S={S} BiLSTM output", r["blstm"][0], z[f"blstm_{S}"])
    close(f"S={S} frame scores", r["frame_scores"][0], z[f"frame_{S}"])
    close(f"S={S} score", r["scores"][0], z[f"score_{S}"])


def test_fixture_head_is_alive():
    z, _ = gold()
    for S in CASES[1:]:
        assert float(np.std(z[f"frame_{S}"], ddof=1)) >= 0.05 and float(np.abs(z[f"blstm_{S}"]).max()) < 0.99


def test_restated_group_norm_layer_matches_torch_and_handles_one_frame():
    torch.manual_seed(2)
    w, g, beta = torch.randn(8, 1, 10, dtype=F64), 1 + 0.1 * torch.randn(8, dtype=F64), 0.1 * torch.randn(8, dtype=F64)
    wav = torch.randn(2, 300, dtype=F64)
    got = UR.conv0_gn(wav, w, None, g, beta, [300, 163])
    for b, n in ((0, 300), (1, 163)):
        y = torch.nn.functional.conv1d(wav[b:b + 1, None, :n], w, stride=5)
        want = torch.nn.functional.gelu(torch.nn.functional.group_norm(y, 8, g, beta, 1e-5))[0].t()
        assert float((got[b, :want.shape[0]] - want).abs().max()) < 1e-12 and float(got[b, want.shape[0]:].abs().max() if n < 300 else 0.0) == 0.0
    one = UR.conv0_gn(wav[:1, :14], w, None, g, beta)                          # one frame: the normalised term is zero
    assert one.shape == (1, 1, 8) and torch.equal(one[0, 0], torch.nn.functional.gelu(beta))


# ---- the hand-loop LSTM ----

@pytest.mark.parametrize("bidirectional", (False, True))
def test_hand_loop_lstm_matches_torch_lstm(bidirectional):
    torch.manual_seed(3)
    ref = torch.nn.LSTM(12, 8, batch_first=True, bidirectional=bidirectional).double()
    sd = {"blstm." + k: v.detach() for k, v in ref.state_dict().items()}
    x = torch.randn(3, 9, 12, dtype=F64)
    lens = [9, 4, 1]
    with torch.no_grad():
        want, _ = ref(x)
        got = UR.lstm(x, sd, lengths=None, bidirectional=bidirectional)
        assert float((got - want).abs().max()) < 1e-12
        packed = torch.nn.utils.rnn.pack_padded_sequence(x, lens, batch_first=True)
        want, _ = torch.nn.utils.rnn.pad_packed_sequence(ref(packed)[0], batch_first=True, total_length=9)
        junk = x.clone()
        junk[1, 4:], junk[2, 1:] = 1e4, 1e4                                    # the padding is never read
        got = UR.lstm(junk, sd, lengths=lens, bidirectional=bidirectional)
    assert float((got - want).abs().max()) < 1e-12 and float(got[1, 4:].abs().max()) == 0.0
    if bidirectional:                                                          # the reversed ragged row starts at ITS last frame
        with torch.no_grad():
            one, _ = ref(x[1:2, :4])
        assert float((got[1, :4] - one[0]).abs().max()) < 1e-12


# ---- converter, refusals, fold ----

def test_convert_hf_state_dict_covers_every_fixture_key():
    from f5e_tts_amd.eval.utmos import UTMOS22Strong
    from f5e_tts_amd.eval.wav2vec2 import Wav2Vec2, convert_hf_state_dict
    z, sd = gold()
    own = Wav2Vec2(tiny_cfg()).state_dict()
    up = {k[len("wav2vec2."):]: v for k, v in sd.items() if k.startswith("wav2vec2.")}
    assert set(up) == set(own) and all(tuple(up[k].shape) == tuple(own[k].shape) for k in up)
    assert len(sd) == sum(k.startswith("w/") for k in z)
    assert "feature_extractor.conv_layers.0.2.weight" in up and "encoder.pos_conv.0.weight_g" in up
    model = tiny_model()
    assert set(model.state_dict()) == set(sd)
    assert torch.equal(model.blstm.weight_hh_l0_reverse, sd["blstm.weight_hh_l0_reverse"])
    assert torch.equal(model.wav2vec2.encoder.layers[2].fc2.weight, sd["wav2vec2.encoder.layers.2.fc2.weight"])
    extra = convert_hf_state_dict({"wav2vec2.masked_spec_embed": torch.zeros(64), "encoder.pos_conv_embed.conv.weight_g": torch.zeros(1, 1, 128)})
    assert set(extra) == {"encoder.pos_conv.0.weight_g"}
    for bad in ("adapter.layers.0.conv.weight", "feature_extractor.conv_layers.1.layer_norm.weight"):
        with pytest.raises(KeyError, match="no counterpart"):
            convert_hf_state_dict({bad: torch.zeros(1)})
    from f5e_tts_amd._C import F5EError
    with pytest.raises(F5EError, match="lacks"):
        UTMOS22Strong.from_checkpoint({"domain_emb": torch.zeros(1, 16)}, cfg=tiny_cfg(), emb_dim=16, lstm_hidden=32, proj_hidden=128)


def test_config_refusals_name_the_field():
    from f5e_tts_amd._C import F5EError
    from f5e_tts_amd.eval.wav2vec2 import Wav2Vec2Config
    from f5e_tts_amd.eval.wavlm import WavLMConfig
    Wav2Vec2Config().check()
    for field, value in (("extractor_mode", "layer_norm"), ("layer_norm_first", True), ("normalize", True),
                         ("conv_dim", (512,) * 6 + (256,)), ("conv_kernel", (8, 3, 3, 3, 3, 2, 2)), ("conv_stride", (5, 4, 2, 2, 2, 2, 2)),
                         ("encoder_attention_heads", 16), ("conv_pos_groups", 7), ("encoder_ffn_embed_dim", 3071)):
        with pytest.raises(F5EError, match=f"Wav2Vec2: {field} = "):
            Wav2Vec2Config(**{field: value}).check()
    for field, value in (("extractor_mode", "default"), ("layer_norm_first", False)):     # WavLM goes on refusing the base family
        with pytest.raises(F5EError, match=f"WavLM: {field} = "):
            WavLMConfig(**{field: value}).check()


def test_bias_fold_equals_the_concatenated_form():
    from f5e_tts_amd.eval.utmos import fold_lstm
    torch.manual_seed(5)
    D, E, H = 24, 6, 32
    blstm = torch.nn.LSTM(D + 2 * E, H, batch_first=True, bidirectional=True).double()
    const = torch.randn(2 * E, dtype=F64)
    w_ih, bias, w_hh, Hp = fold_lstm(blstm, const, D)
    assert Hp == 64 and w_ih.shape == (8 * Hp, D) and bias.shape == (8 * Hp,) and w_hh.shape == (2, 4 * Hp, Hp)
    x = torch.randn(2, 7, D, dtype=F64)
    sd = {"blstm." + k: v.detach() for k, v in blstm.state_dict().items()}
    with torch.no_grad():
        want = UR.lstm(torch.cat([x, const.expand(2, 7, -1)], -1), sd)
        got = UR.lstm_recurrence(torch.nn.functional.linear(x, w_ih, bias), w_hh).view(2, 7, 2, Hp)
    assert float(got[..., H:].abs().max()) == 0.0                              # the padding units stay exactly zero
    assert float((got[..., :H].reshape(2, 7, 2 * H) - want).abs().max()) < 1e-12
    for d, sfx in enumerate(("", "_reverse")):                                  # the fold itself, gate block by gate block
        wi = getattr(blstm, "weight_ih_l0" + sfx).detach()
        b = wi[:, D:] @ const + getattr(blstm, "bias_ih_l0" + sfx).detach() + getattr(blstm, "bias_hh_l0" + sfx).detach()
        assert float((bias.view(2, 4, Hp)[d, :, :H] - b.view(4, H)).abs().max()) < 1e-13


def test_pack_lstm_weight_layout():
    from f5e_tts_amd import ops
    from f5e_tts_amd._C import F5EError
    w = torch.arange(2 * 256 * 64, dtype=torch.float32).view(2, 256, 64)
    p = ops.pack_lstm_weight(w)
    assert p.shape == (2, 64, 1, 64, 4) and p.is_contiguous()
    assert float(p[1, 5, 0, 7, 2]) == float(w[1, 2 * 64 + 5, 7])
    for bad in (torch.zeros(2, 128, 32), torch.zeros(3, 256, 64), torch.zeros(2, 256, 65), torch.zeros(1, 4 * 1088, 1088)):
        with pytest.raises(F5EError, match="pack_lstm_weight"):
            ops.pack_lstm_weight(bad)


def test_ops_refuse_before_any_launch():
    """CPU tensors and bad shapes raise F5EError from the wrappers: nothing reaches the library."""
    from f5e_tts_amd import ops
    from f5e_tts_amd._C import F5EError
    w = ops.pack_lstm_weight(torch.zeros(2, 256, 64))
    with pytest.raises(F5EError):
        ops.lstm_f32(torch.zeros(6, 512), w, None, torch.zeros(2, 3, 128), torch.zeros(2, 2, 64))
    with pytest.raises(F5EError, match="do not fit"):
        ops.lstm_f32(torch.zeros(6, 512), w, None, torch.zeros(2, 3, 64), torch.zeros(2, 2, 64))
    with pytest.raises(F5EError, match="do not fit"):
        ops.lstm_f32(torch.zeros(17, 512), w, None, torch.zeros(17, 1, 128), torch.zeros(2, 17, 64))
    with pytest.raises(F5EError):
        ops.score_mean(torch.zeros(6, 8), torch.zeros(8), None, None, torch.zeros(2), 2)
    with pytest.raises(F5EError, match="w2v_conv0_gn"):
        ops.w2v_conv0_gn(torch.zeros(1, 9), torch.zeros(4, 10), None, torch.zeros(4), torch.zeros(4), None, torch.zeros(1, 1, 4),
                         torch.zeros(8))


# ---- the C ABI ----

def test_abi_entries_declared_bound_and_exported():
    from f5e_tts_amd import _C
    text = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    emap = open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "exports.map")).read()
    assert "f5e_*" in emap                                            # the version script exports the whole f5e_ prefix
    lib = _C.lib()
    for name, arity in ENTRIES:
        m = re.search(r"F5E_API int " + name + r"\((.*?)\);", text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == arity == len(_C.SIGNATURES[name]), name
        assert hasattr(lib, name) and f"`{name}`" in doc, name
    assert "utmos.hip" in open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "Makefile")).read()
    assert "#define F5E_ABI_VERSION 2 " in text and _C.ABI_VERSION == 2          # functions were only added


# ---- the driver on a stub ----

class StubPredictor:
    """score = 1 + the mean of |wave| + sr / 1e6: depends on the file and on the sample rate it was read at."""
    def __call__(self, wave, sr):
        assert wave.ndim == 2 and wave.shape[0] == 1
        return 1.0 + wave.abs().mean(1) + sr / 1e6


def test_run_utmos_writes_the_reference_format(tmp_path, capsys):
    from f5e_tts_amd.eval import eval_utmos
    from f5e_tts_amd.infer.utils_infer import save_wav
    (tmp_path / "sub").mkdir()
    t = np.arange(4000) / 16000.0
    save_wav(str(tmp_path / "b.wav"), 0.5 * np.sin(2 * np.pi * 220 * t), 16000)
    save_wav(str(tmp_path / "sub" / "a.wav"), 0.25 * np.sin(2 * np.pi * 330 * t), 24000)
    (tmp_path / "notes.txt").write_text("not audio")
    mean = eval_utmos.main(["--audio_dir", str(tmp_path), "--ext", "wav", "--device", "cpu"], predictor=StubPredictor())
    lines = (tmp_path / "_utmos_results.jsonl").read_text().split("\n")
    rows = [json.loads(l) for l in lines[:2]]
    assert [r["wav"] for r in rows] == ["b", "a"]                      # sorted by path: b.wav before sub/a.wav
    assert all(set(r) == {"wav", "utmos"} for r in rows)
    assert abs(rows[0]["utmos"] - (1 + 2 / np.pi * 0.5 + 0.016)) < 1e-3 and abs(rows[1]["utmos"] - (1 + 2 / np.pi * 0.25 + 0.024)) < 1e-3
    assert lines[2] == "" and lines[3] == f"UTMOS: {mean:.4f}" and lines[4:] == [""]
    assert abs(mean - (rows[0]["utmos"] + rows[1]["utmos"]) / 2) < 1e-9
    assert f"UTMOS: {mean:.4f}" in capsys.readouterr().out


def test_run_utmos_mixes_down_to_mono(tmp_path):
    import wave as wave_mod
    from f5e_tts_amd.eval import eval_utmos
    pcm = np.zeros((1000, 2), "<i2")
    pcm[:, 0], pcm[:, 1] = 16384, -16384                                # the channels cancel
    with wave_mod.open(str(tmp_path / "s.wav"), "wb") as w:
        w.setnchannels(2), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes(pcm.tobytes())
    assert abs(eval_utmos.run_utmos(str(tmp_path), "wav", StubPredictor(), "cpu") - 1.016) < 1e-6


def test_run_utmos_batches_16k_files_and_keeps_the_order(tmp_path):
    from f5e_tts_amd.eval import eval_utmos
    from f5e_tts_amd.infer.utils_infer import save_wav

    class Batched(StubPredictor):
        calls = []

        def predict(self, rows, n):                                    # padded rows + lengths, as UTMOS22Strong.predict takes them
            self.calls.append(list(n))
            return torch.stack([1.0 + rows[b, :n[b]].abs().mean() + 0.016 for b in range(len(n))])

    for i, (name, sr) in enumerate((("a", 16000), ("b", 16000), ("c", 24000), ("d", 16000))):
        save_wav(str(tmp_path / f"{name}.wav"), np.full(500 + 100 * i, 0.1 * (i + 1)), sr)
    one = eval_utmos.run_utmos(str(tmp_path), "wav", StubPredictor(), "cpu")
    single = (tmp_path / "_utmos_results.jsonl").read_text()
    stub = Batched()
    two = eval_utmos.run_utmos(str(tmp_path), "wav", stub, "cpu", batch=2)
    rows = [json.loads(l) for l in (tmp_path / "_utmos_results.jsonl").read_text().split("\n")[:4]]
    assert stub.calls == [[500, 600], [800]] and [r["wav"] for r in rows] == ["a", "b", "c", "d"]      # c (24 kHz) goes alone
    assert abs(one - two) < 1e-6 and all(abs(r["utmos"] - json.loads(l)["utmos"]) < 1e-6 for r, l in zip(rows, single.split("\n")))


def test_run_utmos_empty_directory_and_missing_checkpoint(tmp_path):
    from f5e_tts_amd.eval import eval_utmos
    assert eval_utmos.run_utmos(str(tmp_path), "wav", StubPredictor(), "cpu") == 0
    assert (tmp_path / "_utmos_results.jsonl").read_text() == "\nUTMOS: 0.0000\n"
    with pytest.raises(SystemExit, match="--utmos_ckpt"):
        eval_utmos.main(["--audio_dir", str(tmp_path)])
