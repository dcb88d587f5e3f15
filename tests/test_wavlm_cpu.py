"""WavLM upstream, the parts that need no GPU: the plain-torch restatement (tests/wavlm_ref.py) against the fixture made from
``transformers.WavLMModel`` (tests/golden/wavlm.npz, tests/golden/make_wavlm_golden.py), the name converter, the weight-norm fold,
the bucket table, the frame-count rule, the ``eval_sim`` audio route on stubs, the refusals and the C ABI entries.

Restatement gate: float64 against every fixture hidden state, relative L2 < 1e-5 -- the fixture is fp32, 7e-7 from its own
float64 run, and the gate is 14 times that."""
import json
import os
import re

import numpy as np
import pytest
import torch

import wavlm_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "wavlm.npz")
CASES = (400, 23457, 40000)
REF_GATE = 1e-5
ENTRIES = (("f5e_wav_norm", 15), ("f5e_wav_norm_partials", 3), ("f5e_wavlm_conv0", 13), ("f5e_layernorm_gelu", 10),
           ("f5e_wavlm_posconv", 14), ("f5e_wavlm_gate", 11), ("f5e_relbias_attn_f32", 18))


def tiny_cfg():
    from f5e_tts_amd.eval.wavlm import WavLMConfig
    return WavLMConfig(conv_dim=(32,) * 7, encoder_embed_dim=64, encoder_layers=3, encoder_attention_heads=4,
                       encoder_ffn_embed_dim=128)


_gold = {}


def gold():
    """(fixture arrays, fairseq-named float32 state dict), loaded once and shared."""
    if not _gold:
        from f5e_tts_amd.eval.wavlm import convert_hf_state_dict
        z = np.load(GOLD)
        _gold["z"] = {k: z[k] for k in z.files}
        _gold["sd"] = convert_hf_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")})
    return _gold["z"], _gold["sd"]


def tiny_model():
    from f5e_tts_amd.eval.wavlm import WavLM
    _, sd = gold()
    model = WavLM(tiny_cfg())
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert missing == ["mask_emb"] and not unexpected       # the fixture's model has no masking, so no mask embedding
    return model


# ---- restatement against the fixture ----

@pytest.mark.parametrize("S", CASES)
def test_restatement_matches_the_fixture(S):
    z, sd = gold()
    hs, frames = WR.forward(WR.cast(sd, torch.float64), tiny_cfg(), torch.from_numpy(z[f"wav_{S}"]).double()[None])
    want = z[f"hs_{S}"]
    assert frames == [want.shape[1]] and hs.shape[0] == want.shape[0] == 4
    for l in range(4):
        err = WR.rel_l2(hs[l, 0], want[l])
        print(f"S={S} hidden state {l}: rel L2 {err:.3e}")
        assert err < REF_GATE


def test_restatement_matches_the_padded_pair():
    z, sd = gold()
    a, b = torch.from_numpy(z["wav_40000"]).double(), torch.from_numpy(z["wav_23457"]).double()
    wav = torch.stack([a, torch.nn.functional.pad(b, (0, 40000 - 23457))])
    hs, frames = WR.forward(WR.cast(sd, torch.float64), tiny_cfg(), wav, [40000, 23457])
    assert frames == z["pair_frames"].tolist() == [124, 73]
    for row in range(2):
        for l in range(4):
            err = WR.rel_l2(hs[l, row, :frames[row]], z[f"hs_pair_{row}"][l])
            print(f"pair row {row} hidden state {l}: rel L2 {err:.3e}")
            assert err < REF_GATE
    assert float(hs[:, 1, 73:].abs().max()) == 0.0


# ---- converter, fold, table, frame counts ----

def test_convert_hf_state_dict_round_trips_names_and_shapes():
    from f5e_tts_amd.eval.wavlm import WavLM, convert_hf_state_dict
    z, sd = gold()
    own = WavLM(tiny_cfg()).state_dict()
    assert set(own) - set(sd) == {"mask_emb"} and not set(sd) - set(own)
    assert all(tuple(sd[k].shape) == tuple(own[k].shape) for k in sd)
    assert len(sd) == sum(k.startswith("w/") for k in z)
    assert "encoder.layers.0.self_attn.relative_attention_bias.weight" in sd and "encoder.layers.2.self_attn.grep_a" in sd
    assert "encoder.layers.1.self_attn.relative_attention_bias.weight" not in sd
    extra = convert_hf_state_dict({"wavlm.masked_spec_embed": torch.zeros(64), "encoder.pos_conv_embed.conv.weight_g": torch.zeros(1, 1, 128)})
    assert set(extra) == {"mask_emb", "encoder.pos_conv.0.weight_g"}
    with pytest.raises(KeyError, match="adapter"):
        convert_hf_state_dict({"adapter.layers.0.conv.weight": torch.zeros(1)})


def test_from_sim_checkpoint_takes_the_feature_extract_slice():
    from f5e_tts_amd._C import F5EError
    from f5e_tts_amd.eval.wavlm import WavLM
    _, sd = gold()
    state = {"feature_extract.model." + k: v for k, v in sd.items()}
    state["feature_extract.model.mask_emb"] = torch.ones(64)
    state["layer1.conv.weight"] = torch.zeros(3)           # the head's keys are not this module's business
    model = WavLM.from_sim_checkpoint(state, tiny_cfg())
    assert torch.equal(model.encoder.layers[1].fc1.weight, sd["encoder.layers.1.fc1.weight"]) and float(model.mask_emb.sum()) == 64
    with pytest.raises(F5EError, match="feature_extract.model."):
        WavLM.from_sim_checkpoint({"layer1.conv.weight": torch.zeros(3)}, tiny_cfg())


def test_weight_norm_fold_equals_the_parametrised_weight():
    from f5e_tts_amd.eval.wavlm import fold_weight_norm
    torch.manual_seed(3)
    conv = torch.nn.utils.parametrizations.weight_norm(torch.nn.Conv1d(64, 64, 128, padding=64, groups=16).double(), name="weight", dim=2)
    with torch.no_grad():
        conv.parametrizations.weight.original0.mul_(1.0 + 0.3 * torch.randn(1, 1, 128, dtype=torch.float64))
    g, v = conv.parametrizations.weight.original0, conv.parametrizations.weight.original1
    assert g.shape == (1, 1, 128)
    w = fold_weight_norm(g.float(), v.float())
    assert w.dtype == torch.float64 and WR.rel_l2(w, conv.weight) < 1e-7
    assert WR.rel_l2(WR.fold_wn(g, v), conv.weight) < 1e-14


@pytest.mark.parametrize("Tt", (1, 80, 81, 124, 900))
def test_bias_table_equals_the_grid_bias_on_every_diagonal(Tt):
    from f5e_tts_amd.eval.wavlm import bias_table
    emb = torch.randn(320, 4, generator=torch.Generator().manual_seed(Tt))
    table, grid = bias_table(emb, Tt), WR.compute_bias(emb, Tt)
    assert table.shape == (4, 2 * Tt - 1) and grid.shape == (4, Tt, Tt)
    i, j = torch.meshgrid(torch.arange(Tt), torch.arange(Tt), indexing="ij")
    assert torch.equal(table[:, j - i + Tt - 1], grid)


def test_frame_count_rule():
    from f5e_tts_amd.eval.wavlm import WavLM, frame_counts
    cfg = tiny_cfg()
    assert [frame_counts(S, cfg)[-1] for S in (399, 400, 23457, 40000)] == [0, 1, 73, 124]
    assert WavLM(cfg).min_samples() == 400
    transformers = pytest.importorskip("transformers")
    hf = transformers.WavLMModel(transformers.WavLMConfig(
        hidden_size=16, num_hidden_layers=1, num_attention_heads=1, intermediate_size=16, conv_dim=(4,) * 7,
        conv_kernel=cfg.conv_kernel, conv_stride=cfg.conv_stride, feat_extract_norm="layer", do_stable_layer_norm=True,
        num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4))
    for S in (400, 401, 719, 720, 23457, 40000):
        assert frame_counts(S, cfg)[-1] == int(hf._get_feat_extract_output_lengths(S))


# ---- refusals ----

def test_other_configurations_are_refused_by_field_name():
    from f5e_tts_amd._C import F5EError
    from f5e_tts_amd.eval.wavlm import WavLM, WavLMConfig
    for field, value in (("extractor_mode", "default"), ("layer_norm_first", False), ("normalize", False),
                         ("encoder_attention_heads", 3), ("conv_stride", (4, 2, 2, 2, 2, 2, 2))):
        kw = dict(conv_dim=(32,) * 7, encoder_embed_dim=64, encoder_layers=1, encoder_attention_heads=4, encoder_ffn_embed_dim=128)
        kw[field] = value
        with pytest.raises(F5EError, match=field if field != "conv_stride" else "conv_kernel"):
            WavLM(WavLMConfig(**kw))
    with pytest.raises(F5EError, match="group-norm"):
        WavLM(WavLMConfig(extractor_mode="default", encoder_layers=1))
    with pytest.raises(F5EError, match="post-LN"):
        WavLM(WavLMConfig(layer_norm_first=False, encoder_layers=1))


def test_cpu_tensors_and_training_are_refused():
    from f5e_tts_amd._C import F5EError
    model = tiny_model()
    with pytest.raises(F5EError, match="no CPU path"):
        model.extract(torch.zeros(1, 4000))
    with pytest.raises(F5EError, match="no CPU path"):
        model([torch.zeros(4000)])
    with pytest.raises(F5EError, match="float32 tensor"):
        model.extract(torch.zeros(4000))
    with pytest.raises(F5EError, match="eval mode only"):
        model.train()
    assert model.workspace_bytes(2, 40000) > 0 and model._plan(2, 40000)["qkv"][1] == (2 * 124, 192)
    T, need, pitch = model._geometry(40000)
    counts = WR.frame_counts(40000, model.cfg)
    assert T == 124 and all(n <= c and n <= p for n, c, p in zip(need, counts, pitch))
    assert all(pitch[l - 1] == model.cfg.conv_stride[l] * pitch[l] for l in range(1, 7))


# ---- eval_sim without --feat_dir, on stubs ----

class StubUpstream:
    """Two 'hidden states' of width 8: frames of 160 samples, their mean and their mean absolute value repeated."""

    def __init__(self):
        self.calls = []

    def __call__(self, wavs):
        self.calls.append([int(w.numel()) for w in wavs])
        frames = [int(w.numel()) // 160 for w in wavs]
        T = max(frames)
        hs = torch.zeros(2, len(wavs), T, 8)
        for b, w in enumerate(wavs):
            f = w[:frames[b] * 160].reshape(frames[b], 160)
            hs[0, b, :frames[b]] = f[:, :8] + 1.0
            hs[1, b, :frames[b]] = f.abs().mean(1, keepdim=True)
        return {"hidden_states": list(hs), "lengths": torch.tensor(frames, dtype=torch.int32)}


class StubEncoder:
    def __call__(self, hs, lengths):
        return torch.stack([hs[0, b, :int(n)].mean(0) for b, n in enumerate(lengths)])


def test_eval_sim_audio_route_and_dump_feats_on_stubs(tmp_path, capsys):
    from f5e_tts_amd.eval import eval_sim
    from f5e_tts_amd.infer.utils_infer import save_wav
    gen, prompts, feats = tmp_path / "gen", tmp_path / "prompts", tmp_path / "feats"
    gen.mkdir(), prompts.mkdir()
    rng = np.random.default_rng(11)
    lines = []
    for i, (ng, npr, sr) in enumerate([(4000, 2400, 16000), (3000, 6000, 24000)]):
        save_wav(str(gen / f"utt{i}.wav"), 0.3 * rng.standard_normal(ng), sr)
        save_wav(str(prompts / f"prompt{i}.wav"), 0.3 * rng.standard_normal(npr), sr)
        lines.append(f"utt{i}|some prompt text|prompts/prompt{i}.wav|the truth {i}")
    (tmp_path / "meta.lst").write_text("\n".join(lines) + "\n")
    args = ["--metalst", str(tmp_path / "meta.lst"), "--gen_wav_dir", str(gen), "--device", "cpu"]
    up = StubUpstream()
    sim = eval_sim.main(args + ["--dump_feats", str(feats)], model=StubEncoder(), upstream=up)
    assert up.calls == [[4000, 2400], [2000, 4000]]            # one ragged pair per utterance, 24 kHz resampled to 16 kHz
    assert f"SIM: {sim:.5f}" in capsys.readouterr().out
    audio = json.load(open(gen / "_sim_results.json"))
    assert [r["wav"] for r in audio] == ["utt0", "utt1"]
    assert sorted(os.listdir(feats)) == ["prompt0.npy", "prompt1.npy", "utt0.npy", "utt1.npy"]
    assert np.load(feats / "utt0.npy").shape == (2, 25, 8) and np.load(feats / "prompt1.npy").shape == (2, 25, 8)
    sim2 = eval_sim.main(args + ["--feat_dir", str(feats)], model=StubEncoder())
    again = json.load(open(gen / "_sim_results.json"))
    assert abs(sim2 - sim) < 1e-6 and all(abs(a["sim"] - b["sim"]) < 1e-6 for a, b in zip(audio, again))
    with pytest.raises(SystemExit, match="dump_feats"):
        eval_sim.main(args + ["--feat_dir", str(feats), "--dump_feats", str(feats)], model=StubEncoder())


# ---- the C ABI ----

def test_abi_entries_declared_bound_and_exported():
    from f5e_tts_amd import _C
    text = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _C.lib()
    for name, arity in ENTRIES:
        m = re.search(r"F5E_API int " + name + r"\((.*?)\);", text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == arity == len(_C.SIGNATURES[name])
        assert hasattr(lib, name) and f"`{name}`" in doc
    assert "wavlm.hip" in open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "Makefile")).read()
