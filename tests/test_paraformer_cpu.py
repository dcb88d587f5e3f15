"""eval/paraformer.py without a GPU: the am.mvn parser, the LFR restatement against hand-computed rows, checkpoint loading by
funasr's names and the refusals, the text join rules, the C ABI entries and the eval_wer flags.  Also the shared fixtures of
tests/test_paraformer_gpu.py (the tiny configuration, its seeded weights and clips) and the two margins the whole-model test
relies on, asserted here on the float64 restatement (tests/paraformer_ref.py)."""
import json
import math
import os
import re

import pytest
import torch

import paraformer_ref as PR
from f5e_tts_amd.eval import eval_wer as W
from f5e_tts_amd.eval import paraformer as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = (("f5e_lfr_cmvn_f32", 18), ("f5e_fsmn_f32", 14), ("f5e_mask_rows_f32", 7), ("f5e_cif_alpha_f32", 12),
           ("f5e_cif_fire_f32", 18), ("f5e_nar_pick", 16))

# the tiny model of the whole-model tests: every width another number, 1 + 2 encoder layers, 2 decoder layers + decoders3
TINY = dict(n_mels=8, d_model=64, heads=4, ff=128, enc_layers=3, kernel=11, dec_layers=2, dec_heads=4, dec_ff=128, dec_kernel=11,
            vocab=50)
SEED = 20261
CLIP_SAMPLES = (4800, 16000, 40000)      # about 0.3 s, 1 s and 2.5 s
MARGIN = 1e-3


def tiny_cfg():
    return P.ParaformerConfig(**TINY)


def tiny_cmvn(cfg):
    g = torch.Generator().manual_seed(SEED + 1)
    u = torch.rand(2, cfg.in_width, generator=g, dtype=torch.float64) * 2 - 1
    return -9.0 + u[0], 0.3 * (1.0 + 0.2 * u[1])


def tiny_tokens(cfg):
    return ["<blank>", "<s>", "</s>"] + [chr(0x4E00 + i) for i in range(cfg.vocab - 8)] + ["hel@@", "lo", "wor@@", "ld", "<unk>"]


def clip(samples: int, seed: int):
    """Seeded audio in [-1, 1]: two tones under noise, as f32."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(samples, dtype=torch.float64) / 16000.0
    f = 200.0 + 600.0 * torch.rand(2, generator=g, dtype=torch.float64)
    x = 0.3 * torch.sin(2 * math.pi * f[0] * t) + 0.2 * torch.sin(2 * math.pi * f[1] * t * (1 + 0.3 * t))
    return (x + 0.1 * (torch.rand(samples, generator=g, dtype=torch.float64) * 2 - 1)).float()


def tiny_clips():
    return [clip(s, SEED + 10 + i) for i, s in enumerate(CLIP_SAMPLES)]


_REF = {}


def tiny_reference():
    """The float64 restatement of every clip, computed once per process and left unchanged."""
    if not _REF:
        cfg = tiny_cfg()
        sd, (shift, scale) = P.seeded_state_dict(cfg, SEED), tiny_cmvn(cfg)
        _REF["rows"] = [PR.forward(sd, cfg, w, shift, scale) for w in tiny_clips()]
    return _REF["rows"]


# ------------------------------------------------------------------ am.mvn
def test_am_mvn_parser_on_a_hand_written_file():
    text = ("<Nnet>\n<Splice> 4 4\n[ 0 ]\n<AddShift> 4 4\n<LearnRateCoef> 0 [ -8.5 -9.25 1e-1 -10 ]\n<Rescale> 4 4\n"
            "<LearnRateCoef> 0 [ 0.125 0.25\n 0.5 2 ]\n</Nnet>\n")
    shift, scale = P.parse_am_mvn(text)
    assert shift.tolist() == [-8.5, -9.25, 0.1, -10.0] and scale.tolist() == [0.125, 0.25, 0.5, 2.0]
    with pytest.raises(Exception, match="<Rescale>"):
        P.parse_am_mvn("<Nnet>\n<AddShift> 2 2\n<LearnRateCoef> 0 [ 1 2 ]\n</Nnet>")
    with pytest.raises(Exception, match="am.mvn"):
        P.Paraformer(tiny_cfg(), cmvn=(shift, scale))                 # 4 values against lfr_m * n_mels = 56


# ------------------------------------------------------------------ LFR
def test_lfr_restatement_against_hand_computed_rows():
    def frames(T):
        return torch.arange(T, dtype=torch.float64)[:, None] * 10 + torch.arange(2, dtype=torch.float64)[None]      # frame t = (10 t, 10 t + 1)

    def rows(x):
        return [[int(v) // 10 for v in r[::2]] for r in x.tolist()]

    # T = 1: one row, frame 0 seven times.  T = 4: the 3 copies of frame 0, frames 0 .. 3.  T = 7: two rows, the second runs past the
    # end after frames 3 .. 6 and repeats frame 6
    assert rows(PR.lfr(frames(1))) == [[0, 0, 0, 0, 0, 0, 0]]
    assert rows(PR.lfr(frames(4))) == [[0, 0, 0, 0, 1, 2, 3]]
    assert rows(PR.lfr(frames(7))) == [[0, 0, 0, 0, 1, 2, 3], [3, 4, 5, 6, 6, 6, 6]]
    x = PR.lfr(frames(7))
    assert x.shape == (2, 14) and x[1, :4].tolist() == [30.0, 31.0, 40.0, 41.0]      # the channel order inside a stacked frame


def test_position_table_restatement_matches_the_models():
    assert float((PR.position_table(9, 56) - P.position_table(9, 56)).abs().max()) < 1e-14      # two spellings of one formula
    t = PR.position_table(3, 8)
    assert t[0, 0] == math.sin(1.0) and t[2, 4] == math.cos(3.0) and abs(float(t[1, 3]) - math.sin(2e-4)) < 1e-18


# ------------------------------------------------------------------ checkpoints
CONFIG_YAML = """
model: {model}
model_conf: {{ctc_weight: 0.0, lsm_weight: 0.1}}
encoder: SANMEncoder
encoder_conf: {{output_size: 64, attention_heads: 4, linear_units: 128, num_blocks: 3, input_layer: pe, kernel_size: 11,
               sanm_shfit: 0, selfattention_layer_type: {sa}}}
decoder: ParaformerSANMDecoder
decoder_conf: {{attention_heads: 4, linear_units: 128, num_blocks: {dec_blocks}, att_layer_num: 2, kernel_size: 11, sanm_shfit: 0}}
predictor: CifPredictorV2
predictor_conf: {{idim: 64, threshold: 1.0, l_order: 1, r_order: 1, tail_threshold: 0.45}}
frontend: WavFrontend
frontend_conf: {{fs: 16000, window: hamming, n_mels: 8, frame_length: 25, frame_shift: 10, lfr_m: 7, lfr_n: 6}}
"""


def write_dir(path, sd, model="Paraformer", sa="sanm", dec_blocks=2, wrap=False):
    cfg = tiny_cfg()
    shift, scale = tiny_cmvn(cfg)
    (path / "config.yaml").write_text(CONFIG_YAML.format(model=model, sa=sa, dec_blocks=dec_blocks))
    (path / "tokens.json").write_text(json.dumps(tiny_tokens(cfg), ensure_ascii=False), encoding="utf-8")
    vec = lambda v: " ".join(repr(float(x)) for x in v)
    (path / "am.mvn").write_text(f"<Nnet>\n<Splice> 56 56\n[ 0 ]\n<AddShift> 56 56\n<LearnRateCoef> 0 [ {vec(shift)} ]\n"
                                 f"<Rescale> 56 56\n<LearnRateCoef> 0 [ {vec(scale)} ]\n</Nnet>\n")
    torch.save({"state_dict": sd} if wrap else sd, path / "model.pt")
    return str(path)


@pytest.mark.parametrize("wrap", [False, True])
def test_a_directory_with_funasrs_names_loads(tmp_path, wrap):
    cfg = tiny_cfg()
    sd = P.seeded_state_dict(cfg, SEED)
    model = P.Paraformer.from_pretrained_dir(write_dir(tmp_path, sd, wrap=wrap))
    assert model.cfg == cfg and model.tokens == tiny_tokens(cfg)
    got = model.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    shift, scale = tiny_cmvn(cfg)
    assert torch.equal(model.cmvn_shift, shift.float()) and torch.equal(model.cmvn_scale, scale.float())
    for name in ("encoder.encoders0.0.self_attn.linear_q_k_v.weight", "encoder.encoders.1.self_attn.fsmn_block.weight",
                 "encoder.after_norm.bias", "predictor.cif_conv1d.weight", "predictor.cif_output.bias",
                 "decoder.decoders.1.src_attn.linear_k_v.weight", "decoder.decoders.0.feed_forward.norm.weight",
                 "decoder.decoders3.0.feed_forward.w_2.weight", "decoder.decoders3.0.norm1.bias", "decoder.after_norm.weight",
                 "decoder.output_layer.bias", "decoder.embed.0.weight"):
        assert name in got, name
    assert "decoder.decoders3.0.feed_forward.w_2.bias" not in got and "decoder.decoders.0.feed_forward.w_2.bias" not in got
    assert got["encoder.encoders0.0.self_attn.linear_q_k_v.weight"].shape == (192, 56)
    assert got["encoder.encoders0.0.norm1.weight"].shape == (56,) and got["decoder.decoders.0.feed_forward.norm.weight"].shape == (128,)


def test_refusals_name_what_they_refuse(tmp_path):
    cfg = tiny_cfg()
    sd = P.seeded_state_dict(cfg, SEED)
    for i, (kw, extra, match) in enumerate((
            (dict(), {"encoder.encoders.0.self_attn.linear_q.weight": torch.zeros(1)}, "encoder.encoders.0.self_attn.linear_q.weight"),
            (dict(model="SeacoParaformer"), {}, "SeacoParaformer"),
            (dict(), {"decoder.decoders2.0.norm1.weight": torch.zeros(64)}, "decoders2"),
            (dict(dec_blocks=3), {}, "decoders2"),
            (dict(sa="selfattn"), {}, "selfattn"))):
        d = tmp_path / f"case{i}"
        d.mkdir()
        with pytest.raises(Exception, match=match):
            P.Paraformer.from_pretrained_dir(write_dir(d, {**sd, **extra}, **kw))
    d = tmp_path / "missing"
    d.mkdir()
    with pytest.raises(Exception, match="predictor.cif_output.bias"):
        P.Paraformer.from_pretrained_dir(write_dir(d, {k: v for k, v in sd.items() if k != "predictor.cif_output.bias"}))
    with pytest.raises(Exception, match="ctc_weight"):
        P.ParaformerConfig.from_yaml_dict({"model": "Paraformer", "model_conf": {"ctc_weight": 0.3}})
    with pytest.raises(Exception, match="cap"):
        P.Paraformer(cfg).frames_of(16000 * 60 * 3)                   # 3 minutes: beyond the cap, refused by name
    assert P.Paraformer(cfg).frames_of(16000 * 60)[1] >= 1000         # the cap holds at least 60 s
    with pytest.raises(Exception, match="GPU"):
        P.Paraformer(cfg).generate(torch.zeros(1, 16000))             # no CPU path


# ------------------------------------------------------------------ text
def test_text_join_rules():
    for join in (P.join_tokens, PR.join_tokens):
        assert join(["你", "好", "世", "界"]) == "你好世界"
        assert join(["hel@@", "lo", "wor@@", "ld"]) == "hello world"
        assert join(["a", "b@@", "c@@", "d", "e"]) == "a bcd e"
        assert join(["你", "好", "hel@@", "lo", "world", "再", "见"]) == "你好hello world再见"
        assert join([]) == "" and join(["tail@@"]) == "tail"
    model = P.Paraformer(tiny_cfg(), tokens=tiny_tokens(tiny_cfg()))
    assert model.decode_ids([3, 4, -1, -1]) == "一丁"
    assert model.decode_ids([45, 46, 47, 48, 6]) == "hello world七"
    with pytest.raises(Exception, match="tokens.json"):
        P.Paraformer(tiny_cfg()).decode_ids([3])


# ------------------------------------------------------------------ the C ABI
def test_abi_entries_declared_bound_and_exported():
    from f5e_tts_amd import _C
    text = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, arity in ENTRIES:
        m = re.search(r"F5E_API int " + name + r"\((.*?)\);", text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == arity == len(_C.SIGNATURES[name]), name
        assert f"`{name}`" in doc, name
    assert "paraformer.hip" in open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "Makefile")).read()
    assert "#define F5E_ABI_VERSION 2 " in text and _C.ABI_VERSION == 2          # functions were only added


# ------------------------------------------------------------------ eval_wer
def test_eval_wer_paraformer_flags(tmp_path, capsys):
    args = W.build_parser().parse_args(["--metalst", "m", "--gen_wav_dir", "g", "--lang", "zh", "--asr", "paraformer",
                                        "--paraformer_dir", "P"])
    assert args.asr == "paraformer" and args.paraformer_dir == "P"
    assert W.build_parser().parse_args(["--metalst", "m", "--gen_wav_dir", "g", "--lang", "zh"]).asr == "wenet"     # the default stays
    with pytest.raises(SystemExit):
        W.main(["--metalst", "m", "--gen_wav_dir", "g", "--lang", "zh", "--asr", "paraformer"])
    assert "--paraformer_dir" in capsys.readouterr().err


# ------------------------------------------------------------------ the margins of the whole-model GPU test, on the reference
def test_reference_margins_of_the_tiny_model_hold_for_every_clip():
    rows = tiny_reference()
    for s, r in zip(CLIP_SAMPLES, rows):
        print(f"{s} samples: n = {r['n']}, fires = {r['fires']}, min |integrate - 1| = {r['fire_margin']:.3e}, "
              f"frac(sum alpha) = {r['frac']:.4f}, ids = {r['ids']}")
        assert r["fire_margin"] >= MARGIN and MARGIN <= r["frac"] <= 1 - MARGIN and r["fires"] == r["n"]
    assert max(r["n"] for r in rows) >= 3


def test_cif_restatement_on_hand_cases():
    h = torch.tensor([[1.0, 2.0], [10.0, 20.0], [100.0, 200.0]], dtype=torch.float64)
    out, pos, _ = PR.cif(torch.tensor([0.5, 0.5, 0.25, 0.45], dtype=torch.float64), h)
    assert pos == [1] and out.tolist() == [[5.5, 11.0]]                            # a fire at exactly the threshold, no remainder
    out, pos, _ = PR.cif(torch.tensor([0.75, 0.75, 0.25, 0.45], dtype=torch.float64), h)
    assert pos == [1, 3] and out[0].tolist() == [0.75 + 2.5, 1.5 + 5.0]            # 0.75 h0 + 0.25 h1; the remainder 0.5 h1 goes on
    assert out[1].tolist() == [5.0 + 25.0, 10.0 + 50.0]                            # 0.5 h1 + 0.25 h2 + 0.25 * 0 (the tail fires)
    assert PR.cif_alpha(torch.zeros(3, dtype=torch.float64))[1] == 1               # 3 * 0.5 + 0.45
