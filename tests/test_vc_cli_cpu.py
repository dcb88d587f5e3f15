"""Host side of command-line voice conversion: the resampling plan shared by the host and device routes, the new C-ABI entry,
the source chunk planner, PPG / codebook models through ``load_model`` and the new ``infer_cli`` flags.  No GPU."""
import json
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")

RATIOS = [(24000, 16000), (16000, 24000), (44100, 24000), (44100, 16000), (48000, 16000), (22050, 24000), (8000, 24000)]


@pytest.mark.parametrize("orig_freq,new_freq", RATIOS)
def test_resample_plan_agrees_with_the_filter_bank(orig_freq, new_freq):
    from f5e_tts_amd.infer import audio as A
    bank, width, orig, new = A.sinc_resample_kernel(orig_freq, new_freq)
    assert A.resample_plan(orig_freq, new_freq) == (orig, new, width, 2 * width + orig)
    assert bank.shape == (new, 1, 2 * width + orig) and math.gcd(orig, new) == 1
    assert orig * new_freq == new * orig_freq


def test_host_resample_is_unchanged_by_the_shared_plan():
    """The host route keeps its arithmetic: the bank restated here from the published formula, then F.conv1d."""
    from f5e_tts_amd.infer import audio as A
    x = torch.randn(2, 1000, generator=torch.Generator().manual_seed(0))
    orig, new, lpw, rolloff = 3, 2, 6, 0.99
    base = min(orig, new) * rolloff
    width = math.ceil(lpw * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None, None] / new + idx
    t = (t * base).clamp_(-lpw, lpw)
    win = torch.cos(t * math.pi / lpw / 2) ** 2
    t = t * math.pi
    k = (torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), t.sin() / t) * win * (base / orig)).float()
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (width, width + orig))[:, None], k, stride=orig)
    y = y.transpose(1, 2).reshape(2, -1)[:, :math.ceil(new * 1000 / orig)]
    assert torch.equal(A.resample(x, 24000, 16000), y)
    assert A.resample(x, 16000, 16000) is x


def test_resample_entry_is_declared_exported_and_bound():
    import ctypes as C
    from f5e_tts_amd import _C
    text = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    m = re.search(r"F5E_API int f5e_resample\((.*?)\);", text, flags=re.S)
    assert m, "f5e_resample is not declared in f5e_abi.h"
    assert len(m.group(1).split(",")) == 12 == len(_C.SIGNATURES["f5e_resample"])
    lib = _C.lib()
    assert hasattr(lib, "f5e_resample") and lib.f5e_abi_version() == _C.ABI_VERSION == 2
    assert "resample.hip" in open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "Makefile")).read()
    # argument checks return before any launch: 3 : 2, width 10, n = 9 -> n_out = 6
    p = C.c_void_p(8)
    call = lambda ld_x, orig, new, ld_y, n, n_out: lib.f5e_resample(None, p, ld_x, p, orig, new, 10, p, ld_y, 1, n, n_out)  # noqa: E731
    assert call(9, 0, 2, 6, 9, 6) == -1 and call(9, 3, 0, 6, 9, 6) == -1 and call(9, 3, 2, 6, 0, 0) == -1
    assert call(9, 3, 2, 7, 9, 7) == -1 and b"ceil" in lib.f5e_last_error()
    assert call(8, 3, 2, 6, 9, 6) == -1 and call(9, 3, 2, 5, 9, 6) == -1
    assert lib.f5e_resample(None, None, 9, p, 3, 2, 10, p, 6, 1, 9, 6) == -1


def test_device_route_raises_on_cpu_tensors():
    from f5e_tts_amd import _C, ops
    from f5e_tts_amd.infer import audio as A
    x = torch.zeros(1, 100)
    with pytest.raises(_C.F5EError):
        ops.resample(x, 24000, 16000)
    with pytest.raises(_C.F5EError):
        A.resample_device(x, 24000, 16000)
    assert ops.resample(x, 16000, 16000) is x


# ------------------------------------------------------------------ plan_vc_chunks

def check_plan(pieces, n, sr, ref_secs, max_total):
    assert pieces[0][0] == 0 and pieces[-1][1] == n
    for (a, b), (c, d) in zip(pieces, pieces[1:]):
        assert b == c                                           # no gap, no overlap
    for a, b in pieces:
        assert 0 < b - a <= int((max_total - ref_secs) * sr)    # within budget


def test_plan_vc_chunks_tiles_the_source_within_budget():
    from f5e_tts_amd.infer.utils_infer import plan_vc_chunks
    sr = 16000
    for n, ref, mx in ((9 * sr, 2.0, 6.0), (100 * sr + 17, 4.5, 22.0), (sr * 4 + 1, 2.0, 6.0), (44100 * 31, 7.25, 22.0)):
        pieces = plan_vc_chunks(n, sr, ref, [], mx)
        check_plan(pieces, n, sr, ref, mx)
        ml = int((mx - ref) * sr)
        assert len(pieces) == -(-n // ml) and all(b - a == ml for a, b in pieces[:-1])      # hard cuts without silences


def test_plan_vc_chunks_cuts_inside_a_silence_of_the_search_window():
    from f5e_tts_amd.infer.utils_infer import plan_vc_chunks
    sr, ref, mx = 24000, 2.0, 6.0                     # 4 s windows; search zone = the last third of each
    n = 11 * sr
    sil = [[500, 900], [2900, 3100], [3300, 3900], [5000, 5050], [7200, 9000]]
    pieces = plan_vc_chunks(n, sr, ref, sil, mx)
    check_plan(pieces, n, sr, ref, mx)
    ml = int((mx - ref) * sr)
    start = 0
    for a, b in pieces[:-1]:
        lo, hi = start + ml - ml // 3, start + ml
        hits = [(max(int(s * sr / 1000), lo), min(int(e * sr / 1000), hi)) for s, e in sil]
        hits = [h for h in hits if h[1] > h[0]]
        if hits:
            longest = max(hits, key=lambda h: h[1] - h[0])
            assert b == (longest[0] + longest[1]) // 2
            assert any(int(s * sr / 1000) <= b <= int(e * sr / 1000) for s, e in sil) and lo <= b <= hi
        else:
            assert b == hi
        start = b
    # the first window [0, 4 s): zone [2.667, 4 s) meets 2.9-3.1 and 3.3-3.9 -> the middle of the longer one
    assert pieces[0][1] == int(3.6 * sr)
    # a silence outside every search zone changes nothing
    assert plan_vc_chunks(n, sr, ref, [[100, 300]], mx) == plan_vc_chunks(n, sr, ref, [], mx)


def test_plan_vc_chunks_single_piece_and_exhausted_budget():
    from f5e_tts_amd.infer.utils_infer import plan_vc_chunks
    assert plan_vc_chunks(3 * 44100, 44100, 2.0, [[1000, 2000]], 22.0) == [(0, 3 * 44100)]
    assert plan_vc_chunks(20 * 16000, 16000, 2.0, [], 22.0) == [(0, 20 * 16000)]               # exactly the budget
    with pytest.raises(ValueError, match="prompt"):
        plan_vc_chunks(16000, 16000, 21.5, [], 22.0)
    with pytest.raises(ValueError):
        plan_vc_chunks(16000, 16000, 5.5, [], 6.0)


# ------------------------------------------------------------------ PPG / codebook models through load_model

def test_load_model_builds_the_ppg_codebook_family_on_cpu():
    from f5e_tts_amd.infer import infer_cli
    from f5e_tts_amd.infer import utils_infer as U
    from f5e_tts_amd.model import DiT
    mc = infer_cli.load_model_config("F5TTS_Small_PPG", "")
    assert mc["arch"] == infer_cli.load_arch("F5TTS_Small_PPG", "")
    assert mc["transformer_ppg_config"]["use_ppg"] and mc["transformer_codebook_config"]["use_codebook"]
    assert mc["frontend_ppg_config"]["model_path"].endswith("33.pt")
    model = U.load_model(DiT, mc["arch"], "", device="cpu",
                         ppg_config=(mc["transformer_ppg_config"], mc["cfm_ppg_config"]),
                         cb_config=(mc["transformer_codebook_config"], mc["cfm_codebook_config"]))
    ref = json.load(open(os.path.join(GOLD, "layouts.json")))["small_ppg_codebook"]
    assert {k: list(v.shape) for k, v in model.transformer.state_dict().items()} == ref
    assert model.use_align_loss is False and model.transformer.use_ppg and model.transformer.use_codebook
    # the plain family is untouched: same arch dict, no PPG keys
    base = infer_cli.load_model_config("F5TTS_v1_Base", "")
    assert base["arch"] == infer_cli.load_arch("F5TTS_v1_Base", "") and not base["transformer_ppg_config"]["use_ppg"]


# ------------------------------------------------------------------ infer_cli

def test_cli_new_flags_parse_and_resolve():
    from f5e_tts_amd.infer.infer_cli import build_parser, resolve_settings
    P = build_parser()
    a = P.parse_args(["--mode", "tts", "--alpha_spk", "1.5", "--alpha_txt", "2", "--alpha_ppg", "4", "--ppg_model", "m.pt",
                      "--ppg_config", "t.yaml", "--ppg_stream", "--source_audio", "s.wav"])
    s = resolve_settings(a, {})
    assert (s["mode"], s["alpha_spk"], s["alpha_txt"], s["alpha_ppg"]) == ("tts", 1.5, 2.0, 4.0)
    assert (s["ppg_model"], s["ppg_config"], s["ppg_stream"], s["source_audio"]) == ("m.pt", "t.yaml", True, "s.wav")
    with pytest.raises(SystemExit):
        P.parse_args(["--mode", "edit"])
    # --source_audio without --mode means voice conversion, from the flag or from the toml
    assert resolve_settings(P.parse_args(["--source_audio", "s.wav"]), {})["mode"] == "vc"
    assert resolve_settings(P.parse_args([]), {"source_audio": "s.wav"})["mode"] == "vc"
    assert resolve_settings(P.parse_args(["--source_audio", "s.wav", "--mode", "cfg"]), {})["mode"] == "cfg"
    assert resolve_settings(P.parse_args([]), {"source_audio": "s.wav", "mode": "tts"})["mode"] == "tts"


def test_cli_precedence_for_new_keys_and_unchanged_old_defaults():
    from f5e_tts_amd.infer import utils_infer as U
    from f5e_tts_amd.infer.infer_cli import build_parser, resolve_settings
    P = build_parser()
    s = resolve_settings(P.parse_args([]), {})
    assert (s["mode"], s["source_audio"], s["alpha_spk"], s["alpha_txt"], s["alpha_ppg"]) == ("cfg", "", 2.5, 3.0, 3.0)
    assert (s["ppg_model"], s["ppg_config"], s["ppg_stream"]) == ("", "", False)
    toml = {"alpha_spk": 1.0, "alpha_ppg": 2.0, "ppg_model": "toml.pt", "mode": "tts", "ppg_stream": True}
    s = resolve_settings(P.parse_args(["--alpha_spk", "4", "--mode", "vc"]), toml)
    assert (s["alpha_spk"], s["alpha_ppg"], s["alpha_txt"], s["ppg_model"], s["mode"], s["ppg_stream"]) == \
        (4.0, 2.0, 3.0, "toml.pt", "vc", True)                                 # flag > toml > default
    assert resolve_settings(P.parse_args(["--alpha_spk", "0"]), toml)["alpha_spk"] == 1.0   # the falsy-`or` rule
    # every key that existed before keeps its default
    s = resolve_settings(P.parse_args([]), {})
    old = dict(model="F5TTS_v1_Base", model_cfg="", ckpt_file="", vocab_file="",
               ref_audio="infer/examples/basic/basic_ref_en.wav",
               ref_text="Some call me nature, others call me mother nature.",
               gen_text="Here we generate something just for test.", gen_file="", output_dir="tests", save_chunk=False,
               remove_silence=False, load_vocoder_from_local=False, vocoder_name="vocos", target_rms=0.1,
               cross_fade_duration=0.15, nfe_step=32, cfg_strength=2.0, sway_sampling_coef=-1.0, speed=1.0,
               fix_duration=None, device=U.device)
    for k, v in old.items():
        assert s[k] == v, k
    assert set(s) - set(old) == {"output_file", "mode", "source_audio", "alpha_spk", "alpha_txt", "alpha_ppg", "ppg_model",
                                 "ppg_config", "ppg_stream"}


@pytest.mark.parametrize("mode", ["tts", "vc"])
def test_cli_refuses_a_model_without_ppg(mode, capsys):
    from f5e_tts_amd.infer import infer_cli
    with pytest.raises(SystemExit) as e:
        infer_cli.main(["--mode", mode, "--source_audio", "s.wav", "-m", "F5TTS_v1_Base"])
    assert "use_ppg" in str(e.value)
    with pytest.raises(SystemExit) as e:
        infer_cli.main(["--mode", "vc", "-m", "F5TTS_Small_PPG"])
    assert "--source_audio" in str(e.value)
