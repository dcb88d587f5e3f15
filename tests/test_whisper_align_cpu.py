"""Whisper word timestamps, the parts that need no GPU: the restatement (tests/whisper_align_ref.py) against the fixture made from
``transformers`` (tests/golden/whisper_align.npz, tests/golden/make_whisper_align_golden.py) in float32 and float64, the word
grouping against the reference's word lists, the configuration, the wiring and the C ABI entries.

The frame indices must come out EXACTLY in both precisions: the fixture's generator asserted that on every cell of every DTW path
the chosen predecessor and the runner-up differ by at least 1e-3 (``gap_<case>``), and the float32 / float64 cost matrices differ
from the stored one by a few 1e-7 (printed)."""
import json
import os
import re

import numpy as np
import pytest

import whisper_align_ref as A
import whisper_ref as R
from test_whisper_cpu import gold, tiny_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (("f5e_cross_attn_probs_f32", 18), ("f5e_dtw_cost_f32", 12), ("f5e_dtw_workspace_bytes", 4), ("f5e_dtw_path", 11))
N0 = 4

_fx = {}


def align_gold():
    """The fixture, loaded once and shared (read-only)."""
    if not _fx:
        _fx.update(A.load_fixture())
    return _fx


def heads():
    return [tuple(h) for h in align_gold()["alignment_heads"].tolist()]


def align_cfg():
    from f5e_tts_amd.eval.whisper import WhisperConfig
    fx = gold()
    gen = dict(fx["generation_config"], alignment_heads=[list(h) for h in heads()])
    return WhisperConfig.from_dicts(fx["config"], gen)


def align_model(which="a"):
    """The tiny model with alignment heads: 'a' = the greedy fixture's weights, 'b' = the second seed's, 'beos' = those with the
    scaled eos row."""
    import torch
    from f5e_tts_amd.eval.whisper import Whisper
    fx, ax = gold(), align_gold()
    sd = {k: torch.from_numpy(v.copy()) for k, v in (fx["sd"] if which == "a" else ax["sd_b"]).items()}
    if which == "beos":
        sd["model.decoder.embed_tokens.weight"][fx["config"]["eos_token_id"]] = torch.from_numpy(ax["eos_row_b_f32"].copy())
    model = Whisper(align_cfg())
    model.load_state_dict(sd)
    model.set_vocab(json.loads(str(fx["vocab_json"])), json.loads(str(fx["added_tokens_json"])))
    return model


# ---- the restatement against the fixture ----

def test_the_fixture_has_the_cases_the_rules_need():
    ax = align_gold()
    names = ax["names"]
    assert len(names) >= 3 and int(ax["seed_a"]) != int(ax["seed_b"])
    shapes = {c: ax[f"probs_{c}"].shape for c in names}
    assert {s[2] for s in shapes.values()} == {45, 150}                               # 0.9 s and 3 s
    assert any(s[1] == 1 for s in shapes.values())                                    # N = 1
    assert any(ax[f"tokens_{c}"][-1] == 140 and len(ax[f"tokens_{c}"]) < 48 for c in names)   # ends on eos before the cap
    for c in names:
        n, (S, N, M) = len(ax[f"tokens_{c}"]), shapes[c]
        assert S == len(heads()) and N == n - N0 - 1 and M == int(ax[f"nframes_{c}"]) // 2
        assert N < 2 or float(ax[f"gap_{c}"]) >= 1e-3
        assert (ax[f"frames_{c}"][:N0] == 0).all() and ax[f"frames_{c}"][-1] == ax[f"frames_{c}"][-2]
    assert max(int(ax[f"frames_{c}"].max()) for c in names) > 100                     # the paths are not trivial


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_restatement_reproduces_the_frame_indices(dtype):
    ax = align_gold()
    for c in ax["names"]:
        want = ax[f"frames_{c}"]
        got = A.token_frames(ax[f"probs_{c}"], len(want), N0, int(ax["median_filter_width"]), dtype)
        if ax[f"probs_{c}"].shape[1] >= 2:
            C = A.cost_matrix(ax[f"probs_{c}"], int(ax["median_filter_width"]), dtype)
            print(f"{c} {dtype.__name__}: cost against the stored one, max abs {np.abs(C - ax[f'cost_{c}']).max():.2e}, smallest "
                  f"on-path gap {float(ax[f'gap_{c}']):.2e}")
            assert np.abs(C - ax[f"cost_{c}"]).max() < 1e-2 * float(ax[f"gap_{c}"])
            assert np.array_equal(A.dtw_first(ax[f"cost_{c}"]), want[N0:-1])           # rules 5-6 alone, on the stored matrix
        assert np.array_equal(got, want), c


def test_restatement_rule_1_from_the_model():
    """The stored probabilities are the float64 model's, softmax over all 150 keys and cut to M."""
    fx, ax = gold(), align_gold()
    ref = R.Ref(fx["sd"], fx["config"])
    enc = ref.encoder(R.log_mel(fx["wave_f32"], 48000, 300, R.slaney_filters(128)))
    want = ax["probs_a3s"]
    got = A.alignment_probs(ref, enc, ax["tokens_a3s"], heads(), N0, want.shape[1], want.shape[2])
    e = R.rel_l2(got, want)
    print(f"a3s: probabilities of the float64 model against the fixture, rel L2 {e:.2e}")
    assert e < 1e-5
    assert (want.sum(-1) < 1.0 + 1e-6).all()


def test_diagonal_evaluation_equals_the_cell_by_cell_one():
    g = np.random.default_rng(5)
    for N, M in ((1, 1), (1, 7), (5, 1), (3, 4), (7, 3), (20, 33)):
        for C in (g.integers(-2, 3, (N, M)).astype(np.float32), g.standard_normal((N, M)).astype(np.float32),
                  g.standard_normal((N, M))):
            assert np.array_equal(A.dtw_first(C), A.dtw_first_loop(C)), (N, M, C.dtype)
    # every tie goes left: on a constant matrix the path runs along the last row and climbs the first column
    assert A.dtw_first_loop(np.zeros((3, 5), np.float32)).tolist() == [0, 0, 0]
    assert A.dtw_first_loop(np.array([[0, 9, 9], [9, 0, 9], [9, 9, 0]], np.float32)).tolist() == [0, 1, 2]


def test_include_last_and_edge_cases_of_the_layout():
    ax = align_gold()
    p = ax["probs_b09"]
    n = len(ax["tokens_b09"])
    assert A.token_frames(p[:, :0], N0 + 1, N0).tolist() == [0] * (N0 + 1)              # N = 0
    assert A.token_frames(p[:, :1], N0 + 2, N0).tolist() == [0] * (N0 + 2)              # N = 1
    last = A.token_frames(p, n - 1, N0, include_last=True)                              # the same rows, one token fewer
    assert np.array_equal(last, ax["frames_b09"][:n - 1])


# ---- words ----

def test_word_lists_equal_the_reference():
    from f5e_tts_amd.eval.whisper import group_tokens
    ax, model = align_gold(), tiny_model()
    assert {w["language"] for w in ax["words"]} == {"english", "chinese"}               # both split modes
    for row, want in zip(ax["word_ids"], ax["words"]):
        ids = [int(i) for i in row if i >= 0]
        words, index = group_tokens(model.id_to_piece, model.first_special, ids, want["language"], model.cfg.eos_token_id)
        assert words == want["words"] and index == want["indices"], (ids, words, want)
    assert group_tokens(model.id_to_piece, model.first_special, [0, 1], "zh")[0] == [" hello", " world"]


def test_words_from_tokens_times():
    model = tiny_model()
    # <|sot|> <|en|> <|transcribe|> <|notimestamps|> " hello" "," " the" " world" "ing" "." <|endoftext|>
    comma, dot = (k for k, p in sorted(model.id_to_piece.items()) if p in (",", "."))
    ids = [141, 142, 146, 159, 0, comma, 2, 1, 3, dot, 140]
    times = [0, 0, 0, 0, 0.1, 0.3, 0.5, 0.9, 1.1, 1.2, 1.6]
    assert model.words_from_tokens(ids, times, "en") == [(" hello,", 0.1, 0.5), (" the", 0.5, 0.9), (" worlding.", 0.9, 1.6)]
    assert model.words_from_tokens(ids[:-1], times[:-1], "en")[-1] == (" worlding.", 0.9, 1.2)     # nothing follows: its last token
    assert model.words_from_tokens([141, 140], [0, 0], "en") == []
    from f5e_tts_amd import _C
    with pytest.raises(_C.F5EError, match="times"):
        model.words_from_tokens(ids, times[:-1], "en")


# ---- configuration ----

def test_config_reads_and_checks_alignment_heads():
    from f5e_tts_amd import _C
    from f5e_tts_amd.eval.whisper import Whisper, WhisperConfig
    fx = gold()
    cfg = align_cfg()
    assert cfg.alignment_heads == tuple(heads()) and cfg.median_filter_width == 7
    plain = WhisperConfig.from_dicts(fx["config"], fx["generation_config"])
    assert plain.alignment_heads == ()                                                  # nothing changes for a model without them
    Whisper(plain)
    assert WhisperConfig.from_dicts(dict(fx["config"], median_filter_width=5), fx["generation_config"]).median_filter_width == 5
    for bad in ([[2, 0]], [[0, 4]], [[-1, 0]], [[0, 0]] * 65):
        with pytest.raises(_C.F5EError, match="alignment_heads"):
            Whisper(WhisperConfig.from_dicts(fx["config"], dict(fx["generation_config"], alignment_heads=bad)))
    with pytest.raises(_C.F5EError, match="alignment_heads"):
        WhisperConfig.from_dicts(fx["config"], dict(fx["generation_config"], alignment_heads=[[0, 1, 2]]))
    for width in (4, 0, 17):
        with pytest.raises(_C.F5EError, match="median_filter_width"):
            Whisper(WhisperConfig.from_dicts(dict(fx["config"], median_filter_width=width), fx["generation_config"]))


def test_times_without_alignment_heads_are_refused():
    import torch
    from f5e_tts_amd import _C
    model = tiny_model()
    with pytest.raises(_C.F5EError, match="alignment_heads"):
        model.token_timestamps([], torch.zeros(1, 6, dtype=torch.int32), [6], 90, 4)
    with pytest.raises(_C.F5EError, match="alignment_heads"):
        model.generate_from_kv([], [141, 142, 146, 159], return_token_timestamps=True)


# ---- wiring ----

class StubWords:
    """A WhisperRecognizer whose transcript is given: ``align`` is the real one."""

    def __init__(self, spans):
        self.spans = spans

    def transcribe_words(self, audio, sr=None):
        return list(self.spans)


def test_align_feeds_diff_parts():
    from f5e_tts_amd.eval.whisper import WhisperRecognizer
    from f5e_tts_amd.infer.speech_edit import diff_parts
    from f5e_tts_amd.ppg.ctc_align import WordSpan, split_words
    spans = [WordSpan("Some", 0.1, 0.4), WordSpan("call", 0.4, 0.8), WordSpan("me", 0.8, 1.0), WordSpan("nature", 1.0, 1.7)]
    stub = StubWords(spans)
    got = WhisperRecognizer.align(stub, None, 16000, "some call me Nature.")
    assert got == [WordSpan("some", 0.1, 0.4), WordSpan("call", 0.4, 0.8), WordSpan("me", 0.8, 1.0), WordSpan("Nature.", 1.0, 1.7)]
    parts, fix = diff_parts(got, split_words("some call you Nature."))
    assert parts == [[0.8, 1.0]] and fix is None
    with pytest.raises(ValueError, match="'you' vs 'me'"):
        WhisperRecognizer.align(stub, None, 16000, "some call you nature")
    with pytest.raises(ValueError, match="word 4"):
        WhisperRecognizer.align(stub, None, 16000, "some call me nature now")
    cjk = StubWords([WordSpan("你好", 0.0, 1.0), WordSpan("world", 1.0, 1.5)])
    assert WhisperRecognizer.align(cjk, None, 16000, "你好 world") == [WordSpan("你", 0.0, 0.5), WordSpan("好", 0.5, 1.0),
                                                                    WordSpan("world", 1.0, 1.5)]


def test_speech_edit_has_the_whisper_flags(capsys):
    from f5e_tts_amd.infer import speech_edit
    base = ["--audio", "a.wav", "--origin_text", "a", "--target_text", "b", "-p", "ckpt.pt"]
    args = speech_edit.build_parser().parse_args(base + ["--whisper_dir", "W", "--whisper_language", "de", "--whisper_beam", "5"])
    assert (args.whisper_dir, args.whisper_language, args.whisper_beam) == ("W", "de", 5)
    none = speech_edit.build_parser().parse_args(base)
    assert (none.whisper_dir, none.whisper_language, none.whisper_beam) == (None, "en", 1)       # opt-in
    with pytest.raises(SystemExit, match="one aligner"):
        speech_edit.main(base + ["--whisper_dir", "W", "--asr_model", "m", "--asr_config", "c", "--asr_dict", "d"])
    with pytest.raises(SystemExit, match="--whisper_dir"):
        speech_edit.main(base)


# ---- C ABI ----

def test_abi_declares_and_binds_the_entries():
    from f5e_tts_amd import _C, ops
    header = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    for name, nargs in ENTRIES:
        m = re.search(r"F5E_API int %s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_C.SIGNATURES[name]), name
    assert "#define F5E_ABI_VERSION 2 " in header and _C.ABI_VERSION == 2               # functions were only added
    assert "whisper_align.hip" in open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "Makefile")).read()
    for fn in ("cross_attn_probs_f32", "dtw_cost_f32", "dtw_workspace_bytes", "dtw_path"):
        assert callable(getattr(ops, fn))
    lib = _C.LIB_PATH
    if os.path.exists(lib):                                                             # exported by the built library
        import ctypes
        handle = ctypes.CDLL(lib)
        for name, _ in ENTRIES:
            assert hasattr(handle, name), name
