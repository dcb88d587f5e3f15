"""eval/eval_wer.py: the edit-distance counts against a brute-force search, the text clean-up, the per-utterance driver with
a stub recogniser, and the command line.  Host code only."""
import json
import random
from functools import lru_cache

import pytest

from f5e_tts_amd.eval import eval_wer as W


def brute_distance(ref, hyp):
    """Minimum number of unit edits by the defining recursion (no table shared with the code under test)."""
    ref, hyp = tuple(ref), tuple(hyp)

    @lru_cache(maxsize=None)
    def go(i, j):
        if i == len(ref):
            return len(hyp) - j
        if j == len(hyp):
            return len(ref) - i
        if ref[i] == hyp[j]:
            return go(i + 1, j + 1)
        return 1 + min(go(i + 1, j + 1), go(i + 1, j), go(i, j + 1))
    return go(0, 0)


def test_word_errors_hand_cases():
    assert W.word_errors([], []) == (0, 0, 0, 0)
    assert W.word_errors(["a", "b", "c"], []) == (0, 0, 3, 0)                      # empty hypothesis: all deleted
    assert W.word_errors([], ["a", "b"]) == (0, 0, 0, 2)                           # empty reference: all inserted
    assert W.word_errors(["a", "b"], ["a", "x", "b"]) == (2, 0, 0, 1)              # pure insertion
    assert W.word_errors(["a", "b", "c"], ["a", "c"]) == (2, 0, 1, 0)
    assert W.word_errors(["a", "b", "c"], ["a", "x", "c"]) == (2, 1, 0, 0)
    assert W.word_errors("kitten", "sitting") == (4, 2, 0, 1)
    # the documented tie-break: diagonal before deletion before insertion (both alignments cost 2)
    assert W.word_errors(["a", "b"], ["b", "c"]) == (0, 2, 0, 0)
    assert W.wer("the cat sat", "the cat sat") == 0.0 and W.wer("the cat sat", "the dog") == pytest.approx(2 / 3)
    assert W.wer("a", "a b c") == 2.0                                              # insertions push WER past 1
    with pytest.raises(ValueError):
        W.wer("", "a")


def test_word_errors_against_brute_force_on_seeded_sequences():
    rng = random.Random(20250)
    for _ in range(300):
        ref = [rng.randrange(4) for _ in range(rng.randrange(0, 9))]
        hyp = [rng.randrange(4) for _ in range(rng.randrange(0, 9))]
        h, s, d, i = W.word_errors(ref, hyp)
        assert min(h, s, d, i) >= 0 and h + s + d == len(ref) and h + s + i == len(hyp)
        assert s + d + i == brute_distance(ref, hyp)


def test_normalize_en_and_zh():
    assert W.normalize("Hello, World!  It's  fine.", "en") == "hello world its fine"
    assert W.normalize("“Quoted” — dash…", "en") == "quoted dash"                   # Unicode category P*
    assert W.normalize("a   b", "en") == "a  b" and W.wer(W.normalize("a   b", "en"), "a b") == 0.0   # ONE pass, as there
    assert W.normalize("你好，世界！", "zh") == "你 好 世 界"
    assert W.normalize("今天 天气。", "zh").split() == ["今", "天", "天", "气"]
    assert W.is_punctuation("。") and W.is_punctuation("'") and W.is_punctuation("$") and not W.is_punctuation("a")
    with pytest.raises(NotImplementedError):
        W.normalize("x", "fr")


class StubAligner:
    def __init__(self, answers):
        self.answers, self.calls = answers, []

    def transcribe(self, audio, sr=None, mode="ctc_greedy_search", **kw):
        self.calls.append((audio, sr, mode, kw))
        return self.answers[audio]


def test_run_asr_wer_with_a_stub_aligner():
    items = [("/x/utt1.wav", "/p/a.wav", "The cat sat."), ("/x/utt2.wav", "/p/b.wav", "Good morning, all")]
    stub = StubAligner({"/x/utt1.wav": "the cat sat", "/x/utt2.wav": "good evening"})
    res = W.run_asr_wer(items, stub, "en", "ctc_prefix_beam_search", beam_size=4)
    assert [r["wav"] for r in res] == ["utt1", "utt2"] and set(res[0]) == {"wav", "truth", "hypo", "wer"}
    assert res[0]["truth"] == "The cat sat." and res[0]["hypo"] == "the cat sat" and res[0]["wer"] == 0.0     # raw texts kept
    assert res[1]["wer"] == pytest.approx(2 / 3)
    assert stub.calls[0] == ("/x/utt1.wav", None, "ctc_prefix_beam_search", {"beam_size": 4})
    zh = W.run_asr_wer([("/x/z.wav", "", "你好，世界")], StubAligner({"/x/z.wav": "你好世间"}), "zh")
    assert zh[0]["wer"] == pytest.approx(1 / 4)
    with pytest.raises(NotImplementedError):
        W.run_asr_wer(items, stub, "fr")


def test_command_line_reads_the_list_and_prints_the_mean(tmp_path, capsys):
    gen = tmp_path / "gen"
    gen.mkdir()
    for utt in ("u1", "u2"):
        (gen / f"{utt}.wav").write_bytes(b"")
    lst = tmp_path / "meta.lst"
    lst.write_text("u1|prompt one|prompts/p1.wav|Hello there.\nu2|prompt two|prompts/p2.wav|General Kenobi|wavs/u2.wav\n"
                   "u3|no wav|prompts/p3.wav|skipped\n")
    stub = StubAligner({str(gen / "u1.wav"): "hello there", str(gen / "u2.wav"): "general"})
    mean = W.main(["--metalst", str(lst), "--gen_wav_dir", str(gen), "--lang", "en", "--mode", "ctc_greedy_search"],
                  aligner=stub)
    assert mean == pytest.approx(0.25)
    out = capsys.readouterr().out
    assert "u1\t0.0000\thello there" in out and "WER: 0.25000 over 2 utterances" in out
    saved = json.loads((gen / "_wer_results.json").read_text())
    assert [r["wav"] for r in saved] == ["u1", "u2"] and saved[1]["wer"] == 0.5
