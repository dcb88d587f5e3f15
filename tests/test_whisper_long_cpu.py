"""Whisper's timestamp decoding and long-form loop, the parts that need no GPU: the float64 restatement (tests/whisper_long_ref.py)
against the fixture made from ``transformers`` (tests/golden/whisper_long.npz, tests/golden/make_whisper_long_golden.py), the
package's host functions (``split_segments``, ``compression_ratio``, the configuration) against the same records, the refusals,
the C ABI entries and the opt-in wiring.

Restatement gates: masks, tokens, seeks and segment boundaries exact (the generator asserts a margin of 1e-2 of the logits' RMS
for every pick and every timestamp / text comparison), times within 1e-9, ``avg_logprob`` and ``no_speech_prob`` within 1e-5 (the
fixture's are fp32 arithmetic)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import whisper_long_ref as LR
import whisper_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (("f5e_whisper_ts_pick", 20), ("f5e_whisper_ts_rule", 17), ("f5e_whisper_beam_step_ts", 33))
WINDOW, CAP = 100, 40

_gold = {}


def gold():
    """The fixture, loaded once and shared (read-only)."""
    if not _gold:
        _gold.update(LR.load_fixture())
    return _gold


def case(name):
    return [c for c in gold()["cases"] if c["name"] == name][0]


def case_wave(c, b=0):
    lo, hi = c["waves"][b]
    return gold()["wave_f32"][lo:hi]


def tiny_cfg(**over):
    from f5e_tts_amd.eval.whisper import WhisperConfig
    gen = dict(gold()["generation_config"])
    gen.update(over)
    return WhisperConfig.from_dicts(gold()["config"], gen)


def tiny_model(name):
    from f5e_tts_amd.eval.whisper import Whisper
    model = Whisper(tiny_cfg())
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in LR.case_sd(gold(), case(name)).items()})
    return model


def ref_run(name, b=0):
    """The restatement's run of row b of a case, computed once and shared."""
    key = ("run", name, b)
    if key not in _gold:
        fx, c = gold(), case(name)
        ref = R.Ref(LR.case_sd(fx, c), fx["config"])
        w = case_wave(c, b)
        feats = R.log_mel(w, len(w), max(len(w) // 160, WINDOW), R.slaney_filters(80))    # shorter than a window: the wave is padded
        _gold[key] = LR.transcribe_long_ref(ref, feats, fx["prompt"].tolist(), fx["generation_config"], CAP, WINDOW,
                                            c.get("num_beams", 1), c.get("no_speech_threshold"), c.get("logprob_threshold"))
    return _gold[key]


def windows_of(c, b):
    """The fixture's (avg_logprob, no_speech_prob) of row b's windows: the records are in decoding order, iteration by iteration
    over the rows that were not finished."""
    out, k = [], 0
    for seeks in c["seeks"]:
        for r in range(len(c["frames"])):
            if seeks[r] < c["frames"][r]:
                if r == b:
                    out.append(c["windows"][k])
                k += 1
    return out


# ---- the restatement against the fixture ----

def test_fixture_shows_every_case():
    kinds = {c["name"]: c["kinds"] for c in gold()["cases"]}
    assert "p" in kinds["a"][0] and "s" in kinds["b"][0] and "N" in kinds["c"][0]
    d = case("d")
    assert d["frames"][0] - d["seeks"][-1][0] < WINDOW                       # a last partial window
    assert "k" in kinds["e"][0] and len(case("e")["segments"][0]) > 0        # one window skipped, others kept
    f = case("f")
    assert len(f["frames"]) == 2 and any(s[1] >= f["frames"][1] and s[0] < f["frames"][0] for s in f["seeks"])
    assert case("g")["waves"][0][1] - case("g")["waves"][0][0] < 160 * WINDOW and case("g")["frames"] == [WINDOW]
    assert case("h")["num_beams"] == 3 and len(set(case("i")["languages"])) >= 2
    assert all(min(case(n)["margins"]) >= 1e-2 for n in "abc") and case("i")["language_margin"] >= 1e-2
    e = case("e")
    assert all(abs(n - e["no_speech_threshold"]) >= 1e-2 and abs(a - e["logprob_threshold"]) >= 1e-2 for a, n in e["windows"])


def test_rule_masks_equal_the_processor():
    fx = gold()
    g = fx["generation_config"]
    for hist, x, want in zip(fx["mask_hist"], fx["mask_logits"], fx["mask_banned"]):
        h = [int(t) for t in hist if t >= 0]
        ban, _ = LR.ts_mask(h, x, g["eos_token_id"], g["no_timestamps_token_id"], g["max_initial_timestamp_index"])
        assert (ban == want).all(), (h, np.nonzero(ban != want)[0])
    assert len({tuple(h) for h in fx["mask_hist"].tolist()}) >= 6 and np.isinf(fx["mask_logits"]).any()


@pytest.mark.parametrize("name,b", [("a", 0), ("b", 0), ("c", 0), ("e", 0), ("f", 1), ("g", 0), ("h", 0)])
def test_restatement_reproduces_the_fixture(name, b):
    c = case(name)
    segs, seeks, gaps, kinds = ref_run(name, b)
    want = c["segments"][b]
    assert [s["tokens"] for s in segs] == [s["tokens"] for s in want]
    assert seeks == [s[b] for s in c["seeks"] if s[b] < c["frames"][b]] and kinds == c["kinds"][b]
    err_t = max([abs(s["start"] - q["start"]) for s, q in zip(segs, want)] + [abs(s["end"] - q["end"]) for s, q in zip(segs, want)])
    assert err_t < 1e-9
    if c.get("num_beams", 1) == 1:
        rec = [w for w, k in zip(windows_of(c, b), kinds) if k != "k"]        # skipped windows leave no segment to compare
        got = []
        for s in segs:
            if not got or got[-1][2] != s["seek"]:
                got.append((s["avg_logprob"], s["no_speech_prob"], s["seek"]))
        err = max(max(abs(a - w[0]), abs(n - w[1])) for (a, n, _), w in zip(got, rec))
        print(f"case {name}[{b}]: {kinds}, time error {err_t:.1e}, avg_logprob / no_speech_prob error {err:.2e}, margins {gaps}")
        assert len(got) == len(rec) and err < 1e-5 and min(gaps) >= 1e-2


def test_detect_language_restatement():
    fx, c = gold(), case("i")
    ref = R.Ref(LR.case_sd(fx, c), fx["config"])
    fb = R.slaney_filters(80)
    got = [LR.detect_language_ref(ref, ref.encoder(R.log_mel(case_wave(c, b), 16000, WINDOW, fb)), fx["generation_config"])
           for b in range(3)]
    assert got == c["languages"]


# ---- the package's host functions against the same records (these fail on the parent commit) ----

def test_split_segments_equals_the_fixture_and_the_restatement():
    from f5e_tts_amd.eval.whisper import split_segments
    tb = gold()["generation_config"]["no_timestamps_token_id"] + 1
    n = 0
    for name in "abcefg":
        c = case(name)
        for b in range(len(c["frames"])):
            seeks = [s[b] for s in c["seeks"] if s[b] < c["frames"][b]] + [c["frames"][b]]
            for lo, hi in zip(seeks[:-1], seeks[1:]):
                want = [s for s in c["segments"][b] if lo * 0.01 - 1e-9 <= s["start"] < hi * 0.01 - 1e-9]
                if not want:
                    continue                                                  # a skipped window
                kept = [t for s in want for t in s["tokens"]]
                nf = min(WINDOW, c["frames"][b] - lo)
                # what the window decoded: the kept tokens, plus anything after a cut that the fixture does not keep
                last = hi == c["frames"][b]                               # a pair near the end may point beyond the recording
                for tail in ([], [7, 12]) if hi - lo < nf else ([],):
                    parts, step = split_segments(kept + tail, tb, lo, nf)
                    assert (lo + step >= hi if last else step == hi - lo) and [p[2] for p in parts] == [s["tokens"] for s in want]
                    assert all(abs(p[0] - s["start"]) < 1e-9 and abs(p[1] - s["end"]) < 1e-9 for p, s in zip(parts, want))
                    assert (parts, step) == LR.split_ref(kept + tail, tb, lo, nf)
                    n += 1
    assert n >= 12


def test_split_segments_branches_by_hand():
    from f5e_tts_amd.eval.whisper import split_segments
    tb = 111
    assert split_segments([tb, 5, 6, tb + 10, tb + 10, 7, tb + 30], tb, 200, 100) == \
        ([(2.0, 2.2, [tb, 5, 6, tb + 10]), (2.2, 2.6, [tb + 10, 7, tb + 30])], 100)           # single-timestamp ending
    assert split_segments([tb + 2, 5, tb + 10, tb + 10, 7, 8], tb, 0, 100) == ([(0.04, 0.2, [tb + 2, 5, tb + 10, tb + 10])], 20)
    assert split_segments([tb, 5, 6], tb, 100, 62) == ([(1.0, 1.0 + 31 * 0.02, [tb, 5, 6])], 62)   # no pair, only <|0.00|>
    assert split_segments([tb + 3, 5, tb + 9], tb, 100, 62) == ([(1.0, 1.0 + 9.0 * 0.02, [tb + 3, 5, tb + 9])], 62)
    assert split_segments([tb + 3], tb, 0, 100) == ([(0.0, 0.06, [tb + 3])], 100)


def test_compression_ratio_is_the_reference_formula():
    import zlib
    from f5e_tts_amd.eval.whisper import compression_ratio
    toks = [5, 6, 5, 6, 5, 6, 5, 6, 200, 5, 6]
    raw = b"".join(t.to_bytes(1, "little") for t in toks)
    assert compression_ratio(toks, 162) == len(raw) / len(zlib.compress(raw))
    raw = b"".join(t.to_bytes(2, "little") for t in toks)
    assert compression_ratio(toks, 51866) == len(raw) / len(zlib.compress(raw))


def test_config_reads_the_new_fields_and_derives_no_speech():
    from f5e_tts_amd import _C
    from f5e_tts_amd.eval.whisper import WhisperConfig
    cfg = tiny_cfg()
    assert (cfg.max_initial_timestamp_index, cfg.prev_sot_token_id, cfg.timestamp_begin, cfg.no_speech_token_id) == (25, 108, 111, 109)
    assert WhisperConfig().max_initial_timestamp_index is None and WhisperConfig().prev_sot_token_id is None
    bare = WhisperConfig.from_dicts(gold()["config"], {k: v for k, v in gold()["generation_config"].items()
                                                       if k != "no_timestamps_token_id"})
    with pytest.raises(_C.F5EError, match="no_timestamps_token_id"):
        bare.timestamp_begin
    with pytest.raises(_C.F5EError, match="no timestamp classes"):
        tiny_cfg(no_timestamps_token_id=161).timestamp_begin


# ---- refusals, before any launch ----

def test_refusals_by_name():
    from f5e_tts_amd import _C
    from f5e_tts_amd.eval.whisper import Whisper, WhisperConfig
    model = Whisper(tiny_cfg())
    wav = torch.zeros(1, 16000)
    for kw in (dict(temperature=(0.0, 0.2)), dict(temperature=0.4), dict(condition_on_prev_tokens=True), dict(prompt_ids=[1, 2]),
               dict(chunk_length_s=30), dict(return_token_timestamps=True), dict(graph=True)):
        with pytest.raises(_C.F5EError, match=f"{list(kw)[0]} = .* is out of scope"):
            model.transcribe_long(wav, **kw)
    with pytest.raises(TypeError, match="unknown argument 'beams'"):
        model.transcribe_long(wav, beams=3)
    with pytest.raises(_C.F5EError, match="no_speech_threshold and logprob_threshold together"):
        model.transcribe_long(wav, no_speech_threshold=0.6)
    with pytest.raises(_C.F5EError, match="there is no CPU path"):
        model.transcribe_long(wav, temperature=0.0, condition_on_prev_tokens=False)
    with pytest.raises(_C.F5EError, match="language is required"):
        model.prompt_ids("")                                                 # only None means detect
    assert model.prompt_ids("en", timestamps=True) == [101, 102, 106] and model.prompt_ids("en")[-1] == 110
    bare = Whisper(WhisperConfig.from_dicts(gold()["config"], {k: v for k, v in gold()["generation_config"].items()
                                                               if k not in ("no_timestamps_token_id", "lang_to_id")}))
    with pytest.raises(_C.F5EError, match="no_timestamps_token_id"):
        bare.transcribe_long(wav, language="en")
    with pytest.raises(_C.F5EError, match="no_timestamps_token_id"):
        bare.generate(wav, language="en", return_timestamps=True)
    with pytest.raises(_C.F5EError, match="lang_to_id"):
        bare._prompts([(torch.zeros(1, 50, 64), torch.zeros(1, 50, 64))], None, "transcribe", False)


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from f5e_tts_amd import _C, ops
    i32 = torch.int32
    z = lambda *s: torch.zeros(*s, dtype=i32)   # noqa: E731
    with pytest.raises(_C.F5EError, match="there is no CPU path"):
        ops.whisper_ts_pick(torch.zeros(2, 162), z(2, 8), z(2), z(2), z(1), torch.zeros(2), 2, 3, 100, 110)
    with pytest.raises(_C.F5EError, match="there is no CPU path"):
        ops.whisper_ts_rule(torch.zeros(2, 162), z(2, 8), 2, 3, 100, 110)
    with pytest.raises(_C.F5EError, match="logits \\[R, >= V\\] and tokens"):
        ops.whisper_ts_rule(torch.zeros(2, 162), z(3, 8), 2, 3, 100, 110)
    with pytest.raises(_C.F5EError, match="V = 200 exceeds"):
        ops.whisper_ts_pick(torch.zeros(2, 162), z(2, 8), z(2), z(2), z(1), torch.zeros(2), 2, 3, 100, 110, V=200)


# ---- C ABI ----

def test_abi_declares_and_binds_the_three_entries():
    from f5e_tts_amd import _C, ops
    header = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    for name, nargs in ENTRIES:
        m = re.search(r"F5E_API int %s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_C.SIGNATURES[name]), name
        assert hasattr(_C.lib(), name)
    assert "#define F5E_ABI_VERSION 2 " in header and _C.ABI_VERSION == 2       # functions were only added
    assert callable(ops.whisper_ts_pick) and callable(ops.whisper_ts_rule) and callable(ops.whisper_beam_step_ts)
    # the entries that were there keep their signatures
    assert len(_C.SIGNATURES["f5e_greedy_pick"]) == 17 and len(_C.SIGNATURES["f5e_whisper_beam_step"]) == 30
    assert "_ts" in inspect.signature(ops.whisper_beam_step).parameters


def test_c_entries_refuse_bad_arguments_without_a_device():
    """Every check of the three entries comes before the first launch: null operands and bad limits return an error code."""
    import ctypes as C
    from f5e_tts_amd import _C
    lib = _C.lib()
    buf = (C.c_int * 64)()
    fbuf = (C.c_float * 64)()
    p, f = C.cast(buf, C.c_void_p), C.cast(fbuf, C.c_void_p)

    def pick(**o):
        a = dict(logits=f, ld=8, tokens=p, ld_tok=8, last=p, done=p, alive=p, sum_logp=f, R=1, V=8, p=2, n0=3, eos=2, no_ts=4, mi=-1)
        a.update(o)
        return lib.f5e_whisper_ts_pick(None, a["logits"], a["ld"], None, 0, None, 0, a["tokens"], a["ld_tok"], a["last"], a["done"],
                                       a["alive"], a["sum_logp"], a["R"], a["V"], a["p"], a["n0"], a["eos"], a["no_ts"], a["mi"])
    for bad in (dict(logits=None), dict(sum_logp=None), dict(V=1), dict(ld=7), dict(p=1), dict(ld_tok=3), dict(eos=8), dict(no_ts=7),
                dict(no_ts=1), dict(mi=-2), dict(n0=0), dict(R=0)):
        assert pick(**bad) != 0, bad
    assert lib.f5e_whisper_ts_rule(None, f, 8, None, 0, None, 0, p, 8, None, 1, 8, 2, 3, 2, 4, -1) != 0
    assert lib.f5e_whisper_ts_rule(None, f, 8, None, 2, None, 0, p, 8, p, 1, 8, 2, 3, 2, 4, -1) != 0     # a list without its pointer


# ---- wiring ----

def test_wiring_is_opt_in():
    from f5e_tts_amd.eval import eval_wer
    from f5e_tts_amd.eval.whisper import Whisper, WhisperRecognizer
    from f5e_tts_amd.infer import infer_cli
    base = ["--metalst", "m", "--gen_wav_dir", "g", "--lang", "en"]
    assert eval_wer.build_parser().parse_args(base).whisper_long is False
    args = eval_wer.build_parser().parse_args(base + ["--asr", "whisper", "--whisper_long", "--whisper_beam", "5"])
    assert args.whisper_long is True and args.whisper_beam == 5
    assert infer_cli.build_parser().parse_args([]).ref_language == "english"
    assert infer_cli.build_parser().parse_args(["--ref_language", "auto"]).ref_language == "auto"
    ps = inspect.signature(WhisperRecognizer.__init__).parameters
    assert ps["long_form"].default is False and ps["language"].default == "en"
    assert inspect.signature(Whisper.generate).parameters["return_timestamps"].default is False
    ps = inspect.signature(Whisper.transcribe_long).parameters
    assert [ps[k].default for k in ("language", "task", "beam_size", "no_speech_threshold", "logprob_threshold", "sync_every")] == \
        [None, "transcribe", 1, None, None, 8]


class _StubModel:
    n_frames = 100

    def __init__(self):
        self.calls = []

    def generate(self, audio, lens, language, **kw):
        self.calls.append(("generate", tuple(audio.shape), language, kw))
        return torch.tensor([[1, 2, 3]]), torch.tensor([3])

    def transcribe_long(self, audio, lens, language, **kw):
        from f5e_tts_amd.eval.whisper import Segment
        self.calls.append(("long", tuple(audio.shape), language, kw))
        return [[Segment(0.0, 0.5, [111, 1, 136], 0, -1.0, 0.1, 1.0), Segment(1.0, 1.5, [111, 2, 136], 100, -1.0, 0.1, 1.0)]]

    def decode_ids(self, ids):
        return f" w{ids[1]}"


def _stub_recognizer(monkeypatch, **attrs):
    from f5e_tts_amd.eval.whisper import WhisperRecognizer
    from f5e_tts_amd.infer import audio as A
    monkeypatch.setattr(A, "resample_device", lambda wav, sr, to: wav)
    rec = object.__new__(WhisperRecognizer)
    rec.device, rec.language, rec.model, rec._warned, rec.beam_size = torch.device("cpu"), "english", _StubModel(), set(), 3
    for k, v in attrs.items():
        setattr(rec, k, v)
    return rec


def test_recognizer_long_form_runs_the_loop_on_the_whole_recording(monkeypatch):
    rec = _stub_recognizer(monkeypatch, long_form=True)
    assert rec.transcribe(torch.zeros(40000), 16000) == "w1 w2"
    assert rec.model.calls == [("long", (1, 40000), "english", dict(beam_size=3))]
    assert rec.transcribe_segments(torch.zeros(40000), 16000) == [(0.0, 0.5, " w1"), (1.0, 1.5, " w2")]


def test_recognizer_without_long_form_still_truncates_with_its_warning(monkeypatch):
    rec = _stub_recognizer(monkeypatch)
    with pytest.warns(UserWarning, match="only the first 1 s are transcribed"):
        rec.transcribe(torch.zeros(40000), 16000)
    assert rec.model.calls == [("generate", (1, 16000), "english", dict(beam_size=3))]


def test_recognizer_auto_language_means_detection(monkeypatch):
    for lang in (None, "auto", "AUTO"):
        rec = _stub_recognizer(monkeypatch, language=lang)
        rec.transcribe(torch.zeros(1600), 16000)
        assert rec.model.calls[-1][2] is None
