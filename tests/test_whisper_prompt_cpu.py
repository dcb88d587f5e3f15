"""Whisper's prompt conditioning on the host: the float64 restatement (tests/whisper_prompt_ref.py) against the fixture made from
``transformers`` (tests/golden/whisper_prompt.npz), the pure functions of eval/whisper.py that build a window's decoder input
against both, the byte-level BPE encoder against ``WhisperTokenizer``'s recorded ids, and every refusal, before any launch.

Case (g) (conditioning under a fallback that keeps a window at 0.8, so the next one is not conditioned) is in the fixture; its
rule, ``conditions_next_window``, is also tested by hand and through ``window_prompt``."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import whisper_long_ref as LR
import whisper_prompt_ref as PR
import whisper_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (("f5e_attn_prefill_f32", 16), ("f5e_attn_decode_from_f32", 18), ("f5e_whisper_embed", 12))
FORCED, PREV, TB, CAP, WINDOW = [101, 102, 106], 108, 111, 40, 100
_gold = {}


def gold():
    if not _gold:
        _gold.update(PR.load_fixture())
    return _gold


def case(name):
    got = [c for c in gold()["cases"] if c["name"] == name]
    assert got, f"tests/golden/whisper_prompt.npz has no case ({name})"
    return got[0]


def rows_of(c):
    return range(len(c["waves"]))


def all_rows():
    return [(n, b) for n in "abcdefghi" for b in range(2 if n in "ei" else 1)]


def tiny_cfg(**over):
    from f5e_tts_amd.eval.whisper import WhisperConfig
    gen = dict(gold()["generation_config"])
    gen.update(over)
    return WhisperConfig.from_dicts(gold()["config"], {k: v for k, v in gen.items() if v is not None})


def tiny_model(c):
    from f5e_tts_amd.eval.whisper import Whisper
    model = Whisper(tiny_cfg())
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in LR.case_sd(gold(), c).items()})
    return model


def context_of(c):
    from f5e_tts_amd.eval.whisper import Context
    ctx = dict(c["context"])
    if ctx.get("prompt_ids") is not None:
        ctx["prompt_ids"] = tuple(ctx["prompt_ids"])
    return Context(**ctx)


def ref_run(name, b):
    """The restatement's run of row b of a case, computed once and shared."""
    key = ("run", name, b)
    if key not in _gold:
        fx, c = gold(), case(name)
        lo, hi = c["waves"][b]
        w = fx["wave_f32"][lo:hi]
        T = max(len(w) // 160, WINDOW)
        feats = R.log_mel(w, len(w), T, R.slaney_filters(80))
        thr = (c.get("no_speech_threshold"), c.get("logprob_threshold"))
        _gold[key] = PR.transcribe_prompt_ref(R.Ref(LR.case_sd(fx, c), fx["config"]), feats, FORCED, fx["generation_config"], CAP,
                                              WINDOW, c["context"], c["num_beams"], *thr, fallback=c.get("fallback"))
    return _gold[key]


# ---- the fixture and the restatement ----------------------------------------------------------------------------------------------

def test_fixture_shows_every_case():
    a, b, c, d, e, f, h = (case(n) for n in "abcdefh")
    assert len(a["kinds"][0]) >= 3 and a["context"] == dict(condition_on_prev_tokens=True)
    assert max(len(p) for p in a["prompts"][0]) > 4 and a["prompts"][0][1][0] == PREV
    assert b["context"]["prompt_condition_type"] == "first-segment" and not b["context"]["condition_on_prev_tokens"]
    ids = b["context"]["prompt_ids"]
    assert all(p == ids + FORCED for p in b["prompts"][0])                   # not conditioned: the prompt leads every window
    assert all(PREV not in s["tokens"] for s in b["segments"][0])                # the returned segments never contain it
    ids = c["context"]["prompt_ids"]
    assert c["context"]["prompt_condition_type"] == "all-segments" and all(p[:len(ids)] == ids for p in c["prompts"][0])
    assert "N" in d["kinds"][0] and any(len(p) == 1 + 19 + 3 for p in d["prompts"][0])
    lens = [[len(p) for p in e["prompts"][r]] for r in range(2)]
    assert any(p > 3 and q > 3 and p != q for p, q in zip(lens[0][1:], lens[1][1:])), lens
    assert f["num_beams"] == 3 and f["waves"] == a["waves"] and f["row_scale"] == a["row_scale"]
    assert "k" in h["kinds"][0] and h["kinds"][0][0] != "k" and h["segments"][0]
    i = case("i")                  # in some iteration row 0, the padded one, picks more than the batch's bound would leave it
    lens = [[len(p) for p in i["prompts"][r]] for r in range(2)]
    assert i["bound_iterations"]
    for k in i["bound_iterations"]:
        assert lens[0][k] < lens[1][k] and i["picks"][0][k] > CAP - lens[1][k]
    assert min(i["margins"]) >= 1e-2
    g = case("g")
    kept, lens = g["kept"][0], [len(p) for p in g["prompts"][0]]
    assert g["fallback"]["temperatures"] == [0.0, 0.8] and g["context"] == dict(condition_on_prev_tokens=True)
    assert any(kept[i] == 0.8 and lens[i + 1] == 3 for i in range(len(kept) - 1))      # a window kept at 0.8: the next is not conditioned
    assert any(kept[i] == 0.0 and lens[i + 1] > 3 for i in range(len(kept) - 1))       # one kept at 0: the next is
    assert all(abs(cr - g["fallback"]["compression_ratio_threshold"]) >= 1e-2 for _, _, cr in g["attempts"])
    for x in (a, b, c, d, e, g, h):
        assert min(x["margins"]) >= 1e-2, (x["name"], x["margins"])
    for avg, ns in h["windows"][0]:
        assert abs(ns - h["no_speech_threshold"]) >= 1e-2 and abs(avg - h["logprob_threshold"]) >= 1e-2


@pytest.mark.parametrize("name,b", all_rows())
def test_restatement_reproduces_the_fixture(name, b):
    c = case(name)
    segs, seeks, gaps, kinds, wins = ref_run(name, b)
    want = c["segments"][b]
    assert [s["tokens"] for s in segs] == [s["tokens"] for s in want]
    assert all(abs(s["start"] - q["start"]) < 1e-9 and abs(s["end"] - q["end"]) < 1e-9 for s, q in zip(segs, want))
    T = c["frames"][b]
    assert seeks == [s for s in c["seeks"][b] if s < T]
    assert kinds == c["kinds"][b] and [w["prompt"] for w in wins] == c["prompts"][b]
    if "kept" in c:
        assert [w["temperature"] for w in wins] == c["kept"][b]
    if c["num_beams"] == 1:
        assert min(gaps) >= 1e-2
        for w, (avg, ns) in zip(wins, c.get("windows", [[]])[b]):
            assert abs(w["avg_logprob"] - avg) < 1e-3 and abs(w["no_speech_prob"] - ns) < 1e-3 * max(ns, 1e-3)


# ---- the decoder input of a window ------------------------------------------------------------------------------------------------

def test_rule_function():
    from f5e_tts_amd.eval.whisper import conditions_next_window
    assert [conditions_next_window(t) for t in (None, 0.0, 0.2, 0.4, 0.49999, 0.5, 0.6, 0.8, 1.0)] == \
        [True, True, True, True, True, False, False, False, False]


def test_previous_text_cut_and_skipped_double_timestamp():
    from f5e_tts_amd.eval.whisper import previous_text
    a, b_, c = [TB, 5, 6, TB + 10, TB + 10], [TB + 10, 7, TB + 30], [TB + 2, TB + 2]
    assert previous_text([a], TB, 19) == [TB, 5, 6, TB + 10]                  # a closing pair loses its second timestamp
    assert previous_text([b_], TB, 19) == b_                                   # text, timestamp: kept whole
    assert previous_text([c], TB, 19) == c                                    # two tokens: the rule needs more than two
    assert previous_text([a, b_], TB, 19) == [TB, 5, 6, TB + 10, TB + 10, 7, TB + 30]
    long = [[TB] + list(range(10, 30)) + [TB + 5, TB + 5], [TB + 5, 40, 41, TB + 9]]
    full = [TB] + list(range(10, 30)) + [TB + 5] + [TB + 5, 40, 41, TB + 9]
    assert previous_text(long, TB, 19) == full[-19:] and len(previous_text(long, TB, 19)) == 19
    assert previous_text([], TB, 19) == []
    for hist in ([a], [a, b_, c], long):
        assert previous_text(hist, TB, 19) == PR.previous_text_ref(hist, TB, 19)


def test_window_layouts():
    from f5e_tts_amd.eval.whisper import Context, window_prompt
    hist = [[TB, 5, 6, TB + 10, TB + 10]]
    ids = (PREV, 20, 31)
    wp = lambda ctx, h, cond=True: window_prompt(ctx, FORCED, h, cond, PREV, TB, 19)   # noqa: E731
    assert wp(None, hist) == FORCED and wp(Context(), hist) == FORCED          # context=None / Context(): today's prompt
    cond = Context(condition_on_prev_tokens=True)
    assert wp(cond, []) == FORCED                                              # nothing to condition on yet
    assert wp(cond, hist) == [PREV, TB, 5, 6, TB + 10] + FORCED
    assert wp(cond, hist, False) == FORCED                                     # the last window was kept at a high temperature
    first = Context(prompt_ids=ids)
    assert wp(first, [[20, 31]]) == list(ids) + FORCED and wp(first, [[20, 31]] + hist) == list(ids) + FORCED
    both = Context(condition_on_prev_tokens=True, prompt_ids=ids)
    assert wp(both, [[20, 31]]) == [PREV, 20, 31] + FORCED                      # the prompt is the first previous segment
    assert wp(both, [[20, 31]] + hist) == [PREV, 20, 31, TB, 5, 6, TB + 10] + FORCED
    assert wp(both, [[20, 31]] + hist, False) == list(ids) + FORCED
    every = Context(condition_on_prev_tokens=True, prompt_ids=ids, prompt_condition_type="all-segments")
    assert wp(every, []) == list(ids) + FORCED
    assert wp(every, hist) == list(ids) + [TB, 5, 6, TB + 10] + FORCED
    long = [list(range(10, 40))]
    assert wp(cond, long) == [PREV] + list(range(21, 40)) + FORCED and len(wp(cond, long)) == 23
    assert len(wp(every, long)) == 3 + 19 + 3


@pytest.mark.parametrize("name,b", all_rows())
def test_window_prompts_equal_the_fixture(name, b):
    """``window_prompt`` on the history that the recorded segments give, window by window."""
    from f5e_tts_amd.eval.whisper import window_prompt
    c = case(name)
    ctx = context_of(c)
    segs, seeks = ref_run(name, b)[:2]
    start = PR.start_history(c["context"], PREV)
    from f5e_tts_amd.eval.whisper import conditions_next_window
    kept = c.get("kept", [[0.0] * len(seeks)] * len(c["waves"]))[b]
    for i, seek in enumerate(seeks):
        hist = start + [s["tokens"] for s in segs if s["seek"] < seek]
        conditioned = ctx.condition_on_prev_tokens and (i == 0 or conditions_next_window(kept[i - 1]))
        assert window_prompt(ctx, FORCED, hist, conditioned, PREV, TB, CAP // 2 - 1) == c["prompts"][b][i], (name, i)


# ---- text prompts -----------------------------------------------------------------------------------------------------------------

def tokenizer_model(merges=True):
    from f5e_tts_amd.eval.whisper import Whisper, WhisperConfig
    t = gold()["tokenizer"]
    added = t["added"]
    cfg = WhisperConfig(vocab_size=len(t["vocab"]) + len(added) + 8, num_mel_bins=80, d_model=16, encoder_layers=1,
                        encoder_attention_heads=1, encoder_ffn_dim=16, decoder_layers=1, decoder_attention_heads=1, decoder_ffn_dim=16,
                        max_source_positions=4, max_target_positions=8, eos_token_id=added["<|endoftext|>"],
                        decoder_start_token_id=added["<|startoftranscript|>"], prev_sot_token_id=added["<|startofprev|>"],
                        no_timestamps_token_id=added["<|notimestamps|>"])
    model = Whisper(cfg)
    model.set_vocab(t["vocab"], added)
    if merges:
        model.set_merges(["#version: 0.2"] + t["merges"] + [""])
    return model, t


def test_encode_text_and_prompt_ids_equal_the_tokenizer():
    model, t = tokenizer_model()
    kinds = "".join(r["text"] for r in t["texts"])
    assert any(ord(ch) > 127 for ch in kinds) and any(ch.isdigit() for ch in kinds) and "'ll" in kinds and "   " in kinds
    for r in t["texts"]:
        assert model.encode_text(r["text"]) == r["ids"], r["text"]
        assert model.get_prompt_ids(r["text"]) == r["prompt_ids"], r["text"]
        assert r["prompt_ids"][0] == model.cfg.prev_sot_token_id
        assert model.decode_ids(model.encode_text(r["text"])) == r["text"]          # encode -> decode_ids round trip
        assert model.encode_text(r["text"]) == PR.encode_ref(r["text"], t["vocab"], t["merges"])
    assert model.encode_text("") == []


def test_text_prompt_refusals(tmp_path, monkeypatch):
    import builtins
    from f5e_tts_amd import _C
    from f5e_tts_amd.eval.whisper import Whisper
    model, t = tokenizer_model()
    with pytest.raises(_C.F5EError, match="special token <\\|en\\|>"):
        model.get_prompt_ids(t["refused"])
    bare, _ = tokenizer_model(merges=False)
    with pytest.raises(_C.F5EError, match="merges.txt"):
        bare.encode_text("hello")
    assert bare.decode_ids(t["texts"][0]["ids"]) == t["texts"][0]["text"]            # everything else works without merges
    with pytest.raises(_C.F5EError, match="not a pair"):
        bare.set_merges(["a b c"])
    with pytest.raises(_C.F5EError, match="prev_sot_token_id"):
        Whisper(tiny_cfg(prev_sot_token_id=None)).get_prompt_ids("x")
    real_import = builtins.__import__

    def no_regex(name, *a, **kw):
        if name == "regex":
            raise ImportError("no regex here")
        return real_import(name, *a, **kw)
    monkeypatch.setattr(builtins, "__import__", no_regex)
    with pytest.raises(_C.F5EError, match="'regex' module"):
        model.encode_text("hello")


# ---- refusals, before any launch --------------------------------------------------------------------------------------------------

def test_context_refusals_by_name():
    from f5e_tts_amd import _C
    from f5e_tts_amd.eval.whisper import Context, Whisper, WhisperRecognizer
    with pytest.raises(_C.F5EError, match="all-segments' needs condition_on_prev_tokens"):
        Context(prompt_ids=(PREV, 5), prompt_condition_type="all-segments")
    with pytest.raises(_C.F5EError, match="prompt_condition_type"):
        Context(prompt_condition_type="every-segment")
    with pytest.raises(_C.F5EError, match="must be a bool"):
        Context(condition_on_prev_tokens=1)
    with pytest.raises(_C.F5EError, match="prompt_ids is empty"):
        Context(prompt_ids=())
    with pytest.raises(_C.F5EError, match="not a sequence of token ids"):
        Context(prompt_ids="abc")
    assert Context(prompt_ids=np.array([PREV, 5])).prompt_ids == (PREV, 5)
    model = Whisper(tiny_cfg())
    wav = torch.zeros(1, 16000)                                               # on the host: a launch would be refused as "no CPU path"
    with pytest.raises(_C.F5EError, match="context=Context"):
        model.transcribe_long(wav, condition_on_prev_tokens=True)             # the old names stay refused and point to the new one
    with pytest.raises(_C.F5EError, match="must be a Context or None"):
        model.transcribe_long(wav, context=dict(condition_on_prev_tokens=True))
    with pytest.raises(_C.F5EError, match="must be ids in"):
        model.transcribe_long(wav, context=Context(prompt_ids=(PREV, 162)))
    with pytest.raises(_C.F5EError, match="a prompt of 37 tokens, up to 19 previous tokens and 3 forced tokens make 40 positions"):
        model.transcribe_long(wav, context=Context(prompt_ids=(PREV,) + (5,) * 36))
    with pytest.raises(_C.F5EError, match="a prompt of 18 tokens.* make 40 positions.*max_target_positions = 40"):
        model.transcribe_long(wav, context=Context(True, (PREV,) + (5,) * 17, "all-segments"))
    model._check_context(Context(True, (PREV,) + (5,) * 16, "all-segments"))    # 17 + 19 + 3 = 39 < 40: the largest that fits
    model._check_context(Context(True, (PREV,) + (5,) * 35))                     # first-segment: the prompt scrolls out of the cut
    bare = Whisper(tiny_cfg(prev_sot_token_id=None))
    for ctx in (Context(condition_on_prev_tokens=True), Context(prompt_ids=(5, 6))):
        with pytest.raises(_C.F5EError, match="prev_sot_token_id"):
            bare.transcribe_long(wav, context=ctx)
    with pytest.raises(_C.F5EError, match="there is no CPU path"):              # a valid context gets as far as the audio check
        model.transcribe_long(wav, context=Context(condition_on_prev_tokens=True))
    with pytest.raises(_C.F5EError, match="there is no CPU path"):
        model.transcribe_long(wav, context=None)
    for kw in (dict(initial_prompt="hello"), dict(condition_on_previous_text=True)):
        with pytest.raises(_C.F5EError, match="need long_form=True"):
            WhisperRecognizer("nowhere", **kw)


def test_wiring_is_opt_in():
    from f5e_tts_amd.eval import eval_wer
    from f5e_tts_amd.eval.whisper import Context, Whisper, WhisperRecognizer
    from f5e_tts_amd.infer import infer_cli
    base = ["--metalst", "m", "--gen_wav_dir", "g", "--lang", "en"]
    args = eval_wer.build_parser().parse_args(base)
    assert args.whisper_prompt is None and args.whisper_condition is False
    args = eval_wer.build_parser().parse_args(base + ["--asr", "whisper", "--whisper_long", "--whisper_prompt", "Dr. Who", "--whisper_condition"])
    assert args.whisper_prompt == "Dr. Who" and args.whisper_condition is True
    assert infer_cli.build_parser().parse_args([]).whisper_prompt is None
    assert infer_cli.build_parser().parse_args(["--whisper_prompt", "x"]).whisper_prompt == "x"
    ps = inspect.signature(WhisperRecognizer.__init__).parameters
    assert ps["initial_prompt"].default is None and ps["condition_on_previous_text"].default is False
    assert inspect.signature(Whisper.transcribe_long).parameters["context"].default is None
    ps = inspect.signature(Whisper.generate_from_kv).parameters
    assert ps["begin"].default is None and ps["prefill"].default is False
    assert inspect.signature(Whisper.decoder_logits).parameters["one_pass"].default is False
    assert Context() == Context(False, None, "first-segment")


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------

def test_abi_declares_and_binds_the_three_entries():
    from f5e_tts_amd import _C, ops
    header = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    for name, nargs in ENTRIES:
        m = re.search(r"F5E_API int %s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_C.SIGNATURES[name]), name
        assert hasattr(_C.lib(), name)
    assert callable(ops.attn_prefill_f32) and callable(ops.whisper_embed)
    assert len(_C.SIGNATURES["f5e_attn_decode_f32"]) == 17 and len(_C.SIGNATURES["f5e_text_gather"]) == 11
    assert inspect.signature(ops.attn_decode_f32).parameters["begin"].default is None


def test_c_entries_refuse_bad_arguments_without_a_device():
    """Every check of the entries comes before the launch: null operands and bad limits return an error code."""
    import ctypes as C
    from f5e_tts_amd import _C
    lib = _C.lib()
    fbuf = (C.c_float * 1024)()
    base = C.addressof(fbuf)
    f = C.c_void_p(base + (-base) % 16)                                        # 16-byte aligned
    odd = C.c_void_p(f.value + 4)

    def prefill(**o):
        a = dict(qkv=f, ld=96, kc=f, vc=f, rs=256, ps=32, out=f, ldo=32, R=1, U=2, Umax=8, H=2, dk=16)
        a.update(o)
        return lib.f5e_attn_prefill_f32(None, a["qkv"], a["ld"], a["kc"], a["vc"], a["rs"], a["ps"], None, a["out"], a["ldo"], a["R"],
                                        a["U"], a["Umax"], a["H"], a["dk"], 1.0)
    for bad in (dict(qkv=None), dict(out=None), dict(U=0), dict(U=9), dict(Umax=4097), dict(ld=95), dict(ld=64), dict(ps=16),
                dict(rs=128), dict(ldo=16), dict(dk=8), dict(dk=24), dict(kc=odd), dict(vc=odd), dict(out=odd), dict(R=0), dict(H=0)):
        assert prefill(**bad) != 0, bad
    assert lib.f5e_attn_decode_from_f32(None, f, 96, f, f, 256, 32, None, 0, f, f, 32, 1, 8, 2, 16, 8, 1.0) != 0      # p == Umax
    assert lib.f5e_attn_decode_from_f32(None, f, 96, f, f, 256, 32, None, 0, f, None, 32, 1, 8, 2, 16, 0, 1.0) != 0   # no out
    for bad in (dict(D=6), dict(p0=7), dict(U=0), dict(ids=None), dict(out=odd)):
        a = dict(ids=f, emb=f, pos=f, out=f, R=1, U=2, D=8, p0=0, max_pos=8, rows=4)
        a.update(bad)
        assert lib.f5e_whisper_embed(None, a["ids"], None, a["emb"], a["pos"], a["out"], a["R"], a["U"], a["D"], a["p0"], a["max_pos"],
                                     a["rows"]) != 0, bad
