"""The Qwen2 path, the parts that need no GPU: the restatement of tests/qwen2_ref.py against the ``transformers`` fixtures (logits
to 1e-5 relative L2, greedy tokens, survivor sets with probabilities to 1e-6, the rotary table bit for bit), the tokeniser and
the chat template, every refusal of the configuration by name, the C ABI's declarations, the inverse-CDF draw's frequencies, and
the voice-chat driver's argument parsing and turn bookkeeping on stubs."""
import json
import os
import re
import unicodedata

import numpy as np
import pytest
import torch

import qwen2_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW = (("f5e_rmsnorm_f32", 9), ("f5e_swiglu_f32", 7), ("f5e_llm_embed_f32", 7), ("f5e_llm_embed_w16", 8),
       ("f5e_gqa_rope_append_f32", 21), ("f5e_gqa_rope_decode_dev_f32", 20), ("f5e_llm_pick_dev", 26))
_fx = {}


def fixture():
    if not _fx:
        fx, sd, cfg = Q.load_fixture()
        _fx.update(fx=fx, sd=sd, cfg=cfg, model=Q.Model(sd, cfg))
    return _fx


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


# ---- the restatement against transformers ----------------------------------------------------------------------------------------------

def test_restatement_matches_the_fixture():
    f = fixture()
    fx, m = f["fx"], f["model"]
    from f5e_tts_amd.infer.qwen2 import rotary_table
    for cos, sin in (Q.rotary_table(32, 1e6, 64), tuple(t.numpy() for t in rotary_table(32, 1e6, 64))):
        assert np.array_equal(cos, fx["cos"]) and np.array_equal(sin, fx["sin"])           # bit for bit
    hid = []
    logits = m.append(m.new_caches(2, 16), fx["ids"], fx["begin"], 0, hidden=hid)
    assert rel(logits, fx["logits"]) <= 1e-5
    for i in range(2):
        assert rel(hid[i][0], fx[f"hidden_{i}"][0]) <= 1e-5 and rel(hid[i][1, 4:], fx[f"hidden_{i}"][1, 4:]) <= 1e-5
    toks, caches, table = m.greedy(fx["ids"], fx["begin"], 16, 1.05)
    assert np.array_equal(toks, fx["tokens"])
    assert float(fx["gaps"].min()) >= 1e-2 and all(len(set(r.tolist())) >= 8 for r in fx["tokens"])
    # the second turn behind row 0's own run: the token that was picked but never fed, then the turn's 6 ids
    t0, c0, tab0 = m.greedy(fx["ids"][:1], [0], 16, 1.05)
    assert np.array_equal(t0[0], fx["tokens"][0])
    c0 = [(np.pad(k, ((0, 0), (0, 8), (0, 0))), np.pad(v, ((0, 0), (0, 8), (0, 0)))) for k, v in c0]
    feed = np.concatenate([tab0[0, -1:], fx["turn2_ids"]])[None]
    assert rel(m.append(c0, feed, [0], 9 + 15)[0], fx["turn2_logits"]) <= 1e-5


@pytest.mark.parametrize("V", (384, 151936))
def test_survivors_match_the_processors(V):
    fx = dict(np.load(os.path.join(GOLD, "qwen2_sample.npz")))
    for i, k in enumerate(fx[f"rows_{V}"]):
        x, h = Q.logits_row(V, int(k)), fx[f"hist_{V}"][i]
        assert h.tolist() == Q.history_row(V, int(k), x)
        for si, (pen, T, tk, tp) in enumerate(fx["settings"]):
            ids, e = Q.survivors(x, h, pen, T, int(tk), tp)
            want = fx[f"keep_id_{V}_{si}"][i]
            n = int((want >= 0).sum())
            assert n == len(ids) and np.array_equal(ids, want[:n]), (V, i, si)
            assert np.abs(e / e.sum() - fx[f"keep_p_{V}_{si}"][i][:n]).max() <= 1e-6


def test_inverse_cdf_draw_frequencies():
    fx = dict(np.load(os.path.join(GOLD, "qwen2_sample.npz")))
    x, h = Q.logits_row(384, int(fx["rows_384"][0])), fx["hist_384"][0]
    ids, e = Q.survivors(x, h, 1.05, 0.7, 20, 0.95)
    p = (e / e.sum()).astype(np.float64)
    N = 20000
    w = Q.SR.philox4x32_10((0, np.arange(N, dtype=np.uint64), 5, 2), (77, 0))
    u = Q.SR.uniform(w[0])
    cum = np.cumsum(e.astype(np.float64))
    picks = np.minimum(np.searchsorted(cum, u * cum[-1], side="left"), len(e) - 1)
    assert [Q.draw(e, float(u[i]))[0] for i in range(200)] == picks[:200].tolist()       # the fp32 walk is this draw
    freq = np.bincount(picks, minlength=len(e)) / N
    assert (np.abs(freq - p) <= 4 * np.sqrt(p * (1 - p) / N)).all(), (freq, p)


# ---- tokeniser and template ------------------------------------------------------------------------------------------------------------

def test_tokeniser_matches_the_trained_one_and_round_trips():
    from f5e_tts_amd.infer.qwen2 import Qwen2Tokenizer
    tok = Qwen2Tokenizer.from_dir(os.path.join(GOLD, "qwen2_tok"))
    assert tok.specials == {"<|endoftext|>": 381, "<|im_start|>": 382, "<|im_end|>": 383} and tok.first_special == 381
    with open(os.path.join(GOLD, "qwen2_tok", "cases.json")) as f:
        cases = json.load(f)
    assert len(cases) >= 40
    for c in cases:
        assert tok.encode(c["text"]) == c["ids"], c["text"]
        assert tok.decode_ids(c["ids"], skip_special_tokens=False) == unicodedata.normalize("NFC", c["text"])
    assert tok.decode_ids(tok.encode("<|im_start|>user\nhi<|im_end|>\n")) == "user\nhi\n"


def test_chat_template():
    from f5e_tts_amd._C import F5EError
    from f5e_tts_amd.infer.qwen2 import DEFAULT_SYSTEM, apply_chat_template
    msgs = [dict(role="system", content="Be brief."), dict(role="user", content="Hi"), dict(role="assistant", content="Hello."),
            dict(role="user", content="Bye")]
    assert apply_chat_template(msgs) == ("<|im_start|>system\nBe brief.<|im_end|>\n<|im_start|>user\nHi<|im_end|>\n"
                                         "<|im_start|>assistant\nHello.<|im_end|>\n<|im_start|>user\nBye<|im_end|>\n"
                                         "<|im_start|>assistant\n")
    assert apply_chat_template(msgs[1:2]) == f"<|im_start|>system\n{DEFAULT_SYSTEM}<|im_end|>\n<|im_start|>user\nHi<|im_end|>\n" \
                                             "<|im_start|>assistant\n"
    assert apply_chat_template(msgs[:2], add_generation_prompt=False).endswith("Hi<|im_end|>\n")
    with pytest.raises(F5EError, match="tools are not built"):
        apply_chat_template(msgs, tools=[dict(name="f")])


# ---- configuration ---------------------------------------------------------------------------------------------------------------------

BASE = dict(model_type="qwen2", vocab_size=384, hidden_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
            intermediate_size=256)


@pytest.mark.parametrize("change,match", (
    (dict(model_type="phi3"), "model_type = 'phi3'"),
    (dict(rope_scaling=dict(type="yarn", factor=4.0)), "rope_scaling"),
    (dict(rope_parameters=dict(rope_type="yarn", rope_theta=1e6)), "rope_scaling"),
    (dict(use_sliding_window=True), "use_sliding_window"),
    (dict(layer_types=["full_attention", "sliding_attention"]), "layer_types entry 'sliding_attention'"),
    (dict(hidden_size=64), "head_dim = 16"),
    (dict(num_attention_heads=2, hidden_size=192), "head_dim = 96"),
    (dict(num_attention_heads=18, num_key_value_heads=2, hidden_size=576), "9 query heads per key/value head"),
    (dict(vocab_size=300000), "vocab_size"),
))
def test_config_refusals_by_name(change, match):
    from f5e_tts_amd._C import F5EError
    from f5e_tts_amd.infer.qwen2 import Qwen2Config
    with pytest.raises(F5EError, match=match):
        Qwen2Config.from_dict(dict(BASE, **change))


def test_config_reads_both_spellings_and_generation_defaults():
    from f5e_tts_amd.infer.qwen2 import GenerationDefaults, Qwen2Config
    a = Qwen2Config.from_dict(dict(BASE, rope_theta=5e5))
    b = Qwen2Config.from_dict(dict(BASE, rope_parameters=dict(rope_type="default", rope_theta=5e5), layer_types=["full_attention"] * 2))
    assert a == b and a.head_dim == 32 and a.group == 2 and a.rope_theta == 5e5
    g = GenerationDefaults.from_dict(dict(do_sample=True, top_k=20, top_p=0.8, temperature=0.7, repetition_penalty=1.05,
                                          eos_token_id=[151645, 151643], pad_token_id=151643))
    assert (g.do_sample, g.top_k, g.repetition_penalty, g.eos_token_id, g.pad_token_id) == (True, 20, 1.05, (151645, 151643), 151643)
    assert GenerationDefaults.from_dict({}).top_k == 50


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_three_times_and_the_abi_version_stays():
    from f5e_tts_amd import _C
    with open(os.path.join(ROOT, "include", "f5e_abi.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "exports.map")) as f:
        assert "global: f5e_*;" in f.read()
    with open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "llm.hip")) as f:
        unit = f.read()
    assert re.search(r"#define F5E_ABI_VERSION 2\b", header) and _C.ABI_VERSION == 2
    for name, arity in NEW:
        m = re.search(r"F5E_API int " + name + r"\(([^;]*)\);", header)
        assert m and len(m.group(1).split(",")) == arity, name
        assert len(_C.SIGNATURES[name]) == arity and f'extern "C" int {name}(' in unit, name
    with open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "Makefile")) as f:
        assert " llm.hip" in f.read()


# ---- the driver on stubs ---------------------------------------------------------------------------------------------------------------

class StubSession:
    def __init__(self):
        self.messages, self.calls = [dict(role="system", content="S")], []

    def say(self, text, max_new_tokens, **kw):
        self.calls.append((text, max_new_tokens, kw))
        reply = "" if text == "silence" else f"echo {text}"
        self.messages += [dict(role="user", content=text), dict(role="assistant", content=reply)]
        return reply

    def clear(self):
        self.messages = self.messages[:1]


class StubTranscriber:
    def transcribe(self, path):
        return "what was spoken"


def make_chat(monkeypatch, **kw):
    from f5e_tts_amd.infer import utils_infer as U, voice_chat as VC
    spoken = []

    def infer_process(ref_audio, ref_text, gen_text, model_obj, vocoder, **k):
        spoken.append((gen_text, k))
        return np.full(100, 0.25, np.float32), 24000, None

    def preprocess(audio, text, clip_short=True, show_info=print, transcriber=None):
        return audio, (text if text.strip() else transcriber.transcribe(audio) + ". ")
    monkeypatch.setattr(U, "infer_process", infer_process)
    monkeypatch.setattr(U, "preprocess_ref_audio_text", preprocess)
    s = StubSession()
    return VC.VoiceChat(None, "dit", "voc", "ref.wav", "ref text", StubTranscriber(), session=s, **kw), s, spoken


def test_driver_turn_bookkeeping(monkeypatch, tmp_path):
    from f5e_tts_amd.infer import voice_chat as VC
    vc, s, spoken = make_chat(monkeypatch, max_new_tokens=32)
    assert vc.say("  ") is None and vc.say() is None and not s.calls                 # an empty message returns nothing
    reply, wave, sr = vc.say("hello")
    assert reply == "echo hello" and len(wave) == 100 and sr == 24000
    assert spoken[0][0] == "echo hello" and spoken[0][1]["cross_fade_duration"] == 0.15 and spoken[0][1]["speed"] == 1.0
    assert s.calls[0] == ("hello", 32, dict(seed=0, step_graph=False, do_sample=True, temperature=0.7, top_p=0.95))
    reply, wave, _ = vc.say(audio="q.wav")                                            # a spoken message goes through the transcriber
    assert reply == "echo what was spoken." and s.calls[1][2]["seed"] == 1
    reply, wave, _ = vc.say("silence")                                                # an empty reply skips synthesis
    assert reply == "" and len(wave) == 0 and len(spoken) == 2
    conv = VC.run_turns(vc, [("text", "again"), ("text", " "), ("audio", "a.wav")], str(tmp_path), seed=5,
                        save_wav=lambda path, w, sr: open(path, "wb").close())
    assert [m["role"] for m in conv] == ["system"] + ["user", "assistant"] * 5
    assert sorted(os.listdir(tmp_path)) == ["conversation.json", "turn_00.wav", "turn_02.wav"]
    with open(tmp_path / "conversation.json") as f:
        assert json.load(f) == conv
    assert s.calls[-1][2]["seed"] == 7
    vc.clear()
    assert vc.turns == 0 and len(vc.conversation) == 1
    g, _, _ = make_chat(monkeypatch, greedy=True, step_graph=True)
    assert g.gen == dict(do_sample=False) and g.step_graph


def test_driver_argument_parsing():
    from f5e_tts_amd.infer import voice_chat as VC
    a = VC.build_parser().parse_args(["--chat_model", "dir", "--input_text", "one", "--input_audio", "two.wav", "--input_text", "three"])
    assert a.turns == [("text", "one"), ("audio", "two.wav"), ("text", "three")]
    assert (a.temperature, a.top_p, a.max_new_tokens, a.greedy, a.chat_seed, a.chat_step_graph, a.chat_weights) == \
        (0.7, 0.95, 512, False, 0, False, "auto")
    assert a.system_prompt == VC.DEFAULT_SYSTEM_PROMPT and a.system_prompt.startswith("You are not an AI assistant")
    b = VC.build_parser().parse_args(["--chat_model", "d", "--greedy", "--chat_step_graph", "--chat_seed", "9", "--chat_weights", "bf16"])
    assert b.greedy and b.chat_step_graph and b.chat_seed == 9 and not getattr(b, "turns", None)
    with pytest.raises(SystemExit):
        VC.main(["--chat_model", "d"])
    with pytest.raises(SystemExit):
        VC.build_parser().parse_args(["--input_text", "x"])
