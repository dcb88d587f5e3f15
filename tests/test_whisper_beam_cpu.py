"""Whisper's beam search, the parts that need no GPU: the float64 restatement (tests/whisper_beam_ref.py) against the fixture made
from ``transformers``' ``generate(num_beams=5)`` (tests/golden/whisper_beam.npz, tests/golden/make_whisper_beam_golden.py), the C
ABI entries and the opt-in wiring.

Restatement gate: all K pool sequences and lengths equal, scores within 1e-4: one tenth of the 1e-3 nats that the generator asserts
for every deciding gap of every stored case (the fixture's scores are fp32 arithmetic)."""
import os
import re

import numpy as np
import pytest
import torch

import whisper_beam_ref as BR
import whisper_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_TOL = 1e-4
ENTRIES = (("f5e_whisper_beam_scratch", 4), ("f5e_whisper_beam_step", 30))

_gold = {}


def gold():
    """The fixture, loaded once and shared (read-only)."""
    if not _gold:
        _gold.update(BR.load_fixture())
    return _gold


def case(i):
    """-> dict(model index, samples of the audio prefix, cap, steps, eos row f32, enc, tokens, lens, scores, greedy, tags)."""
    fx = gold()
    m, n, cap, steps = (int(v) for v in fx[f"case_{i}"])
    return dict(m=m, n=n, cap=cap, steps=steps, eos_row=(fx[f"eos_row_{i}"].astype(np.uint32) << 16).view(np.float32),
                enc=fx[f"enc_{i}"], tokens=fx[f"tokens_{i}"], lens=fx[f"lens_{i}"], scores=fx[f"scores_{i}"],
                greedy=fx[f"greedy_{i}"], tags=str(fx[f"tags_{i}"]), gap=float(fx[f"gap_{i}"]))


def case_sd(i):
    """The decoder's weights of case i (float32 arrays under the Hugging Face names), its own eos row in the tied embedding."""
    fx, c = gold(), case(i)
    sd = dict(fx["models"][c["m"]])
    emb = sd["model.decoder.embed_tokens.weight"].copy()
    emb[fx["config"]["eos_token_id"]] = c["eos_row"]
    sd["model.decoder.embed_tokens.weight"] = emb
    return sd


def tiny_cfg(**over):
    from f5e_tts_amd.eval.whisper import WhisperConfig
    fx = gold()
    gen = dict(fx["generation_config"])
    gen.update(over)
    return WhisperConfig.from_dicts(fx["config"], gen)


def tiny_model(i):
    """The device module with case i's decoder (the encoder keeps its initial weights: the tests start from ``enc``)."""
    from f5e_tts_amd.eval.whisper import Whisper
    model = Whisper(tiny_cfg())
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in case_sd(i).items()}, strict=False)
    return model


# ---- restatement against the fixture ----

def test_fixture_cases_meet_their_conditions():
    fx = gold()
    cases = [case(i) for i in range(fx["n_cases"])]
    tags = "".join(c["tags"] for c in cases)
    assert all(t in tags for t in "abd") and tags.count("c") >= 2 and int(fx["n_models"]) <= 2
    assert all(c["gap"] >= 1e-3 for c in cases)
    n0 = len(fx["prompt"])
    for c in cases:
        if "a" in c["tags"]:
            assert c["cap"] == n0 + 12 and n0 - 1 + c["steps"] == c["cap"] - 1
        if "b" in c["tags"]:
            assert n0 - 1 + c["steps"] < c["cap"] - 1 and len(set(c["lens"].tolist())) >= 2
        if "c" in c["tags"]:
            assert c["tokens"][0, :c["lens"][0]].tolist() != c["greedy"].tolist()
        if "d" in c["tags"]:
            assert c["steps"] >= 12 and n0 - 1 + c["steps"] < c["cap"] - 1


@pytest.mark.parametrize("i", range(3))
def test_restatement_reproduces_the_fixture(i):
    fx, c = gold(), case(i)
    g = fx["generation_config"]
    ref = R.Ref(case_sd(i), fx["config"])
    toks, lens, scores, steps, gap = BR.beam_search_ref(ref, c["enc"].astype(np.float64), fx["prompt"].tolist(), g["suppress_tokens"],
                                                        g["begin_suppress_tokens"], g["eos_token_id"], c["cap"], int(fx["K"]))
    err = float(np.abs(scores - c["scores"]).max())
    print(f"case {i} ({c['tags']}): {steps} steps, lens {lens.tolist()}, score error {err:.2e} (gate {SCORE_TOL:g}), gap {gap:.2e}")
    assert lens.tolist() == c["lens"].tolist() and (toks == c["tokens"]).all()
    assert err < SCORE_TOL and steps == c["steps"]
    assert gap >= 1e-3


def test_step_ref_tie_and_pool_order():
    """The hand case of the rules: ties go to the lower row, then the lower class; an old pool entry stays before a newcomer
    of equal score; hit candidates ranked K .. 2K-1 neither run nor enter."""
    K, V, eos, n0, p = 2, 6, 5, 1, 1
    st = BR.new_state(1, K, 4, [0], eos)
    st["score"][:] = [0.0, 0.0]
    st["pool_n"][0], st["pool_len"][0, 0], st["pool_score"][0, 0] = 1, 2, -1.0
    x = np.full((2, V), -50.0)
    x[0, 1] = x[1, 1] = 0.0                    # equal best candidates in both rows: row 0 first
    x[0, eos] = x[1, eos] = -2.0               # ranked 2 and 3 of 2K = 4: hit, but not among the first K
    out, _ = BR.beam_step_ref(x, st, p, n0, 10, eos, K)
    assert out["hyp"][:, p + 1].tolist() == [1, 1] and out["anc"][:, p].tolist() == [0, 1]
    assert out["pool_n"][0] == 1 and out["open"][0] == 1 and out["alive"][0] == 1
    x[0, eos] = 1.0                            # now the best candidate: enters with value / 2, equal to nothing
    st["pool_score"][0, 0] = -np.log(np.exp(x[0] - 1.0).sum()) / 2.0
    out, _ = BR.beam_step_ref(x, st, p, n0, 10, eos, K)
    assert out["pool_n"][0] == 2 and out["pool_len"][0].tolist() == [2, 3]     # the old entry first at equal score
    assert out["hyp"][:, p + 1].tolist() == [1, 1] and out["anc"][:, p].tolist() == [1, 0]
    assert out["open"][0] == 1                 # the pool is full, but the best open row still beats its worst entry
    st["pool_score"][0, 0], st["pool_score"][0, 1], st["pool_n"][0], st["pool_len"][0, 1] = -0.01, -0.02, 2, 3
    out, _ = BR.beam_step_ref(x, st, p, n0, 10, eos, K)
    assert out["pool_len"][0].tolist() == [2, 3] and out["open"][0] == 0 and out["alive"][0] == 0    # now it cannot: closed


# ---- C ABI ----

def test_abi_declares_and_binds_the_two_entries():
    from f5e_tts_amd import _C
    header = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    for name, nargs in ENTRIES:
        m = re.search(r"F5E_API int %s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_C.SIGNATURES[name]), name
    assert "#define F5E_ABI_VERSION 2 " in header and _C.ABI_VERSION == 2       # functions were only added
    from f5e_tts_amd import ops
    assert callable(ops.whisper_beam_step) and callable(ops.whisper_beam_scratch)


# ---- wiring ----

def test_whisper_beam_defaults_to_one_in_both_parsers():
    from f5e_tts_amd.eval import eval_wer
    from f5e_tts_amd.infer import infer_cli
    args = eval_wer.build_parser().parse_args(["--metalst", "m", "--gen_wav_dir", "g", "--lang", "en"])
    assert args.whisper_beam == 1 and args.beam_size == 10
    assert eval_wer.build_parser().parse_args(["--metalst", "m", "--gen_wav_dir", "g", "--lang", "en", "--whisper_beam", "5"]).whisper_beam == 5
    assert infer_cli.build_parser().parse_args([]).whisper_beam == 1
    assert infer_cli.build_parser().parse_args(["--whisper_beam", "5"]).whisper_beam == 5


class _StubModel:
    n_frames = 300

    def __init__(self):
        self.calls = []

    def generate(self, audio, lens, language, **kw):
        self.calls.append(kw)
        return torch.tensor([[1, 2, 3]]), torch.tensor([3])

    def decode_ids(self, ids):
        return " ok "


@pytest.mark.parametrize("own", (1, 5))
def test_transcribe_accepts_and_ignores_the_wenet_beam_size(own, monkeypatch):
    from f5e_tts_amd.eval.whisper import WhisperRecognizer
    from f5e_tts_amd.infer import audio as A
    monkeypatch.setattr(A, "resample_device", lambda wav, sr, to: wav)
    rec = object.__new__(WhisperRecognizer)
    rec.device, rec.language, rec.model, rec._warned, rec.beam_size = torch.device("cpu"), "english", _StubModel(), set(), own
    assert rec.transcribe(torch.zeros(1600), 16000, mode="ctc_greedy_search", beam_size=10) == "ok"
    assert rec.model.calls == [dict(beam_size=own)]                 # the constructor's, never run_asr_wer's keyword


def test_recognizer_takes_beam_size_and_defaults_to_greedy(monkeypatch):
    import inspect
    from f5e_tts_amd.eval.whisper import Whisper, WhisperRecognizer
    sig = inspect.signature(WhisperRecognizer.__init__)
    assert sig.parameters["beam_size"].default == 1
    for fn in (Whisper.generate, Whisper.generate_from_kv):
        ps = inspect.signature(fn).parameters
        assert ps["beam_size"].default == 1 and ps["length_penalty"].default == 1.0 and ps["return_beams"].default is False


def test_beam_size_one_takes_the_greedy_path(monkeypatch):
    from f5e_tts_amd import _C
    from f5e_tts_amd.eval.whisper import Whisper
    model = Whisper(tiny_cfg())
    kv = [(torch.zeros(1, 150, 64), torch.zeros(1, 150, 64))] * 2

    def no_beam(*a, **k):
        raise AssertionError("the beam search ran")
    monkeypatch.setattr(Whisper, "_beam_from_kv", no_beam)
    with pytest.raises(_C.F5EError, match="there is no CPU path"):     # the greedy path's first act: fold the weights for the GPU
        model.generate_from_kv(kv, [141, 142, 146, 159])
    with pytest.raises(_C.F5EError, match="there is no CPU path"):
        model.generate_from_kv(kv, [141, 142, 146, 159], beam_size=1)
    with pytest.raises(AssertionError, match="the beam search ran"):
        model.generate_from_kv(kv, [141, 142, 146, 159], beam_size=2)


def test_too_few_unsuppressed_classes_are_refused():
    from f5e_tts_amd import _C
    from f5e_tts_amd.eval.whisper import Whisper
    kv = [(torch.zeros(1, 150, 64), torch.zeros(1, 150, 64))] * 2
    model = Whisper(tiny_cfg(suppress_tokens=list(range(0, 149)), begin_suppress_tokens=[149, 150, 0]))   # 160 - 151 = 9 < 10
    with pytest.raises(_C.F5EError, match="needs 10 classes"):
        model.generate_from_kv(kv, [141, 142, 146, 159], beam_size=5)
    with pytest.raises(_C.F5EError, match="there is no CPU path"):     # 2 K = 8 <= 9: passes this check, stops at the device's
        model.generate_from_kv(kv, [141, 142, 146, 159], beam_size=4)
    with pytest.raises(_C.F5EError, match="1 .. 16"):
        Whisper(tiny_cfg()).generate_from_kv(kv, [141, 142, 146, 159], beam_size=17)
