"""Whisper's assisted generation (speculative decoding), the parts that need no GPU: the float64 restatement of the round
(tests/whisper_assist_ref.py: draft, verify, accept, common advance) against the tokens ``transformers``' assisted generation returned
(tests/golden/whisper_assist.npz, tests/golden/make_whisper_assist_golden.py) and against the plain greedy tokens of whisper.npz and
whisper_long.npz with three drafts (the target itself, the target's decoder with seeded noise, a seeded random model); the accept
rule on hand-made cases; the C ABI entries; the refusals, which come before any launch.

Everything here is exact: tokens, lengths, segments and seeks are compared for equality (the fixtures' steps keep margins of at
least 1e-2 of the logits' RMS, and the restatement is float64 on both sides)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import test_whisper_cpu as WC
import test_whisper_long_cpu as LC
import whisper_assist_ref as AR
import whisper_long_ref as LR
import whisper_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (("f5e_attn_append_f32", 17), ("f5e_whisper_verify", 19), ("f5e_whisper_accept", 16), ("f5e_gemm_f32_skinny_workspace", 3),
           ("f5e_gemm_f32_skinny", 16))
DRAFTS = ("self", "noisy", "random")
N_DRAFT = 5

_gold = {}


def gold():
    """tests/golden/whisper_assist.npz, loaded once and shared (read-only)."""
    if not _gold:
        _gold.update(AR.load_fixture())
    return _gold


def draft_sd(sd, kind):
    """The three drafts of a target's weights ``sd``."""
    return sd if kind == "self" else AR.noisy_decoder_sd(sd) if kind == "noisy" else AR.random_sd(sd)


def short_case(name):
    """A case of whisper.npz: (samples, the model with the scaled eos row?, the plain greedy tokens)."""
    fx = WC.gold()
    return (14400, True, fx["tokens_eos"].tolist()) if name == "eos" else (int(name), False, fx[f"tokens_{name}"].tolist())


def target_sd(eos_case):
    return {k: np.asarray(v, dtype=np.float32) for k, v in WC.ref_model(eos_case).sd.items()}


# ---- the restatement ----

@pytest.mark.parametrize("name", ("14400", "40000", "48000", "eos"))
def test_restatement_reproduces_transformers_assisted_generation(name):
    """The fixture's draft (another width, its own encoder), 4 drafts per round, the bound the fixture was made with."""
    fx, wx = gold(), WC.gold()
    c = [c for c in fx["cases"] if c["name"] == name][0]
    n, eos_case, plain = short_case(name)
    assert c["samples"] == n and c["eos_case"] == eos_case and int(fx["num_assistant_tokens"]) == 4
    gc, prompt = wx["generation_config"], wx["prompt"].tolist()
    cap = len(prompt) + c["max_new_tokens"]
    assert c["tokens"] == plain[:cap]                                    # what transformers returned IS the plain greedy run
    ref, dref = WC.ref_model(eos_case), R.Ref(fx["sd"], fx["config"])
    feats = WC.ref_features(n)
    rows, _, stats, adv = AR.assisted_ref(AR.model_fn(ref, [ref.encoder(feats)]), AR.model_fn(dref, [dref.encoder(feats)]), [prompt],
                                          cap, 4, gc["eos_token_id"], AR.plain_pick(gc))
    print(f"case {name}: {stats}, advances {adv}")
    assert rows[0] == c["tokens"] and stats == c["ref_stats"] and sum(adv) == len(c["tokens"]) - len(prompt)


@pytest.mark.parametrize("kind", DRAFTS)
@pytest.mark.parametrize("name", ("14400", "40000", "48000", "eos"))
def test_restatement_equals_plain_greedy_on_the_short_cases(name, kind):
    wx = WC.gold()
    n, eos_case, plain = short_case(name)
    gc, prompt, cap = wx["generation_config"], wx["prompt"].tolist(), wx["config"]["max_target_positions"]
    ref = WC.ref_model(eos_case)
    dref = R.Ref(draft_sd(target_sd(eos_case), kind), wx["config"])
    feats = WC.ref_features(n)
    enc = ref.encoder(feats)
    rows, _, stats, adv = AR.assisted_ref(AR.model_fn(ref, [enc]), AR.model_fn(dref, [enc if kind == "self" else dref.encoder(feats)]),
                                          [prompt], cap, N_DRAFT, gc["eos_token_id"], AR.plain_pick(gc))
    print(f"case {name}, draft {kind}: {stats}")
    assert rows[0] == plain
    if kind == "self":                                                   # full acceptance in every round but the last
        assert all(a == min(N_DRAFT, cap - 2 - p) + 1 for a, p in zip(adv[:-1], np.cumsum([len(prompt) - 1] + adv[:-1])))
    if kind == "random":                                                 # never right, by a margin that fp32 cannot close
        gap = AR.draft_gap(dref, dref.encoder(feats), plain, len(prompt), gc)
        print(f"case {name}: the random draft stays {gap:.3f} of its logits' RMS away from the target's tokens")
        assert gap >= 1e-2 and stats["accepted"] == 0 and stats["rounds"] == len(plain) - len(prompt)


@pytest.mark.parametrize("kind", DRAFTS)
@pytest.mark.parametrize("name,b", [("a", 0), ("b", 0), ("c", 0), ("d", 0), ("e", 0), ("f", 0), ("f", 1), ("g", 0), ("h", 0)])
def test_restatement_equals_plain_greedy_on_the_long_cases(name, b, kind):
    """Segments, tokens and seeks of the assisted seek loop equal the plain greedy one's (case h is the beam case of the fixture:
    its model and wave are decoded greedily here, on both sides)."""
    fx, c = LC.gold(), LC.case(name)
    sd = LR.case_sd(fx, c)
    ref, dref = R.Ref(sd, fx["config"]), R.Ref(draft_sd(sd, kind), fx["config"])
    w = LC.case_wave(c, b)
    feats = R.log_mel(w, len(w), max(len(w) // 160, LC.WINDOW), R.slaney_filters(80))
    gen, prompt = fx["generation_config"], fx["prompt"].tolist()
    thr = (c.get("no_speech_threshold"), c.get("logprob_threshold"))
    key = ("plain", name, b)
    if key not in _gold:
        _gold[key] = LR.transcribe_long_ref(ref, feats, prompt, gen, LC.CAP, LC.WINDOW, 1, *thr)
    want, want_seeks = _gold[key][:2]
    segs, seeks, tot = AR.transcribe_long_assisted_ref(ref, dref, feats, prompt, gen, LC.CAP, LC.WINDOW, N_DRAFT, *thr,
                                                       denc_of=(lambda win, enc: enc) if kind == "self" else None)
    print(f"case {name}[{b}], draft {kind}: {tot}")
    assert [s["tokens"] for s in segs] == [s["tokens"] for s in want] and seeks == want_seeks
    assert [(s["start"], s["end"], s["seek"]) for s in segs] == [(s["start"], s["end"], s["seek"]) for s in want]
    assert max([abs(s["avg_logprob"] - q["avg_logprob"]) for s, q in zip(segs, want)] + [0.0]) < 1e-9
    if c.get("num_beams", 1) == 1:                                       # ... and the fixture's own
        assert [s["tokens"] for s in segs] == [s["tokens"] for s in c["segments"][b]]
    if kind == "self":
        assert tot["accepted"] >= tot["drafted"] - N_DRAFT * len(seeks)


def test_restatement_batch_advances_together_and_rows_stay_their_own():
    """Two rows of different lengths with a noisy draft: the common advance is the smaller one, and every row is its B = 1 run."""
    wx = WC.gold()
    gc, prompt, cap = wx["generation_config"], wx["prompt"].tolist(), wx["config"]["max_target_positions"]
    ref = WC.ref_model(True)
    dref = R.Ref(draft_sd(target_sd(True), "noisy"), wx["config"])
    encs = [ref.encoder(WC.ref_features(n)) for n in (14400, 40000)]
    dencs = [dref.encoder(WC.ref_features(n)) for n in (14400, 40000)]
    pick = AR.plain_pick(gc)
    both, _, stats, adv = AR.assisted_ref(AR.model_fn(ref, encs), AR.model_fn(dref, dencs), [prompt, prompt], cap, N_DRAFT,
                                          gc["eos_token_id"], pick)
    alone = [AR.assisted_ref(AR.model_fn(ref, [e]), AR.model_fn(dref, [d]), [prompt], cap, N_DRAFT, gc["eos_token_id"], pick)
             for e, d in zip(encs, dencs)]
    assert both == [a[0][0] for a in alone]
    assert stats["rounds"] >= max(a[2]["rounds"] for a in alone) and len(both[0]) != len(both[1])


# ---- the accept rule ----

@pytest.mark.parametrize("case", AR.ACCEPT_CASES, ids=[c["name"] for c in AR.ACCEPT_CASES])
def test_accept_rule_by_hand(case):
    logp = AR.accept_logp(case)
    a, new, after, inc = AR.accept_ref(case["cand"], logp, case["drafts"], case["done"], AR.ACCEPT_EOS)
    assert (a, new, [int(d) for d in after]) == (case["a"], case["new"], case["after"])
    assert inc == [sum(logp[r][:k]) for r, k in enumerate(case["kept"])]
    assert 1 <= a <= len(case["cand"][0])


def test_accept_cases_cover_the_list():
    names = " | ".join(c["name"] for c in AR.ACCEPT_CASES)
    for word in ("no match", "bonus", "eos in the middle", "drafted but not picked", "done row beside", "different m", "U = 1"):
        assert word in names, word


# ---- C ABI ----

def test_abi_declares_exports_and_binds_the_entries():
    from f5e_tts_amd import _C, ops
    header = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    exports = open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*f5e_\*;", exports)                      # the version script exports the f5e_ prefix
    for name, nargs in ENTRIES:
        m = re.search(r"F5E_API int %s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_C.SIGNATURES[name]), name
        assert hasattr(_C.lib(), name)
    for fn in ("attn_append_f32", "gemm_f32_skinny", "gemm_f32_skinny_workspace", "whisper_verify", "whisper_accept"):
        assert callable(getattr(ops, fn)), fn
    mk = open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "Makefile")).read()
    assert mk.count("whisper_append") >= 3 and "gemm_f32_skinny.hip" in mk   # the unit, and the MFMA flag in both build lines


def test_c_entries_refuse_bad_arguments_without_a_device():
    """Every check of the entries comes before the launch: null operands and bad limits return an error code."""
    import ctypes as C
    from f5e_tts_amd import _C
    lib = _C.lib()
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(R=1, U=2, Umax=8, H=1, dk=16, p0=2)

    def append(**kw):
        a = dict(ok, **kw)
        return lib.f5e_attn_append_f32(None, kw.get("qkv", p), 48, p, p, 8 * 16, 16, None, p, 16, a["R"], a["U"], a["Umax"], a["H"], a["dk"],
                                       a["p0"], 0.25)
    for bad in (dict(p0=-1), dict(p0=7), dict(U=0), dict(dk=24), dict(qkv=None), dict(R=0)):
        assert append(**bad) != 0, bad
        assert b"attn_append_f32" in lib.f5e_last_error()

    def skinny(M=4, N=8, K=16, act=0, lda=16, A=p, ws=None, nbytes=0):
        return lib.f5e_gemm_f32_skinny(None, A, lda, p, 16, None, act, None, 0, p, 8, ws, nbytes, M, N, K)
    for bad in (dict(M=17), dict(M=0), dict(K=6), dict(K=0), dict(act=1), dict(lda=8), dict(A=None), dict(N=0)):
        assert skinny(**bad) != 0, bad
        assert b"gemm_f32_skinny" in lib.f5e_last_error()
    n = C.c_ulonglong(7)
    assert lib.f5e_gemm_f32_skinny_workspace(8, 16, C.byref(n)) == 0 and n.value == 0   # nothing to split
    assert lib.f5e_gemm_f32_skinny_workspace(0, 16, C.byref(n)) != 0

    def verify(R=1, U=2, V=8, p_=3, n0=2, eos=1, no_ts=-1, ld_hist=8, logits=p):
        return lib.f5e_whisper_verify(None, logits, 8, None, 0, None, 0, p, ld_hist, p, p, R, U, V, p_, n0, eos, no_ts, -1)
    for bad in (dict(logits=None), dict(V=1), dict(p_=0), dict(ld_hist=5), dict(eos=8), dict(no_ts=7), dict(no_ts=0), dict(R=0)):
        assert verify(**bad) != 0, bad
        assert b"whisper_verify" in lib.f5e_last_error()

    def accept(R=1, U=2, p_=3, ld=8, cand=p):
        return lib.f5e_whisper_accept(None, cand, p, p, ld, p, ld, p, p, p, None, p, R, U, p_, 1)
    for bad in (dict(cand=None), dict(U=0), dict(ld=6), dict(R=0), dict(p_=-1)):
        assert accept(**bad) != 0, bad
        assert b"whisper_accept" in lib.f5e_last_error()


# ---- the refusals come before any launch (everything here lives on the CPU: a launch would raise another error) ----

def test_refusals_by_name():
    from f5e_tts_amd import _C
    from f5e_tts_amd.eval.whisper import Whisper, WhisperConfig
    model, draft = WC.tiny_model(), WC.tiny_model()
    wav = torch.zeros(1, 16000)
    kv = [(torch.zeros(1, 150, 64), torch.zeros(1, 150, 64))] * 2
    prompt = WC.gold()["prompt"].tolist()

    def refused(match, **kw):
        with pytest.raises(_C.F5EError, match=match):
            model.generate(wav, None, "en", **kw)
        kw.pop("assistant_shares_encoder", None)
        with pytest.raises(_C.F5EError, match=match):
            model.generate_from_kv(kv, prompt, **dict(kw, assistant=(kw["assistant"], kv)))
    refused("beam_size", assistant=draft, beam_size=2)
    refused("beam_size", assistant=draft, return_beams=True)
    refused("temperature", assistant=draft, temperature=0.5)
    refused("num_assistant_tokens", assistant=draft, num_assistant_tokens=0)
    refused("num_assistant_tokens", assistant=draft, num_assistant_tokens=2.5)
    refused("must be a Whisper", assistant="turbo")
    base = dict(WC.gold()["config"])
    gen = dict(WC.gold()["generation_config"])
    for field, cfg_over, gen_over in (("vocab_size", dict(vocab_size=161), {}), ("eos_token_id", dict(eos_token_id=139), {}),
                                      ("max_target_positions", dict(max_target_positions=40), {}),
                                      ("suppress_tokens", {}, dict(suppress_tokens=[1, 2])),
                                      ("begin_suppress_tokens", {}, dict(begin_suppress_tokens=[5]))):
        other = Whisper(WhisperConfig.from_dicts(dict(base, **cfg_over), dict(gen, **gen_over)))
        refused(field, assistant=other)
    with pytest.raises(_C.F5EError, match="assistant must be"):
        model.generate_from_kv(kv, prompt, assistant=draft)
    narrow = Whisper(WhisperConfig.from_dicts(gold()["config"], gen))                   # the fixture's draft: another width
    with pytest.raises(_C.F5EError, match="d_model"):
        model.generate(wav, None, "en", assistant=narrow, assistant_shares_encoder=True)
    with pytest.raises(_C.F5EError, match="beam_size"):
        model.transcribe_long(wav, None, "en", assistant=draft, beam_size=3)
    with pytest.raises(_C.F5EError, match="num_assistant_tokens"):
        model.transcribe_long(wav, None, "en", assistant=draft, num_assistant_tokens=-1)


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from f5e_tts_amd import _C, ops
    z = torch.zeros
    with pytest.raises(_C.F5EError, match="attn_append_f32"):
        ops.attn_append_f32(z(4, 48), z(2, 8, 16), z(2, 8, 16), 2, 0, 1, 0.25)
    with pytest.raises(_C.F5EError, match="gemm_f32_skinny"):
        ops.gemm_f32_skinny(z(17, 16), z(8, 16), out=z(17, 8))
    with pytest.raises(_C.F5EError, match="whisper_verify"):
        ops.whisper_verify(z(3, 8), z(1, 8, dtype=torch.int32), z(1, 2, dtype=torch.int32), z(1, 2), 3, 2, 1)
    with pytest.raises(_C.F5EError, match="whisper_accept"):
        ops.whisper_accept(z(1, 1, dtype=torch.int32), z(1, 1), z(1, 8, dtype=torch.int32), z(1, 8, dtype=torch.int32),
                           z(1, dtype=torch.int32), z(1, dtype=torch.int32), z(1, dtype=torch.int32), None, z(1, dtype=torch.int32), 3, 1)


def test_wiring_is_opt_in():
    """Without an assistant nothing changes: the new arguments default to off everywhere, and ``layer`` keeps its GEMM."""
    from f5e_tts_amd import xfmr_f32
    from f5e_tts_amd.eval import eval_wer, whisper
    from f5e_tts_amd.infer import infer_cli
    sig = inspect.signature
    assert sig(xfmr_f32.layer).parameters["gemm"].default is None
    for fn in (whisper.Whisper.generate, whisper.Whisper.transcribe_long, whisper.Whisper.generate_from_kv):
        assert sig(fn).parameters["assistant"].default is None and sig(fn).parameters["num_assistant_tokens"].default == 5
    assert sig(whisper.Whisper.generate).parameters["assistant_shares_encoder"].default is False
    rec = sig(whisper.WhisperRecognizer.__init__).parameters
    assert rec["assistant_dir"].default is None and rec["num_assistant_tokens"].default == 5
    assert rec["assistant_shares_encoder"].default is False
    base = ["--gen_wav_dir", "d", "--metalst", "m", "--lang", "en"]
    args = eval_wer.build_parser().parse_args(base)
    assert args.whisper_assistant is None and args.whisper_assistant_tokens == 5 and args.whisper_assistant_shares_encoder is False
    args = eval_wer.build_parser().parse_args(base + ["--asr", "whisper", "--whisper_assistant", "T", "--whisper_assistant_tokens", "3",
                                                      "--whisper_assistant_shares_encoder"])
    assert (args.whisper_assistant, args.whisper_assistant_tokens, args.whisper_assistant_shares_encoder) == ("T", 3, True)
    assert infer_cli.build_parser().parse_args([]).whisper_assistant is None
    assert infer_cli.build_parser().parse_args(["--whisper_assistant", "T"]).whisper_assistant == "T"
