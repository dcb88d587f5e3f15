"""Whisper's sampled step and temperature fallback, the parts that need no GPU: the counter noise of tests/whisper_sample_ref.py
against the published Philox4x32-10 known answers, its draws against softmax(x / T) (chi-square), the float64 restatement against
the fixture made from ``transformers`` (tests/golden/whisper_fallback.npz, tests/golden/make_whisper_fallback_golden.py), the
refusals of ``Fallback``, ``generate`` and ``transcribe_long``, the C ABI entry, the opt-in wiring, and the proof that the inputs
of the GPU step tests leave no undecided draw in the restatement.

Restatement gates: tokens, seeks, temperatures and flags exact (the generator asserts a margin of 1e-2 of the logits' RMS for every
pick, greedy or sampled, and every timestamp / text comparison), times within 1e-9, compression ratios exact, ``avg_logprob`` within
1e-5 (the fixture's are fp32 arithmetic)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import whisper_long_ref as LR
import whisper_ref as R
import whisper_sample_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW, CAP = 100, 40
_gold = {}


def fb_gold():
    """The fixture, loaded once and shared (read-only)."""
    if not _gold:
        _gold.update(S.load_fixture())
    return _gold


def fb_case(name):
    return [c for c in fb_gold()["cases"] if c["name"] == name][0]


def fb_model(c):
    from f5e_tts_amd.eval.whisper import Whisper, WhisperConfig
    fx = fb_gold()
    model = Whisper(WhisperConfig.from_dicts(fx["config"], dict(fx["generation_config"])))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in LR.case_sd(fx, c).items()})
    return model


def tiny():
    from f5e_tts_amd.eval.whisper import Whisper, WhisperConfig
    fx = LR.load_fixture() if not _gold else _gold
    return Whisper(WhisperConfig.from_dicts(fx["config"], dict(fx["generation_config"])))


# ---- the noise ---------------------------------------------------------------------------------------------------------------------

KNOWN = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"))


def test_philox_known_answers():
    for counter, key, want in KNOWN:
        assert " ".join("%08x" % int(v) for v in S.philox4x32_10(counter, key)) == want
    # vectorised over the first counter word, as ``noise`` calls it
    w = S.philox4x32_10((np.array([0, 0x243f6a88], np.uint64), 0, 0, 0), (0, 0))
    assert ["%08x" % int(v[0]) for v in w] == KNOWN[0][2].split()


def test_uniform_lies_strictly_inside_the_unit_interval():
    lo, hi = float(S.uniform(0)), float(S.uniform(0xffffffff))
    assert lo == 2.0 ** -25 and hi == 1.0 - 2.0 ** -25 and 0.0 < lo < hi < 1.0
    g = S.gumbel(np.array([0, 0xff, 0x7fffffff, 0x80000000, 0xffffffff], np.uint64))
    assert np.isfinite(g).all() and g[0] == g[1] and (np.diff(g[1:]) > 0).all()
    assert abs(g[0] + np.log(25 * np.log(2.0))) < 1e-12 and abs(g[-1] - 17.328679) < 1e-5
    # the two branches of ``gumbel`` meet: -log(u) against -log1p(-(1 - u)) around u = 1 / 2
    for w in (0x7fffff00, 0x80000000):
        assert abs(float(S.gumbel(w)) + np.log(-np.log(float(S.uniform(w))))) < 1e-12
    # class i takes word i & 3 of block i >> 2
    n = S.noise(11, 7, 3, -2, 0x1_0000_0002)
    w = S.philox4x32_10((2, 7, 3, -2 & 0xffffffff), (2, 1))
    assert float(n[9]) == float(S.gumbel(w[1])) and float(n[10]) == float(S.gumbel(w[2]))


CHI_X = np.array([0.3, -0.5, 1.0, 0.1, -1.2, 0.8, -0.2, 0.5])


@pytest.mark.parametrize("T,stat", ((0.5, 1.5308374693699207), (1.0, 3.6337611771279192)))
def test_draws_follow_the_softmax(T, stat):
    """4096 row keys at V = 8, seed 0: Pearson's statistic against softmax(x / T).  The noise is deterministic, so it is a constant
    (recorded above); the 99.9 % quantile of chi-square with 7 degrees of freedom is 24.32.  Smallest expected count: 19.3."""
    p = np.exp(CHI_X / T - (CHI_X / T).max())
    p /= p.sum()
    cnt = np.zeros(8)
    for key in range(4096):
        cnt[S.sample_pick_ref([], CHI_X, 1, None, T, 0, 3, 2, key)[0]] += 1
    got = float(((cnt - 4096 * p) ** 2 / (4096 * p)).sum())
    print(f"T={T}: chi-square {got:.4f}")
    assert (4096 * p).min() > 5 and got < 24.32 and abs(got - stat) < 1e-9


def test_sampled_step_follows_the_rules():
    """The rules see the raw logits (rule 6 at T = 1), the draw the scaled ones; with nothing allowed the pick is 0."""
    g = np.random.default_rng(3)
    V, eos, no_ts = 162, 100, 110
    for hist in ([], [111], [111, 4, 120], [111, 4, 5]):
        for T in (0.2, 1.0):
            x = g.standard_normal(V) * 3.0
            ban, _ = LR.ts_mask(hist, x, eos, no_ts, 25, [1, 2])
            for key in range(40):
                pick, logp, _ = S.sample_pick_ref(hist, x, eos, no_ts, T, 9, 3 + len(hist), 0, key, 25, [1, 2])
                assert not ban[pick]
                ok = x[~ban]
                assert abs(logp - (x[pick] - ok.max() - np.log(np.exp(ok - ok.max()).sum()))) < 1e-12
    assert S.sample_pick_ref([], np.full(8, -np.inf), 1, 2, 1.0, 0, 2, 0, 0)[:2] == (0, 0.0)
    # far below every gap, the temperature turns the draw into the argmax of the allowed classes
    x = g.standard_normal(V) * 3.0
    assert S.sample_pick_ref([111, 4, 5], x, eos, no_ts, 1e-4, 9, 5, 0, 0, 25)[0] == LR.ts_pick_ref([111, 4, 5], x, eos, no_ts, 25)[0]


# ---- the restatement against the fixture -------------------------------------------------------------------------------------------

def test_fixture_shows_every_case():
    cs = {n: fb_case(n) for n in "abcdefgh"}
    assert cs["a"]["kept"] == [0.0] * len(cs["a"]["kept"]) and not any(a[3] or a[4] for w in cs["a"]["windows"] for a in w)
    b = cs["b"]["windows"][0]
    assert [a[0] for a in b] == cs["b"]["temperatures"][:2] and b[0][3] and not b[1][3] and b[0][0] == 0.0 and b[1][0] > 0
    assert cs["b"]["logprob_threshold"] is None and b[0][1] > cs["b"]["compression_ratio_threshold"] > b[1][1]
    c = cs["c"]["windows"][0]
    assert [a[0] for a in c] == cs["c"]["temperatures"] and all(a[3] for a in c) and cs["c"]["kept"] == [cs["c"]["temperatures"][-1]]
    d = cs["d"]["windows"][0]
    assert cs["d"]["compression_ratio_threshold"] is None and d[0][3] and d[0][2] < cs["d"]["logprob_threshold"] and len(d) == 2
    e = [a for w in cs["e"]["windows"] for a in w]
    assert any(a[4] and not a[3] and a[2] < cs["e"]["logprob_threshold"] for a in e)      # it would have fallen back: it is skipped
    assert len(cs["e"]["segments"]) > 0 and cs["e"]["no_speech_threshold"] is not None
    f = cs["f"]
    assert len(f["seeks"]) > 1 and f["kept"][0] == 0.0 and any(k > 0 for k in f["kept"][1:]) and f["row_key"] == 1
    g = cs["g"]
    assert g["num_beams"] == 2 and [a[0] for a in g["windows"][0]][0] == 0.0 and g["kept"][0] > 0 and len(g["seeks"]) == 1
    assert cs["h"]["temperature"] > 0 and len(cs["h"]["tokens"]) > 1
    for n in "abcdefg":
        c = cs[n]
        assert min(c["margins"]) >= 1e-2
        for a in (a for w in c["windows"] for a in w):
            assert c["compression_ratio_threshold"] is None or abs(a[1] - c["compression_ratio_threshold"]) >= 1e-2
            assert c["logprob_threshold"] is None or a[2] is None or abs(a[2] - c["logprob_threshold"]) >= 1e-2
    assert min(cs["h"]["margins"]) >= 1e-2


@pytest.mark.parametrize("name", tuple("abcdefg"))
def test_restatement_reproduces_the_fixture(name):
    fx, c = fb_gold(), fb_case(name)
    ref = R.Ref(LR.case_sd(fx, c), fx["config"])
    w = fx["wave_f32"][c["waves"][0][0]:c["waves"][0][1]]
    feats = R.log_mel(w, len(w), max(len(w) // 160, WINDOW), R.slaney_filters(80))
    segs, seeks, windows, gaps = S.transcribe_fallback_ref(
        ref, feats, fx["prompt"].tolist(), fx["generation_config"], CAP, WINDOW, fx["config"]["vocab_size"], c["temperatures"],
        c["compression_ratio_threshold"], c["logprob_threshold"], c["no_speech_threshold"], c["num_beams"], c["seed"], c["row_key"])
    assert [s["tokens"] for s in segs] == [s["tokens"] for s in c["segments"]] and seeks == c["seeks"]
    assert all(abs(s["start"] - q["start"]) < 1e-9 and abs(s["end"] - q["end"]) < 1e-9 for s, q in zip(segs, c["segments"]))
    assert [w_[-1][0] for w_ in windows] == c["kept"]
    err = 0.0
    for mine, theirs in zip(windows, c["windows"]):
        assert [(a[0], a[1], a[3], a[4]) for a in mine] == [(a[0], a[1], a[3], a[4]) for a in theirs]
        err = max([err] + [abs(a[2] - b[2]) for a, b in zip(mine, theirs) if b[2] is not None])
    kept = {s["seek"]: s["temperature"] for s in segs}
    assert all(kept[sk] == w_[-1][0] for sk, w_ in zip(seeks, windows) if sk in kept)
    print(f"case {name}: kept {c['kept']}, avg_logprob error {err:.2e}, margins {gaps}")
    assert err < 1e-5 and min(gaps) >= 1e-2


def test_restatement_reproduces_the_short_form_case():
    fx, c = fb_gold(), fb_case("h")
    ref = R.Ref(LR.case_sd(fx, c), fx["config"])
    w = fx["wave_f32"][c["waves"][0][0]:c["waves"][0][1]]
    enc = ref.encoder(R.log_mel(w, len(w), WINDOW, R.slaney_filters(80)))
    prompt = fx["prompt"].tolist() + [fx["generation_config"]["no_timestamps_token_id"]]
    full, total, _, gap = S.sampled_window_ref(ref, enc, prompt, fx["generation_config"], CAP, c["temperature"], c["seed"], 0, 0,
                                               timestamps=False)
    assert full == c["tokens"] and abs(total / len(full) - c["avg_logprob"]) < 1e-9 and gap >= 1e-2


def test_need_fallback_restatement_by_hand():
    assert S.need_fallback_ref(2.0, -0.5, 0.1, 1.5, None, None) == (True, False)
    assert S.need_fallback_ref(1.0, -0.5, 0.1, 1.5, -1.0, None) == (False, False)
    assert S.need_fallback_ref(1.0, -1.5, 0.1, None, -1.0, None) == (True, False)
    assert S.need_fallback_ref(2.0, -1.5, 0.9, 1.5, -1.0, 0.6) == (False, True)          # the skip wins
    assert S.need_fallback_ref(2.0, -1.5, 0.5, 1.5, -1.0, 0.6) == (True, False)
    assert S.need_fallback_ref(2.0, -0.5, 0.9, 1.5, -1.0, 0.6) == (True, False)          # likely enough: no skip


# ---- the caps of the GPU step tests hold for the oracle alone ------------------------------------------------------------------------

@pytest.mark.parametrize("V,R_", S.PICK_SHAPES)
def test_step_inputs_leave_no_undecided_draw(V, R_):
    """tests/test_whisper_fallback_gpu.py allows 1 % of a test's draws below tau; on these inputs the restatement has none, every
    rule state occurs and |x| <= 12 as ``pick_tau`` assumes."""
    eos, no_ts, sup, beg, mi = S.pick_layout(V)
    assert 0 <= eos <= no_ts < V - 1
    only_ts = set()
    for T in S.PICK_TEMPERATURES:
        draws = undecided = 0
        states = set()
        for hist, x, rk, se in S.pick_inputs(V, R_, T):
            assert np.abs(x).max() <= 12.0 and x.dtype == np.float32 and list(rk) != list(range(R_)) and (se > 0).all()
            tb = no_ts + 1
            states.add((len(hist) == 0, bool(hist) and hist[-1] >= tb, len(hist) < 2 or hist[-2] >= tb))
            for r in range(R_):
                full_sup = sup + (beg if not hist else [])
                pick, _, gap = S.sample_pick_ref(hist, x[r], eos, no_ts, T, S.PICK_SEED, 2 + len(hist), int(se[r]), int(rk[r]), mi, full_sup)
                ban = S.sample_mask(hist, x[r], eos, no_ts, mi, full_sup)
                assert not ban[pick] and (~ban).sum() >= 1
                if len(hist) == 3 and hist[-1] < tb:
                    only_ts.add(bool(ban[:tb].all()))
                draws += 1
                undecided += gap < S.pick_tau(T)
        assert len(states) == 4 and undecided == 0 and undecided <= 0.01 * draws
    assert V < 64 or only_ts                                                   # rule 6 was evaluated with text in play
    assert S.pick_tau(0.2) < 6e-5 and S.pick_tau(1.0) < 3e-5


# ---- refusals, before any launch -------------------------------------------------------------------------------------------------------

def test_fallback_record_and_its_refusals():
    from f5e_tts_amd import _C
    from f5e_tts_amd.eval.whisper import Fallback, Segment
    fb = Fallback()
    assert fb.temperatures == (0.0, 0.2, 0.4, 0.6, 0.8, 1.0) and fb.compression_ratio_threshold is None
    assert fb.logprob_threshold is None and fb.seed == 0
    assert Fallback([0, 0.5]).temperatures == (0.0, 0.5) and Fallback(0.0).temperatures == (0.0,)
    with pytest.raises(Exception, match="cannot assign"):
        fb.seed = 3
    for kw, word in ((dict(temperatures=()), "temperatures"), (dict(temperatures=(0.0, -0.2)), "temperatures"),
                     (dict(temperatures=(0.0, float("nan"))), "temperatures"), (dict(temperatures="warm"), "temperatures"),
                     (dict(compression_ratio_threshold="2"), "compression_ratio_threshold"),
                     (dict(logprob_threshold=float("inf")), "logprob_threshold"), (dict(seed=-1), "seed"), (dict(seed=1 << 64), "seed"),
                     (dict(seed=1.5), "seed")):
        with pytest.raises(_C.F5EError, match=f"Fallback: {word}"):
            Fallback(**kw)
    assert list(inspect.signature(Segment).parameters)[-1] == "temperature"
    assert Segment(0.0, 1.0, [1], 0, -1.0, 0.1, 1.0).temperature == 0.0


def test_transcribe_long_and_generate_refusals_by_name():
    from f5e_tts_amd import _C
    from f5e_tts_amd.eval.whisper import Fallback
    model = tiny()
    wav = torch.zeros(1, 16000)
    with pytest.raises(_C.F5EError, match="temperature = .* is out of scope .*fallback=Fallback"):
        model.transcribe_long(wav, temperature=(0.0, 0.2))                       # the loose keyword stays refused; the door is named
    with pytest.raises(_C.F5EError, match="compression_ratio_threshold = .* is out of scope"):
        model.transcribe_long(wav, compression_ratio_threshold=1.35)
    with pytest.raises(_C.F5EError, match="logprob_threshold = -1.0 and fallback.logprob_threshold = -0.5 are one threshold"):
        model.transcribe_long(wav, no_speech_threshold=0.6, logprob_threshold=-1.0, fallback=Fallback(logprob_threshold=-0.5))
    with pytest.raises(_C.F5EError, match="no_speech_threshold and logprob_threshold together"):
        model.transcribe_long(wav, no_speech_threshold=0.6, fallback=Fallback(compression_ratio_threshold=1.35))
    with pytest.raises(_C.F5EError, match="must be a Fallback or None"):
        model.transcribe_long(wav, fallback=(0.0, 0.2))
    with pytest.raises(_C.F5EError, match="row_keys has 2 entries for 1 recordings"):
        model.transcribe_long(wav, language="en", fallback=Fallback(), row_keys=[0, 1])
    for kw in (dict(no_speech_threshold=0.6, fallback=Fallback(logprob_threshold=-1.0)), dict(fallback=Fallback()),
               dict(no_speech_threshold=0.6, logprob_threshold=-1.0, fallback=Fallback(logprob_threshold=-1.0))):
        with pytest.raises(_C.F5EError, match="there is no CPU path"):        # accepted: the first launch is what stops a CPU run
            model.transcribe_long(wav, language="en", **kw)
    kv = [(torch.zeros(1, 50, 64), torch.zeros(1, 50, 64))]
    for call in (lambda **k: model.generate(wav, None, "en", **k), lambda **k: model.generate_from_kv(kv, [101, 102, 106, 110], **k)):
        with pytest.raises(_C.F5EError, match="beam-sample is not built"):
            call(temperature=0.4, beam_size=2)
        with pytest.raises(_C.F5EError, match="beam-sample is not built"):
            call(temperature=0.4, return_beams=True)
        for bad in (-0.1, float("nan"), float("inf"), "0.4", True):
            with pytest.raises(_C.F5EError, match="temperature = .* must be a finite number >= 0"):
                call(temperature=bad)
        with pytest.raises(_C.F5EError, match="seed = -1 must be an integer"):
            call(temperature=0.4, seed=-1)
    with pytest.raises(_C.F5EError, match="there is no CPU path"):
        model.generate(wav, None, "en", temperature=0.4, seed=5)


def test_op_refuses_cpu_tensors_and_bad_shapes():
    from f5e_tts_amd import _C, ops
    z = lambda *s: torch.zeros(*s, dtype=torch.int32)   # noqa: E731
    with pytest.raises(_C.F5EError, match="there is no CPU path"):
        ops.whisper_sample_pick(torch.zeros(2, 162), z(2, 8), z(2), z(2), z(1), torch.zeros(2), 2, 3, 100, 110, 0.5, 0, z(2), z(2))
    with pytest.raises(_C.F5EError, match="row_key \\[2\\], serial \\[2\\]"):
        ops.whisper_sample_pick(torch.zeros(2, 162), z(2, 8), z(2), z(2), z(1), torch.zeros(2), 2, 3, 100, 110, 0.5, 0, z(3), z(2))
    with pytest.raises(_C.F5EError, match="seed must lie in"):
        ops.whisper_sample_pick(torch.zeros(2, 162), z(2, 8), z(2), z(2), z(1), torch.zeros(2), 2, 3, 100, 110, 0.5, -1, z(2), z(2))
    with pytest.raises(_C.F5EError, match="V = 200 exceeds"):
        ops.whisper_sample_pick(torch.zeros(2, 162), z(2, 8), z(2), z(2), z(1), torch.zeros(2), 2, 3, 100, 110, 0.5, 0, z(2), z(2), V=200)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------

def test_abi_declares_binds_and_exports_the_entry():
    from f5e_tts_amd import _C, ops
    header = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    m = re.search(r"F5E_API int f5e_whisper_sample_pick\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == 24 == len(_C.SIGNATURES["f5e_whisper_sample_pick"])
    assert "float temperature" in m.group(1) and "unsigned long long seed" in m.group(1)
    assert "const int* row_key" in m.group(1) and "const int* serial" in m.group(1)
    emap = open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*f5e_\*;", emap)                              # the map exports the ABI by its prefix
    assert hasattr(_C.lib(), "f5e_whisper_sample_pick") and callable(ops.whisper_sample_pick)
    assert "#define F5E_ABI_VERSION 2 " in header and _C.ABI_VERSION == 2       # a function was only added
    assert len(_C.SIGNATURES["f5e_whisper_ts_pick"]) == 20                      # the entry it extends keeps its signature


def test_c_entry_refuses_bad_arguments_without_a_device():
    """Every check comes before the first launch: null operands, the limits of f5e_whisper_ts_pick and the temperature."""
    import ctypes as C
    from f5e_tts_amd import _C
    lib = _C.lib()
    buf, fbuf = (C.c_int * 64)(), (C.c_float * 64)()
    p, f = C.cast(buf, C.c_void_p), C.cast(fbuf, C.c_void_p)

    def pick(**o):
        a = dict(logits=f, ld=8, tokens=p, ld_tok=8, last=p, done=p, alive=p, sum_logp=f, R=1, V=8, p=2, n0=3, eos=2, no_ts=4, mi=-1,
                 T=0.5, seed=1, row_key=p, serial=p)
        a.update(o)
        return lib.f5e_whisper_sample_pick(None, a["logits"], a["ld"], None, 0, None, 0, a["tokens"], a["ld_tok"], a["last"],
                                           a["done"], a["alive"], a["sum_logp"], a["R"], a["V"], a["p"], a["n0"], a["eos"],
                                           a["no_ts"], a["mi"], a["T"], a["seed"], a["row_key"], a["serial"])
    for bad in (dict(logits=None), dict(sum_logp=None), dict(row_key=None), dict(serial=None), dict(V=1), dict(ld=7), dict(p=1),
                dict(ld_tok=3), dict(eos=8), dict(no_ts=7), dict(no_ts=1), dict(no_ts=-2), dict(mi=-2), dict(n0=0), dict(R=0),
                dict(T=0.0), dict(T=-1.0), dict(T=float("nan")), dict(T=float("inf")), dict(no_ts=-1, mi=-2)):
        assert pick(**bad) != 0, bad


# ---- wiring ------------------------------------------------------------------------------------------------------------------------------

def test_wiring_is_opt_in():
    from f5e_tts_amd.eval import eval_wer
    from f5e_tts_amd.eval.whisper import Fallback, Whisper, WhisperRecognizer
    base = ["--metalst", "m", "--gen_wav_dir", "g", "--lang", "en"]
    args = eval_wer.build_parser().parse_args(base)
    assert args.whisper_fallback is False and args.whisper_seed == 0
    args = eval_wer.build_parser().parse_args(base + ["--asr", "whisper", "--whisper_long", "--whisper_fallback", "--whisper_seed", "7"])
    assert args.whisper_fallback is True and args.whisper_seed == 7
    assert inspect.signature(WhisperRecognizer.__init__).parameters["fallback"].default is None
    ps = inspect.signature(Whisper.transcribe_long).parameters
    assert ps["fallback"].default is None and ps["row_keys"].default is None and ps["trace"].default is None
    for fn in (Whisper.generate, Whisper.generate_from_kv):
        ps = inspect.signature(fn).parameters
        assert ps["temperature"].default == 0.0 and ps["seed"].default == 0

    class Stub:
        def transcribe_long(self, audio, lens, language, **kw):
            self.kw = kw
            return [[]]
    rec = object.__new__(WhisperRecognizer)
    rec.device, rec.language, rec.model, rec._warned, rec.beam_size = torch.device("cpu"), "en", Stub(), set(), 1
    rec._audio = lambda audio, sr, cut=True: audio
    rec.transcribe_segments(torch.zeros(1, 10), 16000)
    assert rec.model.kw == dict(beam_size=1)                                   # a recogniser built without the record asks for nothing
    rec.fallback = Fallback(compression_ratio_threshold=1.35, logprob_threshold=-1.0, seed=7)
    rec.transcribe_segments(torch.zeros(1, 10), 16000)
    assert rec.model.kw == dict(beam_size=1, fallback=rec.fallback)
