"""Makes tests/golden/whisper_fallback.npz from ``transformers`` (5.15.0 when this was run): temperature fallback and sampling of the
long-form ``generate`` on the tiny model, wave and configs of tests/golden/whisper_long.npz (the helpers of
make_whisper_long_golden.py are imported; the weights are that fixture's and are not stored again -- only the rows of the tied
embedding that a case scales).  One utterance per call.

``torch.multinomial`` is replaced for the run by a Gumbel-argmax over log(probs) + g with the counter noise of
tests/whisper_sample_ref.py: g = -log(-log(u)), u from Philox4x32-10(counter = (class >> 2, step, serial, row_key), key = seed).
A wrapper around ``_sample`` keeps ``step`` (the position of the token fed, from the prompt's last one on) and ``serial`` (the
sampled decodes the recording has started before).  ``top_k=0`` switches off the top-50 warper that ``generate`` adds by default when
it samples: the draw is from the whole softmax over the allowed classes, as in the paper's and faster-whisper's fallback.

Cases (``temperatures`` and thresholds are per case; every threshold lies at least 1e-2 away from every compression ratio and
average log-probability that ``_need_fallback`` saw):
  a  no fallback needed                                   e  the no-speech skip wins over fallback (one temperature)
  b  fails on compression ratio at 0, passes at the 2nd   f  several windows, only a later one falls back (row_key 1)
  c  fails at every temperature, the last attempt kept    g  num_beams = 2 at temperature 0, then a sampled single row
  d  triggered by logprob_threshold alone                 h  short-form sampling without timestamps
Asserted per case, through the float64 restatement (which must reproduce tokens, segments, seeks, the temperatures tried per
window and the needs_fallback / should_skip flags): the greedy margins of the long-form fixture, and a top-1 / top-2 margin of
the perturbed values x / T + g of at least 1e-2 of the logits' RMS at every sampled step.  The seed is the first of ``SEEDS`` for
which every case is found.

    python tests/golden/make_whisper_fallback_golden.py
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_whisper_long_golden as G      # noqa: E402
import whisper_long_ref as LR             # noqa: E402
import whisper_ref as R                   # noqa: E402
import whisper_sample_ref as S            # noqa: E402

SEEDS = tuple(range(1, 41))
MARGIN = G.MARGIN
PROMPT = [G.SOT, G.EN, G.TRANSCRIBE]
SLICES = ([0, 16000], [16000, 32000], [38400, 54400], [3200, 19200], [8000, 24000], [24000, 40000])


class Noise:
    """Stands in for torch.multinomial while a model samples; ``wrap`` counts decodes and steps."""

    def __init__(self, seed, row_key, n0):
        self.seed, self.row_key, self.n0, self.serial, self.step = seed, row_key, n0, -1, 0

    def multinomial(self, probs, num_samples=1, **kw):
        assert num_samples == 1 and probs.shape[0] == 1
        g = S.noise(probs.shape[1], self.step, self.serial, self.row_key, self.seed)
        with np.errstate(divide="ignore"):
            y = np.log(probs[0].double().numpy()) + g
        self.step += 1
        return torch.tensor([[int(np.argmax(y))]])

    def wrap(self, model):
        orig = type(model)._sample                     # generate() looks the decoding method up on the class

        def sample(m, input_ids, logits_processor, stopping_criteria, generation_config, **kw):
            if generation_config.do_sample:
                self.serial += 1
                self.step = input_ids.shape[1] - 1
            return orig(m, input_ids, logits_processor, stopping_criteria, generation_config, **kw)
        type(model)._sample = sample
        return orig


def run_hf(model, fe, wave, temperatures, cr_thr, lp_thr, ns_thr, seed, row_key=0, num_beams=1):
    """-> dict(segments, seeks, windows = per window the attempts (temperature, compression ratio, average log-probability or
    None, needs_fallback, should_skip, no-speech probability or None))."""
    from transformers.generation.logits_process import WhisperNoSpeechDetection
    feats, mask, frames = G.features(fe, [wave])
    seeks, calls = [], []
    orig_need = model._need_fallback

    def spy(seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size, temperature):
        cr = float(model._retrieve_compression_ratio(seek_sequence, vocab_size))
        avg = None
        if isinstance(seek_outputs[index], dict) and "scores" in seek_outputs[index] and (num_beams == 1 or temperature > 0):
            avg = float(model._retrieve_avg_logprobs(seek_outputs[index]["scores"], seek_sequence, temperature))
        need, skip = orig_need(seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size, temperature)
        ns = [float(p.no_speech_prob[index]) for p in logits_processor if isinstance(p, WhisperNoSpeechDetection)]
        calls.append((len(seeks) - 1, float(temperature), cr, avg, bool(need), bool(skip), ns[0] if ns else None))   # report, then window
        return need, skip
    noise = Noise(seed, row_key, len(PROMPT))
    orig_sample, orig_multi = noise.wrap(model), torch.multinomial
    model._need_fallback, torch.multinomial = spy, noise.multinomial
    kw = dict(num_beams=num_beams) if num_beams > 1 else {}
    try:
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = model.generate(input_features=feats, attention_mask=mask, return_timestamps=True, return_segments=True,
                                 language="en", task="transcribe", condition_on_prev_tokens=False, temperature=tuple(temperatures), top_k=0,
                                 compression_ratio_threshold=cr_thr, logprob_threshold=lp_thr, no_speech_threshold=ns_thr,
                                 monitor_progress=lambda t: seeks.append(t[:, 0].tolist()), **kw)
    finally:
        model._need_fallback, type(model)._sample, torch.multinomial = orig_need, orig_sample, orig_multi
    segs = [dict(start=float(s["start"]), end=float(s["end"]), tokens=[int(t) for t in s["tokens"]]) for s in out["segments"][0]]
    T = frames[0]
    seeks = [s[0] for s in seeks if s[0] < T]
    windows = [[list(c[1:]) for c in calls if c[0] == w] for w in range(len(seeks))]
    return dict(segments=segs, seeks=seeks, windows=windows, frames=frames)


def ref_of(model):
    sd = {k: v.numpy() for k, v in model.state_dict().items() if k != "proj_out.weight"}
    return R.Ref(sd, G.hf_config().to_dict())


def check_with_ref(model, res, wave, temperatures, cr_thr, lp_thr, ns_thr, seed, row_key=0, K=1, far=True):
    """The float64 restatement must give the same segments, seeks, attempts and flags; thresholds lie MARGIN away from what was
    seen.  -> its margins [rule, greedy pick, sampled pick]."""
    gen = G.generation_config_dict()
    T = max(len(wave) // 160, G.WINDOW)
    feats = R.log_mel(wave, len(wave), T, R.slaney_filters(80))
    segs, seeks, windows, gaps = S.transcribe_fallback_ref(ref_of(model), feats, PROMPT, gen, G.MAX_TARGET, G.WINDOW, G.V, temperatures,
                                                           cr_thr, lp_thr, ns_thr, K, seed, row_key)
    assert seeks == res["seeks"], ("seeks", seeks, res["seeks"])
    assert [s["tokens"] for s in segs] == [s["tokens"] for s in res["segments"]], ("tokens", segs, res["segments"])
    assert all(abs(s["start"] - q["start"]) < 1e-9 and abs(s["end"] - q["end"]) < 1e-9 for s, q in zip(segs, res["segments"]))
    assert len(windows) == len(res["windows"]), ("windows", windows, res["windows"])
    for mine, theirs in zip(windows, res["windows"]):
        assert [(a[0], a[3], a[4]) for a in mine] == [(a[0], a[3], a[4]) for a in theirs], ("attempts", mine, theirs)
        for a, b in zip(mine, theirs):
            assert abs(a[1] - b[1]) < 1e-12 and (b[2] is None or abs(a[2] - b[2]) < 1e-3), ("figures", a, b)
            if far:
                assert cr_thr is None or abs(b[1] - cr_thr) >= MARGIN, ("cr near its threshold", b, cr_thr)
                assert lp_thr is None or b[2] is None or abs(b[2] - lp_thr) >= MARGIN, ("avg near its threshold", b, lp_thr)
    assert min(gaps) >= MARGIN, ("margins", gaps)
    res["kept"] = [w[-1][0] for w in res["windows"]]
    return gaps


def attempt(model, fe, wave, temperatures, cr_thr, lp_thr, ns_thr, seed, row_key=0, K=1):
    res = run_hf(model, fe, wave, temperatures, cr_thr, lp_thr, ns_thr, seed, row_key, K)
    gaps = check_with_ref(model, res, wave, temperatures, cr_thr, lp_thr, ns_thr, seed, row_key, K)
    return res, gaps


def probe(model, fe, wave, temperatures, seed, row_key=0, K=1):
    """Every temperature of the tuple on every window (thresholds that always fail, no margins asked): -> per window the attempts."""
    res = run_hf(model, fe, wave, temperatures, -1.0, None if K > 1 else -100.0, None, seed, row_key, K)
    return res["windows"]


def between(lo, hi):
    return 0.5 * (lo + hi) if hi - lo >= 2.5 * MARGIN else None


def find_cases(models, fe, wave, seed, e_case):
    found = {}

    def put(name, model_name, spec, temps, cr_thr, lp_thr, ns_thr, row_key=0, K=1, want=None):
        if name in found:
            return
        w = wave[spec[0]:spec[1]]
        try:
            res, gaps = attempt(models[model_name][1], fe, w, temps, cr_thr, lp_thr, ns_thr, seed, row_key, K)
            if want is not None:
                assert want(res), ("pattern", res["windows"])
        except AssertionError as e:
            print(f"    ({name}) {model_name} {spec} {temps}: rejected:", str(e)[:200])
            return
        print(f"    ({name}) {model_name} {spec} {temps} thresholds {cr_thr} {lp_thr} {ns_thr}: kept {res['kept']} margins {gaps}")
        found[name] = dict(name=name, row_scale=models[model_name][0], waves=[spec], temperatures=list(temps),
                           compression_ratio_threshold=cr_thr, logprob_threshold=lp_thr, no_speech_threshold=ns_thr,
                           row_key=row_key, num_beams=K, seed=seed, segments=res["segments"], seeks=res["seeks"],
                           windows=res["windows"], kept=res["kept"], frames=res["frames"], margins=gaps)

    # (e) the no-speech skip wins over fallback: the long-form fixture's case (e) -- its model, recording and thresholds, whose
    # greedy margins that fixture vetted -- with the logprob threshold now also the fallback's.  Every window misses it; the one
    # whose no-speech probability exceeds its threshold is skipped instead of falling back.  The tuple is (0.0,): a second
    # temperature moves the seek trajectory onto windows whose greedy picks miss the margin.
    put("e", "e", [0, G.S_LONG], (0.0,), None, e_case["logprob_threshold"], e_case["no_speech_threshold"],
        want=lambda r: any(a[4] and not a[3] for w_ in r["windows"] for a in w_) and any(a[3] for w_ in r["windows"] for a in w_)
        and len(r["segments"]) > 0 and all(abs(a[5] - e_case["no_speech_threshold"]) >= MARGIN for w_ in r["windows"] for a in w_))
    if "e" not in found:
        return found
    # (f) several windows: the first passes, a later one falls back (on its compression ratio, else on its log-probability)
    for mname in ("a", "b", "c"):
        for spec in ([0, G.S_LONG], [0, 32000], [16000, G.S_LONG], [9600, 41600], [16000, 48000]):
            if "f" in found:
                break
            base = probe(models[mname][1], fe, wave[spec[0]:spec[1]], (0.0,), seed, row_key=1)
            if len(base) < 2:
                continue
            crs, avgs = [w_[0][1] for w_ in base], [w_[0][2] for w_ in base]
            thr = []
            if between(crs[0], max(crs[1:])):
                thr.append((between(crs[0], max(crs[1:])), None))
            if between(min(avgs[1:]), avgs[0]):
                thr.append((None, between(min(avgs[1:]), avgs[0])))
            for cr_thr, lp_thr in thr:
                for t2 in (0.4, 0.8, 0.2, 1.0, 0.6):
                    put("f", mname, spec, (0.0, t2), cr_thr, lp_thr, None, row_key=1,
                        want=lambda r: len(r["kept"]) > 1 and r["kept"][0] == 0.0 and t2 in r["kept"][1:])
    if "f" not in found:
        return found
    for mname in ("c", "a", "b"):
        for spec in SLICES:
            w = wave[spec[0]:spec[1]]
            for t2 in (0.4, 0.8, 0.2, 1.0, 0.6):
                if all(k in found for k in "abcdg"):
                    break
                pr = probe(models[mname][1], fe, w, (0.0, t2, 1.0), seed)[0]
                crs, avgs = [a[1] for a in pr], [a[2] for a in pr]
                put("a", mname, spec, (0.0, t2), max(crs) + 0.1, min(avgs) - 0.5, None, want=lambda r: r["kept"] == [0.0])
                if crs[1] < crs[0] and between(crs[1], crs[0]):
                    put("b", mname, spec, (0.0, t2, 1.0), between(crs[1], crs[0]), None, None, want=lambda r: r["kept"] == [t2])
                put("c", mname, spec, (0.0, t2, 1.0), min(crs) - 0.05, None, None, want=lambda r: r["kept"] == [1.0])
                put("d", mname, spec, (0.0, t2), None, (avgs[1] > avgs[0] and between(avgs[0], avgs[1])) or max(avgs[:2]) + 0.25,
                    None, want=lambda r: r["kept"] == [t2])
                prg = probe(models[mname][1], fe, w, (0.0, t2), seed, K=2)[0]
                put("g", mname, spec, (0.0, t2), prg[0][1] - 0.05, None, None, K=2, want=lambda r: r["kept"] == [t2])
    return found


def short_form(model, fe, wave, T, seed):
    """(h) ``generate(return_timestamps=False, temperature=T)`` on one window: -> the generated tokens with the closing eos."""
    feats = torch.from_numpy(fe(wave, sampling_rate=16000, return_tensors="np").input_features)
    prompt = PROMPT + [G.NOTS]
    noise = Noise(seed, 0, len(prompt))
    orig_sample, orig_multi = noise.wrap(model), torch.multinomial
    torch.multinomial = noise.multinomial
    try:
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = model.generate(feats, language="en", task="transcribe", return_timestamps=False, temperature=T, top_k=0)
    finally:
        type(model)._sample, torch.multinomial = orig_sample, orig_multi
    ids = out[0].tolist()
    if ids[:len(prompt)] == prompt:
        ids = ids[len(prompt):]
    while len(ids) > 1 and ids[-1] == G.EOS and ids[-2] == G.EOS:
        ids.pop()
    gen = G.generation_config_dict()
    enc = ref_of(model).encoder(R.log_mel(wave, len(wave), G.WINDOW, R.slaney_filters(80)))
    full, total, _, gap = S.sampled_window_ref(ref_of(model), enc, prompt, gen, G.MAX_TARGET, T, seed, 0, 0, timestamps=False)
    seq = full[:-1] if full[-1] == G.EOS else full
    got = ids[:-1] if ids and ids[-1] == G.EOS else ids
    assert got == seq, ("short form", ids, full)
    assert gap >= MARGIN, ("short-form margin", gap)
    return full, total / len(full), gap


def main():
    from transformers import WhisperFeatureExtractor
    fe = WhisperFeatureExtractor(feature_size=80, chunk_length=1)
    long_fx = LR.load_fixture()
    wave = long_fx["wave_f32"]
    assert np.array_equal(np.round(G.make_wave() * 32768).astype(np.int16), long_fx["wave"])
    base = G.build_model(int(long_fx["seed"]))
    for k, v in base.state_dict().items():
        if k != "proj_out.weight":
            assert np.array_equal(G.bf16_bits(v), np.load(os.path.join(HERE, "whisper_long.npz"))["w/" + k]), k
    by_name = {c["name"]: c for c in long_fx["cases"]}
    models = {n: ([list(r) for r in by_name[n]["row_scale"]], G.scaled(base, by_name[n]["row_scale"])) for n in ("a", "b", "c", "e")}
    chosen = None
    for seed in SEEDS:
        print("seed", seed)
        found = find_cases(models, fe, wave, seed, by_name["e"])
        missing = [n for n in "abcdefg" if n not in found]
        if missing:
            print("  missing", missing)
            continue
        try:
            h = None
            for mname in ("a", "b", "c"):
                for spec in SLICES:
                    for T in (0.6, 1.0, 0.3):
                        try:
                            full, avg, gap = short_form(models[mname][1], fe, wave[spec[0]:spec[1]], T, seed)
                        except AssertionError as e:
                            print("    (h) rejected:", str(e)[:160])
                            continue
                        h = dict(name="h", row_scale=models[mname][0], waves=[spec], temperature=T, seed=seed, tokens=full,
                                 avg_logprob=avg, margins=[gap])
                        break
                    if h:
                        break
                if h:
                    break
            assert h, "no short-form case"
        except AssertionError as e:
            print("  rejected:", str(e)[:200])
            continue
        chosen = seed
        break
    assert chosen is not None, "no seed shows every case with its margins"
    cases = [found[n] for n in "abcdefg"] + [h]
    out = {"seed": np.int64(chosen), "cases_json": np.array(json.dumps(cases))}
    for c in cases:
        m = G.scaled(base, c["row_scale"])
        for lo, hi, fac in c["row_scale"]:
            out[f"rows_{c['name']}_{lo}"] = G.bf16_bits(m.model.decoder.embed_tokens.weight[lo:hi])
    path = os.path.join(HERE, "whisper_fallback.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", [(c["name"], c.get("kept")) for c in cases])
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
