"""Whisper's one-pass decoder prefill and prompt conditioning on the GPU (``Whisper.decoder_prefill``, ``decoder_logits(one_pass=
True)``, ``generate_from_kv(begin=, prefill=)``, ``transcribe_long(context=Context(...))``) against
  * the fixture made from ``transformers`` (tests/golden/whisper.npz): teacher-forced logits within the existing relative-L2 gate
    of 2e-4 (tests/test_whisper_gpu.py);
  * the cached single-position step, the yardstick of the prefill: cache slots bit for bit, logits within the same gate, and
    equal tokens for greedy, ruled, sampled and beam decoding wherever every decision of the run has the project's margin (top-1
    minus top-2 of at least 1e-2 of the logits' RMS, 50x the gate; asserted on the device's own teacher-forced logits);
  * a row's own B = 1 run for the rows of a left-padded ragged batch: tokens equal.  Bit for bit this does NOT hold in general
    for the logits: f5e_attn_prefill_f32 and the FROM step sum a padded row's keys in tiles that start at begin[r] rounded down
    to 16 (prefill) or at begin[r] itself (step), so the summation order of a padded row differs from its unpadded run; the
    test holds the logits to the 1e-5 row gate of tests/test_whisper_gpu.py instead and prints the figure.

Measured on an MI355X: one-pass logits against the fixture 3.8e-7 .. 5.3e-7 and against the cached step 3.1e-7 .. 3.3e-7; cache slots
of layer 0 bit-equal, of the later layers within 3.1e-7; ``no_speech_logp`` within 8.5e-8; a row padded by 15 against its unpadded
run 2.4e-7 (not bit-equal); ``avg_logprob`` / ``no_speech_prob`` of the fixture cases within 1.6e-6 relative."""
import numpy as np
import pytest
import torch

import whisper_long_ref as LR
import whisper_ref as R
import test_whisper_long_cpu as LC
from test_whisper_cpu import gold, tiny_model

pytestmark = pytest.mark.gpu

GATE, ROW_GATE, MARGIN = 2e-4, 1e-5, 1e-2
F32, I32 = torch.float32, torch.int32
_dev = {}


def model_gpu():
    if "model" not in _dev:
        _dev["model"] = tiny_model().cuda()
    return _dev["model"]


def kv_gpu(n):
    if n not in _dev:
        wav = torch.from_numpy(gold()["wave_f32"][:n].copy()).cuda()[None]
        _dev[n] = model_gpu().encode(wav)
    return _dev[n]


def long_gpu():
    """The long-form fixture's tiny model (it has timestamp classes, <|startofprev|> = 108 and 40 target positions) with the
    cross keys / values of the first window of its case (a)."""
    if "long" not in _dev:
        model = LC.tiny_model("a").cuda()
        wav = torch.from_numpy(LC.case_wave(LC.case("a"))[:160 * model.n_frames].copy()).cuda()[None]
        _dev["long"] = (model, model.encode(wav))
    return _dev["long"]


def rows_of(kv, idx):
    return [(k[idx].contiguous(), v[idx].contiguous()) for k, v in kv]


def long_prompt(seed, n_prev):
    """``n_prev`` made-up text ids in front of the fixture's forced tokens: what a conditioned window starts with."""
    fx = gold()
    g = np.random.default_rng(seed)
    return [int(t) for t in g.integers(1, 100, n_prev)] + [int(t) for t in fx["prompt"]]


def clear_margin(model, kv, tokens, n, n0, begin=None):
    """Every greedy decision of row 0 of ``tokens`` (positions n0 - 1 .. n - 2) has top-1 - top-2 >= MARGIN x RMS, on the
    device's own teacher-forced logits through the cached step."""
    ids = tokens[:1, :n - 1] if begin is None else tokens[:1, begin:n - 1]
    lg = model.decoder_logits([(k[:1], v[:1]) for k, v in kv], ids.contiguous())[0].double()
    lg = lg[n0 - 1 - (begin or 0):]
    top = lg.topk(2, -1).values
    return float(((top[:, 0] - top[:, 1]) / lg.pow(2).mean(-1).sqrt()).min())


@pytest.mark.parametrize("n", (14400, 40000, 48000))
def test_one_pass_logits_against_the_fixture_and_the_cached_step(n):
    fx, model = gold(), model_gpu()
    ids = torch.from_numpy(fx[f"tokens_{n}"][:12].copy()).cuda()[None]
    one = model.decoder_logits(kv_gpu(n), ids, one_pass=True)
    loop = model.decoder_logits(kv_gpu(n), ids)
    e_fx, e_loop = R.rel_l2(one[0].cpu().numpy(), fx[f"logits_{n}"]), R.rel_l2(one[0].cpu().numpy(), loop[0].cpu().numpy())
    print(f"n={n}: one-pass logits vs fixture {e_fx:.2e}, vs the cached step {e_loop:.2e} (gate {GATE:g})")
    assert one.shape == loop.shape and torch.isfinite(one).all()
    assert e_fx < GATE and e_loop < GATE


@pytest.mark.parametrize("R_", (1, 2))
def test_prefill_leaves_the_caches_of_single_steps(R_):
    """K and V of slots 0 .. U0 - 1 are bit-equal in layer 0 (the same embedding rows through the same LayerNorm and GEMM rows);
    in later layers the inputs differ by the attention's summation order, so they are held to the gate.  The wanted logits
    equal the steps' within the gate, and only slots 0 .. U0 - 1 are written."""
    fx, model = gold(), model_gpu()
    n, U0 = 40000, 11
    kv = rows_of(kv_gpu(n), [0] * R_)
    ids = torch.from_numpy(fx[f"tokens_{n}"][:U0].copy()).cuda()[None].repeat(R_, 1).to(I32)
    a, b = model._dec_state(R_, U0 + 2, ids.device), model._dec_state(R_, U0 + 2, ids.device)
    for st in (a, b):
        for kc, vc in st["caches"]:
            kc.fill_(-7.0), vc.fill_(-7.0)
    got = model.decoder_prefill(a, kv, ids, want=(0, U0 - 1))
    steps = [model._dec_step(b, kv, ids[:, p].contiguous(), p, True).clone() for p in range(U0)]
    worst = 0.0
    for i, ((ka, va), (kb, vb)) in enumerate(zip(a["caches"], b["caches"])):
        assert bool((ka[:, U0:] == -7.0).all()) and bool((va[:, U0:] == -7.0).all()), "slots beyond the prompt were written"
        if i == 0:
            assert torch.equal(ka, kb) and torch.equal(va, vb), "layer 0: K / V slots must be bit-equal"
        worst = max(worst, R.rel_l2(ka[:, :U0].cpu().numpy(), kb[:, :U0].cpu().numpy()),
                    R.rel_l2(va[:, :U0].cpu().numpy(), vb[:, :U0].cpu().numpy()))
    e0, e1 = R.rel_l2(got[:, 0].cpu().numpy(), steps[0].cpu().numpy()), R.rel_l2(got[:, 1].cpu().numpy(), steps[-1].cpu().numpy())
    print(f"R={R_}: caches of layers >= 1 within {worst:.2e}, logits of position 0 {e0:.2e}, of position {U0 - 1} {e1:.2e}")
    assert worst < GATE and e0 < GATE and e1 < GATE


def clear_prompt(model, kv, forced, n_prev):
    """The first seeded prompt of ``n_prev`` made-up text ids + ``forced`` whose plain greedy run has the margin at every step
    (a condition on the inputs, measured through the cached step)."""
    for seed in range(50):
        g = np.random.default_rng(seed)
        prompt = [int(t) for t in g.integers(10, 60, n_prev)] + forced
        tokens, n = model.generate_from_kv(kv, prompt, max_new_tokens=12)
        if int(n[0]) > len(prompt) + 2 and clear_margin(model, kv, tokens, int(n[0]), len(prompt)) >= MARGIN:
            return prompt
    raise AssertionError("no seeded prompt has the margin at every greedy step")


@pytest.mark.parametrize("sync_every", (1, 8))
@pytest.mark.parametrize("mode", ("greedy", "beam", "ruled", "sampled", "beam_ruled"))
def test_a_continuation_after_the_prefill_equals_the_stepped_one(mode, sync_every):
    """Greedy: on a prompt whose every step has the margin.  The ruled, sampled and beam runs reuse the pick kernels unchanged on
    logits that differ from the stepped ones by the figure of test_prefill_leaves_the_caches_of_single_steps (1e-6 of their
    scale), so a fixed seeded prompt is compared outright."""
    ts = mode in ("ruled", "beam_ruled", "sampled")
    if ts:
        model, kv = long_gpu()
        prompt = [108] + [int(t) for t in np.random.default_rng(1).integers(10, 60, 9)] + [101, 102, 106]
    else:
        model, kv = model_gpu(), kv_gpu(40000)
        prompt = clear_prompt(model, kv, [int(t) for t in gold()["prompt"]], 9)
    kw = dict(sync_every=sync_every, return_timestamps=ts, max_new_tokens=16)
    if mode.startswith("beam"):
        kw["beam_size"] = 3
    if mode == "sampled":
        kw.update(temperature=0.4, seed=5)
    sa, sb = {}, {}
    want, n_w = model.generate_from_kv(kv, prompt, stats=sa if ts else None, begin=[0] if ts else None, **kw)[:2]
    got, n_g = model.generate_from_kv(kv, prompt, stats=sb if ts else None, prefill=True, **kw)[:2]
    n = int(n_w[0])
    print(f"{mode} sync_every={sync_every}: {n} tokens {want[0, len(prompt):n].tolist()}")
    assert torch.equal(got, want) and torch.equal(n_g, n_w)
    assert n > len(prompt) + 2, "the run must pick something"
    for key in ("sum_logp", "no_speech_logp") if ts else ():
        e = float((sa[key] - sb[key]).abs().max() / sa[key].abs().max().clamp(min=1e-30))
        print(f"  {key}: {e:.2e}")
        assert e < GATE, key


def test_no_speech_logp_is_read_at_startoftranscript():
    """A long prompt moves <|startoftranscript|> to n0 - 3, and both paths must read the probability there: equal to the
    teacher-forced logits of that position."""
    from f5e_tts_amd import ops
    model, kv = long_gpu()
    prompt = [108] + [int(t) for t in np.random.default_rng(2).integers(10, 60, 9)] + [101, 102, 106]
    sot = len(prompt) - 3
    lg = model.decoder_logits(kv, torch.tensor([prompt], dtype=I32).cuda())[:, sot]
    want = ops.token_logp(lg.contiguous(), torch.tensor([model.cfg.no_speech_token_id], dtype=I32).cuda())
    for prefill in (False, True):
        st = {}
        model.generate_from_kv(kv, prompt, max_new_tokens=2, return_timestamps=True, stats=st, prefill=prefill,
                               begin=None if prefill else [0])
        e = float((st["no_speech_logp"] - want).abs() / want.abs())
        print(f"prefill={prefill}: no_speech_logp {float(st['no_speech_logp']):.6f} vs {float(want):.6f} ({e:.2e})")
        assert e < GATE


@pytest.mark.parametrize("prefill", (False, True))
@pytest.mark.parametrize("beam", (1, 3))
def test_rows_of_a_left_padded_batch_equal_their_own_runs(prefill, beam):
    """Tokens equal (the logits of a padded row are not bit-equal to its own run: see the module docstring)."""
    fx, model = gold(), model_gpu()
    forced = [int(t) for t in fx["prompt"]]
    kvs = [kv_gpu(40000), kv_gpu(14400)]
    kv2 = [(torch.cat((a[0], b[0])), torch.cat((a[1], b[1]))) for a, b in zip(*kvs)]
    prompts = [clear_prompt(model, kvs[0], forced, 17), clear_prompt(model, kvs[1], forced, 2)]
    n0 = max(len(p) for p in prompts)
    begin = [n0 - len(p) for p in prompts]
    assert begin == [0, 15]
    padded = [[model.cfg.eos_token_id] * b + p for b, p in zip(begin, prompts)]
    tokens, n = model.generate_from_kv(kv2, padded, max_new_tokens=12, beam_size=beam, begin=begin, prefill=prefill)[:2]
    for r in range(2):
        one, n1 = model.generate_from_kv(kvs[r], prompts[r], max_new_tokens=12, beam_size=beam)[:2]
        n1 = int(n1[0])
        assert tokens[r, begin[r]:int(n[r])].tolist() == one[0, :n1].tolist(), f"row {r}"
        assert int(n[r]) - begin[r] == n1


def test_padded_row_logits_against_the_unpadded_row():
    """The figure behind "token equality, not bit equality": row 1 of the padded batch, teacher-forced, against its own run."""
    fx, model = gold(), model_gpu()
    kv = kv_gpu(14400)
    row = long_prompt(7, 3) + [int(t) for t in fx["tokens_14400"][4:10]]
    pad = 15
    ids = torch.tensor([[model.cfg.eos_token_id] * pad + row], dtype=I32).cuda()
    st = model._dec_state(1, ids.shape[1], ids.device)
    got = model.decoder_prefill(st, kv, ids, torch.tensor([pad], dtype=I32).cuda(), want=range(pad, ids.shape[1]))
    want = model.decoder_logits(kv, torch.tensor([row], dtype=I32).cuda(), one_pass=True)
    e = R.rel_l2(got[0].cpu().numpy(), want[0].cpu().numpy())
    print(f"padded by {pad}: logits vs the unpadded row {e:.2e} (bit-equal: {torch.equal(got, want)})")
    assert e < ROW_GATE


def test_refusals_before_any_launch():
    from f5e_tts_amd._C import F5EError
    fx, model = gold(), model_gpu()
    kv = kv_gpu(14400)
    prompt = [int(t) for t in fx["prompt"]]
    st = model._dec_state(1, 8, kv[0][0].device)
    with pytest.raises(F5EError, match="decoder_prefill"):
        model.decoder_prefill(st, kv, [[1, 2, model.cfg.vocab_size]])              # an id outside the table, known to the host
    with pytest.raises(F5EError, match="decoder_prefill"):
        model.decoder_prefill(st, kv, [list(range(9))])                             # more tokens than the state caches
    with pytest.raises(F5EError, match="decoder_prefill"):
        model.decoder_prefill(st, kv, [[1, 2, 3]], want=(3,))                       # a wanted position outside the prompt
    with pytest.raises(F5EError, match="begin"):
        model.generate_from_kv(kv, prompt, begin=[len(prompt)])                     # a row that is all padding
    with pytest.raises(F5EError, match="begin"):
        model.generate_from_kv(kv, prompt, begin=[0, 0])                            # two pad counts for one row
    with pytest.raises(F5EError, match="startoftranscript"):
        model.generate_from_kv(kv, [1, 2, 3], prefill=True, stats={})               # nowhere to read the no-speech probability


# ---- the fixture made from transformers (tests/golden/whisper_prompt.npz) ----------------------------------------------------------

import test_whisper_prompt_cpu as PC   # noqa: E402


def case_model(c):
    key = ("case", tuple(tuple(r) for r in c["row_scale"]))
    if key not in _dev:
        _dev[key] = PC.tiny_model(c).cuda()
    return _dev[key]


def run_case(c, rows, sync_every=8, context="case"):
    """``transcribe_long`` on rows of a case (one call, a ragged batch when there are two) -> (segments per row, trace)."""
    fx = PC.gold()
    waves = [fx["wave_f32"][c["waves"][b][0]:c["waves"][b][1]] for b in rows]
    S = max(len(w) for w in waves)
    batch = torch.full((len(rows), S), 1e4, dtype=F32)                         # garbage beyond a row's length
    for i, w in enumerate(waves):
        batch[i, :len(w)] = torch.from_numpy(w.copy())
    trace = []
    kw = {}
    if c.get("fallback") is not None:
        from f5e_tts_amd.eval.whisper import Fallback
        fb = c["fallback"]
        kw["fallback"] = Fallback(tuple(fb["temperatures"]), fb["compression_ratio_threshold"], fb["logprob_threshold"], fb["seed"])
        kw["row_keys"] = [fb["row_key"]] * len(rows)
    if c.get("no_speech_threshold") is not None:
        kw = dict(no_speech_threshold=c["no_speech_threshold"], logprob_threshold=c["logprob_threshold"])
    out = case_model(c).transcribe_long(batch.cuda(), [len(w) for w in waves], "en", beam_size=c["num_beams"], sync_every=sync_every,
                                        trace=trace, context=PC.context_of(c) if context == "case" else context, **kw)
    return out, trace


def check_row_against_the_fixture(c, b, segs, trace, row):
    want, T = c["segments"][b], c["frames"][b]
    assert [s.tokens for s in segs] == [s["tokens"] for s in want], (c["name"], b)
    assert all(abs(s.start_s - q["start"]) < 1e-9 and abs(s.end_s - q["end"]) < 1e-9 for s, q in zip(segs, want))
    mine = [t for t in trace if t["row"] == row]
    assert [t["seek"] for t in mine] == [s for s in c["seeks"][b] if s < T]
    assert [t["prompt"] for t in mine] == c["prompts"][b]
    assert [t["should_skip"] for t in mine] == [k == "k" for k in c["kinds"][b]]
    assert all(t["temperature"] == 0.0 and not t["needs_fallback"] for t in mine) and all(s.temperature == 0.0 for s in segs)
    worst = 0.0
    if c["num_beams"] == 1:
        for t, (avg, ns) in zip(mine, c["windows"][b]):
            worst = max(worst, abs(t["avg_logprob"] - avg) / abs(avg), abs(t["no_speech_prob"] - ns) / ns)
        assert worst < GATE, (c["name"], b, worst)
    return worst


@pytest.mark.parametrize("sync_every", (1, 8))
@pytest.mark.parametrize("name", "abcdefhi")
def test_fixture_cases(name, sync_every):
    c = PC.case(name)
    for b in PC.rows_of(c):
        out, trace = run_case(c, [b], sync_every)
        worst = check_row_against_the_fixture(c, b, out[0], trace, 0)
        print(f"({name}) row {b} sync_every={sync_every}: {len(out[0])} segments, {len(trace)} windows, avg_logprob / no_speech_prob "
              f"within {worst:.2e}")


@pytest.mark.parametrize("sync_every", (1, 8))
def test_fixture_case_g_a_window_kept_at_a_high_temperature_does_not_condition_the_next(sync_every):
    """Conditioning under ``Fallback(temperatures=(0.0, 0.8))``: the attempts (window, temperature, compression ratio) and their
    needs_fallback flags, the temperature kept per window, every window's decoder input (the one after the window kept at 0.8 is
    the forced tokens alone), tokens, boundaries and seeks equal ``transformers``'."""
    c = PC.case("g")
    out, trace = run_case(c, [0], sync_every)
    want, seeks, thr = c["segments"][0], c["seeks"][0], c["fallback"]["compression_ratio_threshold"]
    assert [s.tokens for s in out[0]] == [s["tokens"] for s in want]
    assert all(abs(s.start_s - q["start"]) < 1e-9 and abs(s.end_s - q["end"]) < 1e-9 for s, q in zip(out[0], want))
    assert [(t["seek"], t["temperature"]) for t in trace] == [(seeks[w], temp) for w, temp, _ in c["attempts"]]
    assert all(abs(t["compression_ratio"] - cr) < 1e-12 for t, (_, _, cr) in zip(trace, c["attempts"]))
    assert [t["needs_fallback"] for t in trace] == [cr > thr for _, _, cr in c["attempts"]]
    kept = {t["seek"]: (t["temperature"], t["prompt"]) for t in trace}                 # the last attempt of every window
    assert [kept[s][0] for s in seeks] == c["kept"][0] and [kept[s][1] for s in seeks] == c["prompts"][0]
    assert all(s.temperature == kept[s.seek][0] for s in out[0])
    print(f"(g) sync_every={sync_every}: kept {c['kept'][0]}, decoder inputs of {[len(p) for p in c['prompts'][0]]} tokens")


@pytest.mark.parametrize("name", ("e", "i"))
def test_rows_of_the_ragged_cases_equal_their_own_runs(name):
    """Cases (e) and (i) as ONE batch each.  (e): in some iteration both rows are conditioned on previous texts of different
    lengths (the left-pad path).  (i): in some iteration the row with the shorter decoder input, the padded one, picks more
    tokens than the batch's bound leaves it (that bound counts the pad columns); its own bound is ``max_target_positions`` from
    its first token, so it is decoded again alone (``at_bound``), and without that it would lose the picks beyond.  Tokens,
    boundaries, seeks and prompts equal the rows' B = 1 runs of ``transformers``; the figures within the gate (not bit for bit:
    see the module docstring)."""
    c = PC.case(name)
    out, trace = run_case(c, [0, 1])
    for b in range(2):
        check_row_against_the_fixture(c, b, out[b], trace, b)
        alone, _ = run_case(c, [b])
        assert [(s.tokens, s.start_s, s.end_s, s.seek) for s in alone[0]] == [(s.tokens, s.start_s, s.end_s, s.seek) for s in out[b]]
        for s, q in zip(alone[0], out[b]):
            assert abs(s.avg_logprob - q.avg_logprob) < GATE * abs(s.avg_logprob)


@pytest.mark.parametrize("name", "abcdefgh")
def test_no_context_reproduces_the_long_form_fixture(name):
    """``context=None`` takes the launches it always took (dataclass equality with a call that does not name the argument), and
    ``Context()`` -- nothing to condition on, no prompt, but the prefill and the left-pad path -- gives the same tokens, boundaries
    and seeks as tests/golden/whisper_long.npz records."""
    from f5e_tts_amd.eval.whisper import Context
    c = LC.case(name)
    key = ("long", name)
    if key not in _dev:
        _dev[key] = LC.tiny_model(name).cuda()
    model = _dev[key]
    kw = dict(beam_size=c.get("num_beams", 1))
    if "no_speech_threshold" in c:
        kw.update(no_speech_threshold=c["no_speech_threshold"], logprob_threshold=c["logprob_threshold"])
    for b in range(len(c["waves"])):
        w = torch.from_numpy(LC.case_wave(c, b).copy()).cuda()[None]
        plain = model.transcribe_long(w, language="en", **kw)[0]
        assert model.transcribe_long(w, language="en", context=None, **kw)[0] == plain            # every float bit for bit
        ctx = model.transcribe_long(w, language="en", context=Context(), **kw)[0]
        assert [s.tokens for s in plain] == [s["tokens"] for s in c["segments"][b]]
        assert [(s.tokens, s.start_s, s.end_s, s.seek) for s in ctx] == [(s.tokens, s.start_s, s.end_s, s.seek) for s in plain]
        for s, q in zip(ctx, plain):
            assert abs(s.no_speech_prob - q.no_speech_prob) <= GATE * q.no_speech_prob
            assert kw["beam_size"] > 1 or abs(s.avg_logprob - q.avg_logprob) <= GATE * abs(q.avg_logprob)


def test_recognizer_with_a_text_prompt_from_a_checkpoint_directory(tmp_path):
    """``eval_wer --whisper_long --whisper_prompt TEXT [--whisper_condition]`` builds exactly this: vocab.json and merges.txt turn
    the text into case (b)'s prompt ids, and the recogniser reproduces that case; with conditioning it equals the direct call."""
    import json
    from f5e_tts_amd.eval.whisper import Context, WhisperRecognizer
    from test_whisper_cpu import write_safetensors
    fx, c = PC.gold(), PC.case("b")
    ids = c["context"]["prompt_ids"]
    assert len(ids) == 3 and ids[0] == 108
    d = tmp_path / "ckpt"
    d.mkdir()
    vocab = {f"w{i}": i for i in range(100)}
    del vocab[f"w{ids[1]}"], vocab[f"w{ids[2]}"]
    vocab["Ġhello"], vocab["Ġworld"] = ids[1], ids[2]
    (d / "config.json").write_text(json.dumps(fx["config"]))
    (d / "generation_config.json").write_text(json.dumps(fx["generation_config"]))
    (d / "vocab.json").write_text(json.dumps(vocab))
    (d / "added_tokens.json").write_text(json.dumps({f"<|s{i}|>": i for i in range(100, 162)}))
    (d / "merges.txt").write_text("#version: 0.2\nĠ h\nĠh e\nĠhe l\nĠhel l\nĠhell o\nĠ w\nĠw o\nĠwo r\nĠwor l\nĠworl d\n", encoding="utf-8")
    write_safetensors(str(d / "model.safetensors"), {k: (v, "F32") for k, v in LR.case_sd(fx, c).items()})
    lo, hi = c["waves"][0]
    wave = torch.from_numpy(fx["wave_f32"][lo:hi].copy())
    rec = WhisperRecognizer(str(d), "cuda", "en", long_form=True, initial_prompt=" hello world ")
    assert rec.context == Context(False, tuple(ids), "first-segment")
    segs = rec.transcribe_segments(wave, 16000)
    want = c["segments"][0]
    assert len(segs) == len(want)
    assert all(abs(s[0] - q["start"]) < 1e-9 and abs(s[1] - q["end"]) < 1e-9 for s, q in zip(segs, want))
    assert [s[2] for s in segs] == [rec.model.decode_ids(q["tokens"]) for q in want]
    both = WhisperRecognizer(str(d), "cuda", "en", long_form=True, initial_prompt="hello world", condition_on_previous_text=True)
    direct = both.model.transcribe_long(wave[None].cuda(), None, "en", context=Context(True, tuple(ids)))[0]
    assert [(s[0], s[1]) for s in both.transcribe_segments(wave, 16000)] == [(s.start_s, s.end_s) for s in direct]
    assert direct and [s.tokens for s in direct] != [q["tokens"] for q in want]           # conditioning changes the transcript
