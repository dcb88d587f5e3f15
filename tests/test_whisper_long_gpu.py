"""Whisper's timestamp rules and long-form loop on the GPU (f5e_whisper_ts_pick, f5e_whisper_ts_rule, f5e_whisper_beam_step_ts in
csrc/whisper.hip; ``generate(return_timestamps=True)``, ``transcribe_long`` and ``detect_language`` in eval/whisper.py) against
  * the float64 restatement tests/whisper_long_ref.py on crafted (history, logits) pairs, one per rule branch plus random rows: the
    pick and the mask exact, guard bands and the logits untouched;
  * the fixture made from ``transformers`` (tests/golden/whisper_long.npz): tokens, segment boundaries, seek trajectories and
    detected languages equal, with ``sync_every`` 1 and 8; the rows of the ragged batch equal their own B = 1 runs bit for bit.

Bounds.  ``sum_logp`` (the log-probability of a pick among the allowed classes): the error against the float64 restatement is held
to 4 x the error that a NumPy float32 evaluation of the same formula, (x[pick] - M) - log(sum exp(x - M)), shows on the same inputs
(that figure is floored at one float32 spacing of the value and at 2^-23: the sum S >= 1 is held to a relative 2^-23 in float32 and
d log S = dS / S, so a NumPy run that happens to round its S exactly does not set a bound below the format's own), the method of
the log-mel test.  ``avg_logprob`` / ``no_speech_prob`` of the fixture
cases: the project's relative-L2 gate for teacher-forced logits, 2e-4 (tests/test_whisper_gpu.py).

Measured on an MI355X: see DESIGN.md 4o."""
import numpy as np
import pytest
import torch

import whisper_beam_ref as BR
import whisper_long_ref as LR
from test_whisper_long_cpu import case, case_wave, gold, tiny_model, windows_of

pytestmark = pytest.mark.gpu

GATE = 2e-4
F32, I32 = torch.float32, torch.int32
_dev = {}


def model_gpu(name):
    rs = tuple(tuple(r) for r in case(name)["row_scale"])
    if rs not in _dev:
        _dev[rs] = tiny_model(name).cuda()
    return _dev[rs]


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---- the ruled pick and the rule pre-pass on crafted rows ------------------------------------------------------------------------

def crafted(V, Rr, seed, ties=True):
    """-> (logits f32 [Rr, V], histories, eos, no_ts, suppress).  Row r cycles through the rule branches; the timestamp block
    is shifted per row so that both outcomes of the lse / max comparison occur."""
    g = np.random.default_rng(seed)
    n_ts = 51 if V <= 1000 else 1501
    no_ts = V - n_ts - 1
    tb, eos = no_ts + 1, no_ts - 10
    x = (g.standard_normal((Rr, V)) * 3.0).astype(np.float32)
    hists = [[], [tb + 3], [tb + 3, tb + 3], [17, tb + 9], [tb, 17], [tb, 17, tb + 7, tb + 7, 21], [11, tb + n_ts - 1], [tb + 2, 30, 31]]
    hists = [hists[r % len(hists)] for r in range(Rr)]
    for r in range(Rr):
        x[r, tb:] += (-6.0, 2.0, 0.0)[r % 3] - np.log(n_ts / 51.0)
    if Rr > 4 and ties:
        x[2, [3, tb + 20, eos]] = -np.inf                                    # -inf present
        x[3, tb + 12] = x[3, tb + 30] = 40.0                                 # a tie among the timestamps: the lower index
        x[3, eos] = 40.0                                                     # ... and with the text class that stays allowed
        x[4, 20] = x[4, 40] = 45.0                                           # a tie among the text classes
    sup = [2, 3, -1, V + 5, eos + 1, tb + 5]
    return x, hists, eos, no_ts, sup


@pytest.mark.parametrize("V,ld,Rr", ((160, 160, 1), (160, 160, 5), (163, 163, 5), (51866, 51868, 1), (51866, 51868, 5)))
@pytest.mark.parametrize("max_initial", (None, 25))
def test_ts_pick_and_rule_exact(V, ld, Rr, max_initial):
    from f5e_tts_amd import ops
    x, hists, eos, no_ts, sup = crafted(V, Rr, V + Rr)
    n0, L = 3, 5
    p = n0 + L - 1
    wide = torch.full((Rr, ld), 1e9)
    wide[:, :V] = torch.from_numpy(x)
    dl = wide.cuda()
    view = dl[:, :V] if ld > V else dl
    sup_t = torch.tensor(sup, dtype=I32).cuda()
    beg_t = torch.tensor([4, eos], dtype=I32).cuda()
    worst, worst32 = 0.0, 0.0
    # every row is given its history as the LAST tokens before p + 1 (n0 moves with the history's length): one launch per length
    for n_h in sorted({len(h) for h in hists}):
        rows = [r for r in range(Rr) if len(hists[r]) == n_h]
        n0_h = p + 1 - n_h
        tokens = torch.full((Rr, p + 4), -5, dtype=I32)
        for r in range(Rr):
            tokens[r, n0_h:p + 1] = torch.tensor(hists[r][:n_h] if len(hists[r]) >= n_h else [1] * n_h, dtype=I32)
        tok_d = tokens.cuda()
        before = tok_d.clone()
        done0 = [1 if (r == Rr - 1 and Rr > 1 and max_initial is not None) else 0 for r in range(Rr)]
        last, alive = torch.full((Rr,), -5, dtype=I32).cuda(), torch.full((3,), -5, dtype=I32).cuda()
        done, slp = torch.tensor(done0, dtype=I32).cuda(), torch.full((Rr + 2,), 0.5, dtype=F32).cuda()
        slp[1:Rr + 1] = 0.0                                                   # the rows' own cells: the sum starts at 0
        desc = torch.full((Rr + 2, 4), -7, dtype=I32).cuda()
        first = n_h == 0
        ops.whisper_ts_rule(view, tok_d, p, n0_h, eos, no_ts, V=V, suppress=sup_t, begin_suppress=beg_t, max_initial=max_initial,
                            out=desc[1:Rr + 1])
        assert torch.equal(tok_d, before)
        ops.whisper_ts_pick(view, tok_d, last, done, alive[1:2], slp[1:Rr + 1], p, n0_h, eos, no_ts, V=V, suppress=sup_t,
                            begin_suppress=beg_t, max_initial=max_initial)
        got, got_lp, got_desc = tok_d[:, p + 1].tolist(), slp.cpu().numpy(), desc.cpu().numpy()
        full_sup = sup + ([4, eos] if first else [])
        for r in rows:
            if done0[r]:
                assert got[r] == eos and got_lp[1 + r] == 0.0
                continue
            pick, logp, _, _ = LR.ts_pick_ref(hists[r], x[r], eos, no_ts, max_initial, full_sup)
            _, logp32, _, _ = LR.ts_pick_ref(hists[r], x[r], eos, no_ts, max_initial, full_sup, dtype=np.float32)
            ban, _ = LR.ts_mask(hists[r], x[r], eos, no_ts, max_initial, full_sup)
            assert got[r] == pick and last[r].item() == pick, (r, hists[r], got[r], pick)
            want_mask = ban | ~np.isfinite(x[r])
            got_mask = LR.desc_mask(got_desc[1 + r], V, eos, no_ts, full_sup) | ~np.isfinite(x[r])
            assert (got_mask == want_mask).all(), (r, hists[r], got_desc[1 + r])
            assert done[r].item() == int(pick == eos)
            err, err32 = abs(float(got_lp[1 + r]) - logp), abs(logp32 - logp)
            bound = 4.0 * max(err32, float(np.spacing(np.float32(abs(logp)))), 2.0 ** -23)
            worst, worst32 = max(worst, err), max(worst32, err32)
            assert err <= bound, (r, err, bound)
        # containment: guard cells, the other columns, the logits
        assert got_lp[0] == 0.5 and got_lp[-1] == 0.5 and (got_desc[0] == -7).all() and (got_desc[-1] == -7).all()
        assert alive[0].item() == -5 and alive[2].item() == -5 and alive[1].item() == sum(1 for r in range(Rr) if not done[r].item())
        rest = tok_d.clone()
        rest[:, p + 1] = before[:, p + 1]
        assert torch.equal(rest, before) and torch.equal(dl.cpu(), wide)
    print(f"V={V} R={Rr} max_initial={max_initial}: sum_logp error {worst:.2e} (float32 NumPy {worst32:.2e})")


def test_ts_entries_refuse_bad_arguments():
    from f5e_tts_amd import _C, ops
    z = lambda *s: torch.zeros(*s, dtype=I32, device="cuda")       # noqa: E731
    x = torch.zeros(2, 162, device="cuda")
    with pytest.raises(_C.F5EError, match="no_timestamps"):
        ops.whisper_ts_pick(x, z(2, 8), z(2), z(2), z(1), torch.zeros(2, device="cuda"), 2, 3, 100, 161)
    with pytest.raises(_C.F5EError, match="no_timestamps"):
        ops.whisper_ts_rule(x, z(2, 8), 2, 3, 120, 110)                       # eos above <|notimestamps|>
    with pytest.raises(_C.F5EError, match="p >= n0 - 1"):
        ops.whisper_ts_rule(x, z(2, 8), 1, 3, 100, 110)
    with pytest.raises(_C.F5EError, match="sum_logp"):
        ops.whisper_ts_pick(x, z(2, 8), z(2), z(2), z(1), torch.zeros(3, device="cuda"), 2, 3, 100, 110)
    with pytest.raises(_C.F5EError, match="desc"):
        ops.whisper_beam_step_ts(x, torch.zeros(2, device="cuda"), z(2, 8), z(2, 8), z(2, 8) + 1, z(2, 8) + 1, z(2), z(1, 2, 8),
                                 z(1, 2), torch.zeros(1, 2, device="cuda"), z(1), z(1), z(1), 2, 3, 8, 100, 2, 110, z(3, 4))


@pytest.mark.parametrize("V", (162, 51866))
def test_beam_step_ts_equals_the_restatement(V):
    """Two utterances of K = 3 rows with different histories per row, one step in the middle of a search and the first step."""
    from f5e_tts_amd import ops
    K, B, n0, cap = 3, 2, 3, 12
    x, _, eos, no_ts, sup = crafted(V, B * K, 7, ties=False)
    tb = no_ts + 1
    for hists in ([[tb + 1, 9], [tb + 1, 9, tb + 4], [tb + 2, tb + 2], [tb, 5, 6], [tb + 3, 8, tb + 6, tb + 6], [tb + 1]], [[]] * 6):
        n_h = max(len(h) for h in hists)
        p = n0 + n_h - 1
        st = BR.new_state(B, K, cap, [1, 2, 3], eos)
        if n_h:
            st["score"][:] = [-1.0, -1.5, -2.0, -0.5, -0.7, -3.0]
            for r, h in enumerate(hists):                                     # shorter histories start later: pad with text
                st["hyp"][r, n0:p + 1] = [12] * (n_h - len(h)) + h
        want, gap = LR.beam_step_ts_ref(x, st, p, n0, cap, eos, K, no_ts, 25, sup, [4, eos])
        dev = {k: torch.from_numpy(v.astype(np.float32 if v.dtype == np.float64 else np.int32)).cuda() for k, v in st.items()}
        hyp_out, anc_out = torch.full_like(dev["hyp"], -5), torch.full_like(dev["anc"], -5)
        desc = torch.zeros(B * K, 4, dtype=I32).cuda()
        dl = torch.from_numpy(x).cuda()
        ops.whisper_beam_step_ts(dl, dev["score"], dev["hyp"], dev["anc"], hyp_out, anc_out, dev["last"], dev["pool_hyp"],
                                 dev["pool_len"], dev["pool_score"], dev["pool_n"], dev["open"], dev["alive"], p, n0, cap, eos, K,
                                 no_ts, desc, max_initial=25, suppress=torch.tensor(sup, dtype=I32).cuda(),
                                 begin_suppress=torch.tensor([4, eos], dtype=I32).cuda())
        assert gap > 1e-4, gap
        assert hyp_out[:, :p + 2].tolist() == want["hyp"][:, :p + 2].tolist() and (hyp_out[:, p + 2:] == -5).all()
        assert anc_out[:, :p + 1].tolist() == want["anc"][:, :p + 1].tolist() and dev["last"].tolist() == want["last"].tolist()
        fin = np.isfinite(want["score"])
        assert (np.isfinite(dev["score"].cpu().numpy()) == fin).all()
        assert np.abs(dev["score"].cpu().numpy()[fin] - want["score"][fin]).max() < 1e-4
        assert dev["pool_n"].tolist() == want["pool_n"].tolist() and dev["open"].tolist() == want["open"].tolist()
        assert dev["alive"].tolist() == want["alive"].tolist() and torch.equal(dl.cpu(), torch.from_numpy(x))


# ---- the fixture cases -----------------------------------------------------------------------------------------------------------

def run_long(name, rows=None, **kw):
    """transcribe_long on a case's recordings (all rows as one ragged batch, garbage beyond a row's length)."""
    c = case(name)
    rows = list(range(len(c["frames"]))) if rows is None else rows
    waves = [case_wave(c, b) for b in rows]
    S = max(len(w) for w in waves)
    batch = torch.full((len(rows), S + 37), 0.7)
    for i, w in enumerate(waves):
        batch[i, :len(w)] = torch.from_numpy(w.copy())
    return model_gpu(name).transcribe_long(batch.cuda(), [len(w) for w in waves], language="en", beam_size=c.get("num_beams", 1),
                                           no_speech_threshold=c.get("no_speech_threshold"),
                                           logprob_threshold=c.get("logprob_threshold"), **kw)


def check_row(c, b, segs):
    want = c["segments"][b]
    assert [s.tokens for s in segs] == [s["tokens"] for s in want]
    assert all(abs(s.start_s - q["start"]) < 1e-9 and abs(s.end_s - q["end"]) < 1e-9 for s, q in zip(segs, want))
    seeks = [s[b] for s in c["seeks"] if s[b] < c["frames"][b]]
    kept = [sk for sk, k in zip(seeks, c["kinds"][b]) if k != "k"]
    assert sorted({s.seek for s in segs}) == kept                             # the seek trajectory of the windows that were kept
    if c.get("num_beams", 1) > 1:
        return None
    rec = [w for w, k in zip(windows_of(c, b), c["kinds"][b]) if k != "k"]
    got = {s.seek: (s.avg_logprob, s.no_speech_prob) for s in segs}
    got = [got[k] for k in kept]
    return rel_l2([g[0] for g in got], [w[0] for w in rec]), rel_l2([g[1] for g in got], [w[1] for w in rec])


@pytest.mark.parametrize("name", ("a", "b", "c", "e", "f", "g", "h"))
@pytest.mark.parametrize("sync_every", (1, 8))
def test_fixture_cases(name, sync_every):
    c = case(name)
    out = run_long(name, sync_every=sync_every)
    for b in range(len(c["frames"])):
        errs = check_row(c, b, out[b])
        if errs is not None:
            print(f"case {name}[{b}] sync_every={sync_every}: avg_logprob rel-L2 {errs[0]:.2e}, no_speech_prob rel-L2 {errs[1]:.2e} "
                  f"(gate {GATE:g})")
            assert errs[0] < GATE and errs[1] < GATE
        assert all(s.compression_ratio > 0 for s in out[b])


def test_ragged_batch_rows_equal_their_own_runs_bit_for_bit():
    both = run_long("f")
    for b in range(2):
        alone = run_long("f", rows=[b])[0]
        assert alone == both[b]                                               # dataclass equality: every float bit for bit


def test_short_recording_equals_generate_with_timestamps():
    c = case("g")
    w = torch.from_numpy(case_wave(c).copy()).cuda()[None]
    model = model_gpu("g")
    segs = model.transcribe_long(w, language="en")[0]
    eos = model.cfg.eos_token_id
    assert [s.tokens for s in segs] == [s["tokens"] for s in c["segments"][0]]
    for K in (1, 3):
        tokens, n = model.generate(w, None, "en", return_timestamps=True, beam_size=K)[:2]
        seq = tokens[0, 3:int(n[0])].tolist()
        seq = seq[:-1] if seq[-1] == eos else seq
        assert tokens[0, :3].tolist() == [101, 102, 106] and seq[0] >= model.cfg.timestamp_begin and 110 not in seq
        if K == 1:                                                            # one window: the same tokens, cut into segments
            kept = [t for s in segs if s.seek == 0 for t in s.tokens]
            assert kept == seq[:len(kept)] and (len(kept) == len(seq) or c["kinds"][0][0] == "p")
        else:
            first = model.transcribe_long(w, language="en", beam_size=3)[0][0].tokens
            assert first == seq[:len(first)]


def test_detect_language_and_generate_without_a_language():
    c = case("i")
    model = model_gpu("i")
    batch = torch.stack([torch.from_numpy(case_wave(c, b).copy()) for b in range(3)]).cuda()
    kv = model.encode(batch)
    assert model.detect_language(kv).tolist() == c["languages"]
    tokens, n = model.generate(batch, None, None, max_new_tokens=4)
    assert tokens[:, 1].tolist() == c["languages"] and tokens[:, 0].tolist() == [101] * 3 and tokens[:, 3].tolist() == [110] * 3
    for b in range(3):                                                        # a detected prompt decodes as the named one does
        name = {102: "en", 103: "zh", 104: "de"}[c["languages"][b]]
        t1, n1 = model.generate(batch[b:b + 1], None, name, max_new_tokens=4)
        assert torch.equal(t1[0], tokens[b]) and n1[0] == n[b]
    lo, hi = c["auto_wave"]
    w = torch.from_numpy(gold()["wave_f32"][lo:hi].copy()).cuda()[None]
    segs = model.transcribe_long(w, language=None)[0]
    assert [s.tokens for s in segs] == [s["tokens"] for s in c["auto_segments"][0]]


# ---- unchanged behaviour ---------------------------------------------------------------------------------------------------------

def test_generate_without_the_new_arguments_is_unchanged():
    from test_whisper_cpu import gold as gold0, tiny_model as tiny0
    fx = gold0()
    model = tiny0().cuda()
    w = torch.from_numpy(fx["wave_f32"][:14400].copy()).cuda()[None]
    tokens, n = model.generate(w, None, "en")
    want = fx["tokens_14400"]
    assert tokens[0, :int(n[0])].tolist() == want.tolist()


# ---- the wiring, end to end: a checkpoint directory, a recording longer than a window ------------------------------------------------

def test_recognizer_long_form_from_a_checkpoint_directory(tmp_path):
    """``eval_wer --asr whisper --whisper_long --whisper_beam N`` and ``infer_cli --ref_language auto`` build exactly this: the
    recogniser reaches the end of a recording longer than one window and detects its language; without ``long_form`` it still
    cuts the recording with its warning."""
    import json
    from f5e_tts_amd.eval.whisper import WhisperRecognizer
    from test_whisper_cpu import write_safetensors
    fx, c = gold(), case("a")
    d = tmp_path / "ckpt"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(fx["config"]))
    (d / "generation_config.json").write_text(json.dumps(fx["generation_config"]))
    (d / "vocab.json").write_text(json.dumps({f"w{i}": i for i in range(100)}))
    (d / "added_tokens.json").write_text(json.dumps({f"<|s{i}|>": i for i in range(100, 162)}))
    write_safetensors(str(d / "model.safetensors"), {k: (v, "F32") for k, v in LR.case_sd(fx, c).items()})
    wave = torch.from_numpy(case_wave(c).copy())
    rec = WhisperRecognizer(str(d), "cuda", "en", beam_size=1, long_form=True)
    segs = rec.transcribe_segments(wave, 16000)
    want = c["segments"][0]
    assert len(segs) == len(want) and segs[-1][1] > 3.0                                                    # windows are 1 s
    assert all(abs(s[0] - q["start"]) < 1e-9 and abs(s[1] - q["end"]) < 1e-9 for s, q in zip(segs, want))
    assert [s[2] for s in segs] == ["".join(f"w{t}" for t in q["tokens"] if t < 100) for q in want]
    assert rec.transcribe(wave, 16000) == "".join(s[2] for s in segs).strip()
    auto = WhisperRecognizer(str(d), "cuda", "auto", beam_size=3, long_form=True)
    assert auto.transcribe_segments(wave, 16000)[-1][0] >= 2.0                  # segments from beyond the second window
    lang = auto.model.detect_language(auto.model.encode(wave[None, :16000].cuda())).tolist()
    assert lang == case("i")["languages"][:1]
    plain = WhisperRecognizer(str(d), "cuda", "en")
    with pytest.warns(UserWarning, match="only the first 1 s are transcribed"):
        short = plain.transcribe(wave, 16000)
    assert short and short != rec.transcribe(wave, 16000)
