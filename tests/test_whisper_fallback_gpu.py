"""Whisper's sampled step and temperature fallback on the GPU (f5e_whisper_sample_pick in csrc/whisper.hip;
``transcribe_long(fallback=...)`` and ``generate(temperature=...)`` in eval/whisper.py) against
  * the float64 restatement tests/whisper_sample_ref.py on the step inputs of ``pick_inputs`` (V 5 .. 51866, every rule state, two
    temperatures, row keys that are not the row index, a non-zero serial);
  * the fixture made from ``transformers`` (tests/golden/whisper_fallback.npz): tokens, segments, seeks, the temperature kept per
    window and the needs_fallback / should_skip flags of every attempt equal.

Decided draws.  The kernel evaluates y = x / T + g in fp32: one division (2.5 ulp allowed, |x / T| <= 12 / T), e = -log(u) or
-log1p(-(1 - u)) from an argument that fp32 holds exactly (3 ulp of e, which moves log(e) by 3 * 2^-23), g = -log(e) (3 ulp of
|g| <= 17.33 < 32, i.e. 3 * 2^-19) and one addition (half an ulp of |y| < 128, i.e. 2^-18).  A gap of two such values is off by at
most tau = 2 * (2.5 * 2^-23 * 12 / T + 3 * 2^-23 + 3 * 2^-19 + 2^-18) = 5.6e-5 at T = 0.2 and 2.7e-5 at T = 1
(``whisper_sample_ref.pick_tau``; derived, not measured).  Where the restatement's gap between its two largest perturbed values
is at least tau the pick must be equal; draws below it may be at most 1 % of a test's draws, and
tests/test_whisper_fallback_cpu.py proves on the restatement alone that these inputs have none.

``sum_logp``: the bound of tests/test_whisper_long_gpu.py for f5e_whisper_ts_pick (4 x the error of a NumPy float32 evaluation of
the same formula, floored at one float32 spacing and 2^-23).  ``avg_logprob`` of the fixture cases: the same 2e-4 gate."""
import numpy as np
import pytest
import torch

import whisper_sample_ref as S
from test_whisper_fallback_cpu import fb_case, fb_gold, fb_model

pytestmark = pytest.mark.gpu

GATE = 2e-4
F32, I32 = torch.float32, torch.int32
N0 = 3
_dev = {}


def model_gpu(c):
    rs = tuple(tuple(r) for r in c["row_scale"])
    if rs not in _dev:
        _dev[rs] = fb_model(c).cuda()
    return _dev[rs]


def launch(x, hist, T, row_key, serial, seed, *, ld=None, done0=None, no_rules=False, layout=None, slp0=0.0):
    """One f5e_whisper_sample_pick on rows that share a history, every output inside guard cells.  -> dict of host arrays."""
    from f5e_tts_amd import ops
    R, V = x.shape
    eos, no_ts, sup, beg, mi = layout or S.pick_layout(V)
    p = N0 + len(hist) - 1
    ld = V if ld is None else ld
    wide = torch.full((R, ld), 1e9)
    wide[:, :V] = torch.from_numpy(x)
    dl = wide.cuda()
    tokens = torch.full((R + 2, p + 4), -5, dtype=I32)
    tokens[:, N0:p + 1] = torch.tensor(hist, dtype=I32)
    tok_d = tokens.cuda()
    last, done = torch.full((R + 2,), -5, dtype=I32).cuda(), torch.full((R + 2,), -5, dtype=I32).cuda()
    done[1:R + 1] = torch.tensor(done0 or [0] * R, dtype=I32).cuda()
    alive, slp = torch.full((3,), -5, dtype=I32).cuda(), torch.full((R + 2,), 0.5, dtype=F32).cuda()
    slp[1:R + 1] = slp0                                                       # the rows' own cells
    before = dict(tokens=tok_d.clone(), last=last.clone(), done=done.clone(), alive=alive.clone(), slp=slp.clone())
    args = (dl[:, :V], tok_d[1:R + 1], last[1:R + 1], done[1:R + 1], alive[1:2], slp[1:R + 1], p, N0, eos, None if no_rules else no_ts,
            T, seed, torch.from_numpy(row_key).cuda(), torch.from_numpy(serial).cuda())
    kw = dict(V=V, suppress=torch.tensor(sup, dtype=I32).cuda() if sup else None,
              begin_suppress=torch.tensor(beg, dtype=I32).cuda() if beg else None, max_initial=None if no_rules else mi)
    try:
        ops.whisper_sample_pick(*args, **kw)
        err = None
    except Exception as e:                                                    # noqa: BLE001 -- the refusal tests read it
        err = e
    out = dict(tokens=tok_d.cpu().numpy(), last=last.cpu().numpy(), done=done.cpu().numpy(), alive=alive.cpu().numpy(),
               slp=slp.cpu().numpy(), p=p, err=err, before={k: v.cpu().numpy() for k, v in before.items()})
    assert dl.cpu().numpy().tobytes() == wide.numpy().tobytes()               # the logits are only read (bytes: a row may hold NaN)
    return out


def contained(o, R):
    """Guard cells and the columns other than p + 1 are untouched."""
    b, p = o["before"], o["p"]
    rest = o["tokens"].copy()
    rest[1:R + 1, p + 1] = b["tokens"][1:R + 1, p + 1]
    assert (rest == b["tokens"]).all()
    for k in ("last", "done", "slp"):
        assert o[k][0] == b[k][0] and o[k][-1] == b[k][-1], k
    assert o["alive"][0] == -5 and o["alive"][2] == -5


def untouched(o):
    return all((o[k] == o["before"][k]).all() for k in ("tokens", "last", "done", "alive", "slp"))


# ---- picks against the restatement -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V,R", S.PICK_SHAPES)
@pytest.mark.parametrize("T", S.PICK_TEMPERATURES)
def test_sample_pick_equals_the_restatement(V, R, T):
    eos, no_ts, sup, beg, mi = S.pick_layout(V)
    tau, draws, undecided, worst, worst32 = S.pick_tau(T), 0, 0, 0.0, 0.0
    for hist, x, rk, se in S.pick_inputs(V, R, T):
        o = launch(x, hist, T, rk, se, S.PICK_SEED, ld=V + (3 if V % 2 else 0))
        assert o["err"] is None, o["err"]
        contained(o, R)
        full_sup = sup + (beg if not hist else [])
        for r in range(R):
            pick, logp, gap = S.sample_pick_ref(hist, x[r], eos, no_ts, T, S.PICK_SEED, o["p"], int(se[r]), int(rk[r]), mi, full_sup)
            _, logp32, _ = S.sample_pick_ref(hist, x[r], eos, no_ts, T, S.PICK_SEED, o["p"], int(se[r]), int(rk[r]), mi, full_sup,
                                             dtype=np.float32)
            got = int(o["tokens"][1 + r, o["p"] + 1])
            draws += 1
            if gap < tau:
                undecided += 1
            else:
                assert got == pick, (hist, r, got, pick, gap)
            assert o["last"][1 + r] == got and o["done"][1 + r] == int(got == eos)
            if got == pick:
                err, err32 = abs(float(o["slp"][1 + r]) - logp), abs(logp32 - logp)
                bound = 4.0 * max(err32, float(np.spacing(np.float32(abs(logp)))), 2.0 ** -23)
                worst, worst32 = max(worst, err), max(worst32, err32)
                assert err <= bound, (hist, r, err, bound)
        assert o["alive"][1] == R - int(o["done"][1:R + 1].sum())
    print(f"V={V} R={R} T={T}: {draws} draws, {undecided} undecided (tau {tau:.1e}); sum_logp error {worst:.2e} "
          f"(float32 NumPy {worst32:.2e})")
    assert undecided <= 0.01 * draws


def test_no_rules_all_banned_and_done_rows():
    V, R, T = 162, 3, 0.6
    hist, x, rk, se = S.pick_inputs(V, R, 1.0)[3]
    eos, no_ts, sup, beg, mi = S.pick_layout(V)
    # without the timestamp rules: every class that is not suppressed competes, <|notimestamps|> included
    o = launch(x, hist, T, rk, se, 7, no_rules=True)
    assert o["err"] is None
    contained(o, R)
    for r in range(R):
        pick, logp, gap = S.sample_pick_ref(hist, x[r], eos, None, T, 7, o["p"], int(se[r]), int(rk[r]), None, sup)
        assert gap >= S.pick_tau(T) and o["tokens"][1 + r, o["p"] + 1] == pick
        assert abs(float(o["slp"][1 + r]) - logp) < 1e-5
    # a done row gets eos and keeps its sum; a row whose classes are all banned picks 0 and keeps it too
    y = x.copy()
    y[1, :] = -np.inf
    y[1, 5] = np.nan
    o = launch(y, hist, T, rk, se, 7, done0=[0, 0, 1], slp0=0.25)
    contained(o, R)
    assert o["tokens"][2, o["p"] + 1] == 0 and o["last"][2] == 0 and o["slp"][2] == 0.25 and o["done"][2] == 0
    assert o["tokens"][3, o["p"] + 1] == eos and o["last"][3] == eos and o["slp"][3] == 0.25 and o["done"][3] == 1
    assert o["alive"][1] == 2


def test_determinism_and_independence():
    V, R, T = 51866, 3, 1.0
    hist, x, rk, se = S.pick_inputs(V, R, T)[3]
    a = launch(x, hist, T, rk, se, S.PICK_SEED)
    b = launch(x, hist, T, rk, se, S.PICK_SEED)
    assert all((a[k] == b[k]).all() for k in ("tokens", "last", "done", "alive")) and a["slp"].tobytes() == b["slp"].tobytes()
    for r in range(R):                                                        # a row equals its own R = 1 launch
        one = launch(x[r:r + 1], hist, T, rk[r:r + 1], se[r:r + 1], S.PICK_SEED)
        assert one["tokens"][1, one["p"] + 1] == a["tokens"][1 + r, a["p"] + 1]
        assert one["slp"][1:2].tobytes() == a["slp"][1 + r:2 + r].tobytes()
    eos, no_ts, sup, beg, mi = S.pick_layout(V)
    ref = [[S.sample_pick_ref(hist, x[r], eos, no_ts, T, seed, a["p"], int(se[r]), int(rk[r]), mi, sup) for r in range(R)]
           for seed in (S.PICK_SEED, S.PICK_SEED + 1)]
    assert any(u[0] != v[0] for u, v in zip(*ref)) and all(u[2] >= S.pick_tau(T) for row in ref for u in row)
    c = launch(x, hist, T, rk, se, S.PICK_SEED + 1)
    assert [int(t) for t in c["tokens"][1:R + 1, c["p"] + 1]] == [u[0] for u in ref[1]]
    assert [int(t) for t in a["tokens"][1:R + 1, a["p"] + 1]] == [u[0] for u in ref[0]]


def test_refusals_leave_the_outputs_untouched():
    from f5e_tts_amd import _C
    V, R = 162, 2
    hist, x, rk, se = S.pick_inputs(V, 3, 1.0)[3]
    x, rk, se = x[:R], rk[:R], se[:R]
    eos, no_ts, sup, beg, mi = S.pick_layout(V)
    for T in (0.0, -0.5, float("nan"), float("inf")):
        o = launch(x, hist, T, rk, se, 1)
        assert isinstance(o["err"], _C.F5EError) and "temperature" in str(o["err"]) and untouched(o), T
    for layout, word in (((eos, V - 1, sup, beg, mi), "no_timestamps"), ((no_ts + 1, no_ts, sup, beg, mi), "no_timestamps"),
                         ((V, no_ts, sup, beg, mi), "eos"), ((eos, no_ts, sup, beg, -2), "max_initial")):
        o = launch(x, hist, 0.5, rk, se, 1, layout=layout)
        assert isinstance(o["err"], _C.F5EError) and word in str(o["err"]) and untouched(o), layout
    o = launch(x, hist, 0.5, rk[:1], se, 1)
    assert isinstance(o["err"], _C.F5EError) and "row_key" in str(o["err"]) and untouched(o)


# ---- the fixture cases ---------------------------------------------------------------------------------------------------------------

def run_case(c, waves=None, row_keys=None, **kw):
    from f5e_tts_amd.eval.whisper import Fallback
    fx = fb_gold()
    waves = [fx["wave_f32"][c["waves"][0][0]:c["waves"][0][1]]] if waves is None else waves
    L = max(len(w) for w in waves)
    batch = torch.full((len(waves), L + 37), 0.7)
    for i, w in enumerate(waves):
        batch[i, :len(w)] = torch.from_numpy(w.copy())
    trace = []
    fb = Fallback(tuple(c["temperatures"]), c["compression_ratio_threshold"], c["logprob_threshold"], c["seed"])
    out = model_gpu(c).transcribe_long(batch.cuda(), [len(w) for w in waves], language="en", beam_size=c["num_beams"],
                                       no_speech_threshold=c["no_speech_threshold"], fallback=fb,
                                       row_keys=[c["row_key"]] if row_keys is None else row_keys, trace=trace, **kw)
    return out, trace


def check_case(c, segs, trace):
    want = c["segments"]
    assert [s.tokens for s in segs] == [s["tokens"] for s in want]
    assert all(abs(s.start_s - q["start"]) < 1e-9 and abs(s.end_s - q["end"]) < 1e-9 for s, q in zip(segs, want))
    seeks = sorted({t["seek"] for t in trace})
    assert seeks == c["seeks"]
    got_avg, want_avg = [], []
    for sk, attempts in zip(c["seeks"], c["windows"]):
        mine = [t for t in trace if t["seek"] == sk]
        assert [(t["temperature"], t["needs_fallback"], t["should_skip"]) for t in mine] == [(a[0], a[3], a[4]) for a in attempts]
        assert all(abs(t["compression_ratio"] - a[1]) < 1e-12 for t, a in zip(mine, attempts))
        got_avg += [t["avg_logprob"] for t, a in zip(mine, attempts) if a[2] is not None]
        want_avg += [a[2] for a in attempts if a[2] is not None]
        kept = [s for s in segs if s.seek == sk]
        assert all(s.temperature == attempts[-1][0] for s in kept) and (not attempts[-1][4] or not kept)
    if want_avg:
        err = float(np.linalg.norm(np.array(got_avg) - np.array(want_avg)) / np.linalg.norm(want_avg))
        print(f"case {c['name']}: avg_logprob rel-L2 {err:.2e} (gate {GATE:g})")
        assert err < GATE


@pytest.mark.parametrize("name", tuple("abcdefg"))
@pytest.mark.parametrize("sync_every", (1, 8))
def test_fixture_cases(name, sync_every):
    c = fb_case(name)
    out, trace = run_case(c, sync_every=sync_every)
    check_case(c, out[0], trace)


def test_short_form_sampling_without_timestamps():
    c, fx = fb_case("h"), fb_gold()
    w = torch.from_numpy(fx["wave_f32"][c["waves"][0][0]:c["waves"][0][1]].copy()).cuda()[None]
    model = model_gpu(c)
    tokens, n = model.generate(w, None, "en", temperature=c["temperature"], seed=c["seed"])
    assert tokens[0, :4].tolist() == [101, 102, 106, 110] and tokens[0, 4:int(n[0])].tolist() == c["tokens"]
    stats = {}
    model.generate_from_kv(model.encode(w), [101, 102, 106, 110], stats=stats, temperature=c["temperature"], seed=c["seed"])
    assert abs(float(stats["sum_logp"][0]) / len(c["tokens"]) - c["avg_logprob"]) < GATE * abs(c["avg_logprob"])
    with_ts, _ = model.generate(w, None, "en", temperature=c["temperature"], seed=c["seed"], return_timestamps=True)
    assert with_ts[0, 3].item() >= model.cfg.timestamp_begin                 # the rules hold while sampling


def test_batch_of_two_equals_the_rows_own_runs():
    """The recordings of (b) and (f) as one B = 2 call under (f)'s model and record (a call has one of each): row 1 is (f) itself,
    with its row key 1, and both rows equal their own B = 1 runs."""
    b, f, fx = fb_case("b"), fb_case("f"), fb_gold()
    wb = fx["wave_f32"][b["waves"][0][0]:b["waves"][0][1]]
    wf = fx["wave_f32"][f["waves"][0][0]:f["waves"][0][1]]
    both, trace = run_case(f, waves=[wb, wf], row_keys=[0, 1])
    check_case(f, both[1], [t for t in trace if t["row"] == 1])
    alone0, _ = run_case(f, waves=[wb], row_keys=[0])
    alone1, _ = run_case(f, waves=[wf], row_keys=[1])
    assert both[0] == alone0[0] and both[1] == alone1[0]                      # dataclass equality: every float bit for bit


# ---- opt-in ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("a", "e", "f", "h"))
def test_fallback_none_and_a_single_zero_temperature_change_nothing(name):
    from f5e_tts_amd.eval.whisper import Fallback
    from test_whisper_long_gpu import check_row, run_long
    from test_whisper_long_cpu import case
    c = case(name)
    base = run_long(name)
    assert run_long(name, fallback=None) == base and run_long(name, fallback=Fallback(temperatures=(0.0,))) == base
    for b in range(len(c["frames"])):
        check_row(c, b, base[b])
        assert all(s.temperature == 0.0 for s in base[b])
