"""The captured Whisper decode step on the GPU (csrc/whisper_step.hip; ``generate_from_kv(step_graph=True)`` in eval/whisper.py).

Kernel level: every device-position kernel against its host-position twin on the same inputs, ``torch.equal`` (they share one
body, so there is no tolerance to set): f5e_attn_decode_dev_f32 for every head dim the twin is built for, positions on both
sides of the 64-lane stride, with and without ``begin``; f5e_whisper_embed_dev; the three picks on crafted rows (first step,
later step, a done row, ties, V = 160 / 163 / 51866).  Containment: every cache slot but [r][p], the output's padding, the
logits, the token table but column p + 1 and the record but p keep their bytes; a record outside the launch's extents
(p = P + 1, p = -3) lands in the last / first slot, which guard rows and columns behind the extents would show otherwise.

End to end: the replayed run against the eager run of the same call, tokens, counts, ``sum_logp`` and ``no_speech_logp`` with
``torch.equal`` ("f32" replays the eager launches), and against the fixture's tokens; a second call on a cached state with other
audio, another prompt length and another bound (stale cross keys, a baked position or prompt length would show here); another
row count; the LRU.  ``step_gemm="skinny"`` changes the summation order: tokens equal the fixture (every margin is >= 1e-2 of
the logits' RMS) and ``sum_logp`` of the same tokens lies within 2e-4, relative, of the eager run's (the project's gate for
fp32 chains, tests/test_whisper_gpu.py).  ``transcribe_long(step_graph=True)`` gives the eager segments, bit for bit.

Measured on an MI355X: see DESIGN.md 4o."""
import numpy as np
import pytest
import torch

from test_whisper_cpu import gold, tiny_model
from test_whisper_gpu import kv_gpu, model_gpu
from test_whisper_long_gpu import check_row, crafted, run_long
from test_whisper_long_gpu import model_gpu as long_model_gpu
from test_whisper_long_cpu import case, case_wave

pytestmark = pytest.mark.gpu

GATE = 2e-4
F32, I32 = torch.float32, torch.int32


def rec_of(p, n0=1, seed=0, temperature=0.0):
    from f5e_tts_amd import ops
    return ops.whisper_step_record(p, n0, seed, temperature).cuda()


# ---- f5e_attn_decode_dev_f32 -----------------------------------------------------------------------------------------------------

def attn_inputs(dk, R=3, H=2, P=136, guard=4, seed=0):
    g = torch.Generator().manual_seed(seed + dk)
    D = H * dk
    qkv = torch.randn(R, 3 * D + 4, generator=g).cuda()[:, :3 * D]          # a row-strided view
    kc, vc = torch.randn(R, P + guard, D, generator=g).cuda(), torch.randn(R, P + guard, D, generator=g).cuda()
    return qkv, kc, vc, D


def attn_pair(dk, p, begin, rec_p=None, R=3, H=2, P=136):
    """-> (out, kc, vc) of the device-position launch and of its twin at ``p``; ``rec_p``: what the record holds (None: p)."""
    from f5e_tts_amd import ops
    qkv, kc, vc, D = attn_inputs(dk, R, H, P)
    scale = dk ** -0.5
    bt = None if begin is None else torch.tensor(begin, dtype=I32).cuda()
    kc2, vc2 = kc.clone(), vc.clone()
    pad = torch.full((R, D + 8), -7.0).cuda()
    pad2 = pad.clone()
    rec = rec_of(p if rec_p is None else rec_p, 3, 11, 0.5)
    rec0 = rec.clone()
    ops.attn_decode_dev_f32(qkv, kc[:, :P], vc[:, :P], rec, H, scale, out=pad[:, :D], begin=bt)
    ops.attn_decode_f32(qkv, kc2[:, :P], vc2[:, :P], p, H, scale, out=pad2[:, :D], begin=bt)
    assert torch.equal(rec, rec0)                                            # the attention reads the record, nothing more
    assert (pad[:, D:] == -7.0).all()                                        # the output's padding
    return (pad, kc, vc), (pad2, kc2, vc2), qkv


@pytest.mark.parametrize("with_begin", (False, True))
@pytest.mark.parametrize("dk", (16, 32, 64, 128))
def test_attn_decode_dev_equals_its_twin(dk, with_begin):
    for p in (0, 1, 63, 64, 65, 130):
        begin = [0, min(p, 5), p] if with_begin else None                     # begin[r] = p: the row sees its own position only
        got, want, qkv = attn_pair(dk, p, begin)
        first = attn_inputs(dk)
        for a, b in zip(got, want):
            assert torch.equal(a, b), (dk, p, with_begin)
        D = first[3]
        for cache, src, off in ((got[1], first[1], D), (got[2], first[2], 2 * D)):
            keep = torch.ones(cache.shape[1], dtype=torch.bool)
            keep[p] = False
            assert torch.equal(cache[:, keep.cuda()], src[:, keep.cuda()])    # every slot but [r][p], the guard rows included
            assert torch.equal(cache[:, p], qkv[:, off:off + D])              # ... which holds the step's k / v
        assert torch.isfinite(got[0][:, :D]).all()


@pytest.mark.parametrize("with_begin", (False, True))
@pytest.mark.parametrize("dk", (16, 128))
def test_attn_decode_dev_clamps_the_record_to_the_caches(dk, with_begin):
    P = 136
    for rec_p, p in ((P + 1, P - 1), (-3, 0), (2 ** 31 - 1, P - 1), (-2 ** 31, 0)):
        got, want, _ = attn_pair(dk, p, [0, 3, 200] if with_begin else None, rec_p=rec_p)
        first = attn_inputs(dk)
        for a, b in zip(got, want):
            assert torch.equal(a, b), (dk, rec_p)
        assert torch.equal(got[1][:, P:], first[1][:, P:]) and torch.equal(got[2][:, P:], first[2][:, P:])      # the guard rows


def test_attn_decode_dev_refuses_bad_arguments():
    from f5e_tts_amd import _C, ops
    qkv, kc, vc, D = attn_inputs(16)
    with pytest.raises(_C.F5EError, match="rec"):
        ops.attn_decode_dev_f32(qkv, kc, vc, torch.zeros(4, dtype=I32).cuda(), 2, 0.25)
    with pytest.raises(_C.F5EError, match="rec"):
        ops.attn_decode_dev_f32(qkv, kc, vc, torch.zeros(12, dtype=I32).cuda()[1:9], 2, 0.25)        # not 16-byte aligned
    with pytest.raises(_C.F5EError, match="heads"):
        ops.attn_decode_dev_f32(qkv, kc, vc, rec_of(0), 5, 0.25)
    with pytest.raises(_C.F5EError, match="begin"):
        ops.attn_decode_dev_f32(qkv, kc, vc, rec_of(0), 2, 0.25, begin=torch.zeros(2, dtype=I32).cuda())


# ---- f5e_whisper_embed_dev -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_begin", (False, True))
def test_embed_dev_equals_its_twins_and_clamps(with_begin):
    from f5e_tts_amd import ops
    R, D, V, P = 3, 64, 160, 48
    g = torch.Generator().manual_seed(3)
    emb, pos = torch.randn(V, D, generator=g).cuda(), torch.randn(P, D, generator=g).cuda()
    last = torch.tensor([5, 159, 400], dtype=I32).cuda()                      # the last id lies outside the table: clamped
    for rec_p, p in ((0, 0), (1, 1), (17, 17), (P - 1, P - 1), (P + 5, P + 5), (-3, 0)):
        begin = [0, min(p, 4), p] if with_begin else None
        bt = None if begin is None else torch.tensor(begin, dtype=I32).cuda()
        out = torch.full((R + 1, D), -7.0).cuda()
        rec = rec_of(rec_p)
        ops.whisper_embed_dev(last, emb, pos, out[:R], rec, bt)
        rows = [min(max(p - (begin[r] if begin else 0), 0), P - 1) for r in range(R)]
        want = emb[last.clamp(0, V - 1).long()] + pos[torch.tensor(rows).cuda()]      # one fp32 addition: exact in torch too
        assert torch.equal(out[:R], want) and (out[R] == -7.0).all() and rec.tolist()[0] == rec_p, (rec_p, with_begin)
        if p < P:                                                                # the twins refuse a position outside the table
            twin = torch.empty(R, 1, D).cuda()
            if with_begin:
                ops.whisper_embed(last.view(R, 1), emb, pos, twin, p, bt)
            else:
                ops.text_gather(last.clamp(0, V - 1).view(R, 1), emb, pos[p:p + 1], None, twin)
            assert torch.equal(out[:R], twin.view(R, D)), (rec_p, with_begin)


# ---- the three picks -------------------------------------------------------------------------------------------------------------

def pick_pair(kind, V, Rr, p, n0, rec_p=None, rec_n0=None, n_tok=16, guard=4):
    """The device-position pick against its twin at (p, n0) on crafted rows: histories per row behind column n0, ties, a done
    row; tokens, last, done, alive and sum_logp equal, everything else untouched, the record advanced by one."""
    from f5e_tts_amd import ops
    x, hists, eos, no_ts, sup = crafted(V, Rr, 100 * V + p)
    tb, L = no_ts + 1, p + 1 - n0
    ld = (V + 3) // 4 * 4 + 4
    wide = torch.full((Rr, ld), 1e9)
    wide[:, :V] = torch.from_numpy(x)
    dl = wide.cuda()
    tokens = torch.full((Rr, n_tok + guard), -5, dtype=I32)
    for r in range(Rr):
        h = hists[r][-L:] if L else []
        tokens[r, n0:p + 1] = torch.tensor([12] * (L - len(h)) + h, dtype=I32)
    done0 = torch.tensor([1 if (r == Rr - 1 and Rr > 1) else 0 for r in range(Rr)], dtype=I32)
    sup_t, beg_t = torch.tensor(sup, dtype=I32).cuda(), torch.tensor([4, eos], dtype=I32).cuda()
    seed, temp = (0x9E3779B9 << 32) | 0x85EBCA6B, 0.7
    outs = []
    for dev in (True, False):
        tok, last, done = tokens.cuda(), torch.full((Rr,), -5, dtype=I32).cuda(), done0.cuda()
        alive, slp = torch.full((3,), -5, dtype=I32).cuda(), torch.full((Rr + 2,), 0.5, dtype=F32).cuda()
        keys, ser = torch.arange(7, 7 + Rr, dtype=I32).cuda(), torch.arange(Rr, dtype=I32).cuda() % 2
        rec = rec_of(p if rec_p is None else rec_p, n0 if rec_n0 is None else rec_n0, seed, temp)
        rec0 = rec.tolist()
        view, tv, kw = dl[:, :V], tok[:, :n_tok], dict(V=V, suppress=sup_t, begin_suppress=beg_t)
        if kind == "greedy":
            if dev:
                ops.greedy_pick_dev(view, tv, last, done, alive[1:2], rec, eos, **kw)
            else:
                ops.greedy_pick(view, tv, last, done, alive[1:2], p, eos, first_step=p + 1 == n0, **kw)
        elif kind == "ts":
            if dev:
                ops.whisper_ts_pick_dev(view, tv, last, done, alive[1:2], slp[1:Rr + 1], rec, eos, no_ts, max_initial=25, **kw)
            else:
                ops.whisper_ts_pick(view, tv, last, done, alive[1:2], slp[1:Rr + 1], p, n0, eos, no_ts, max_initial=25, **kw)
        else:
            ts = no_ts if kind == "sample_ts" else None
            if dev:
                ops.whisper_sample_pick_dev(view, tv, last, done, alive[1:2], slp[1:Rr + 1], rec, eos, ts, keys, ser,
                                            max_initial=25 if ts else None, **kw)
            else:
                ops.whisper_sample_pick(view, tv, last, done, alive[1:2], slp[1:Rr + 1], p, n0, eos, ts, temp, seed, keys, ser,
                                        max_initial=25 if ts else None, **kw)
        if dev:
            after = rec.tolist()
            assert after[0] == rec0[0] + 1 and after[1:] == rec0[1:], (rec0, after)          # p += 1, nothing else of the record
        assert torch.equal(dl.cpu(), wide)                                                   # the logits
        rest = tok.cpu()
        rest[:, p + 1] = tokens[:, p + 1]
        assert torch.equal(rest, tokens), (kind, dev, p)                                     # the table but column p + 1
        assert alive[0].item() == -5 and alive[2].item() == -5 and slp[0].item() == 0.5 and slp[-1].item() == 0.5
        outs.append((tok[:, p + 1].cpu(), last.cpu(), done.cpu(), alive.cpu(), slp.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b), (kind, V, p, n0, outs)
    col, last, done, alive, _ = outs[0]
    assert torch.equal(col, last) and (col >= 0).all() and (col < V).all()
    assert alive[1].item() == int((done == 0).sum()) and (Rr == 1 or (col[-1].item() == eos and done[-1].item() == 1))
    return col.tolist()


@pytest.mark.parametrize("V,Rr", ((160, 1), (160, 5), (163, 5), (51866, 5)))
@pytest.mark.parametrize("kind", ("greedy", "ts", "sample_ts", "sample"))
def test_pick_dev_equals_its_twin(kind, V, Rr):
    first = pick_pair(kind, V, Rr, p=2, n0=3)                                 # the first step: begin_suppress counts
    later = pick_pair(kind, V, Rr, p=9, n0=3)                                 # a later step, the histories of every rule branch
    assert len(first) == Rr and len(later) == Rr


@pytest.mark.parametrize("kind", ("greedy", "ts", "sample_ts"))
def test_pick_dev_clamps_the_record_to_the_token_table(kind):
    n_tok = 16
    pick_pair(kind, 160, 5, p=n_tok - 2, n0=3, rec_p=n_tok + 5)               # column p + 1 stays inside the table's width
    pick_pair(kind, 160, 5, p=n_tok - 2, n0=3, rec_p=2 ** 31 - 3)
    pick_pair(kind, 160, 5, p=0, n0=1, rec_p=-3)
    pick_pair(kind, 160, 5, p=5, n0=6 if kind != "greedy" else 40, rec_n0=40)  # n0 beyond p + 1: no history (greedy: no begin list)
    if kind != "greedy":
        pick_pair(kind, 160, 5, p=5, n0=1, rec_n0=-2)


# ---- end to end: replayed against eager ---------------------------------------------------------------------------------------------

def totals(model):
    """(captures, replays) over the model's cached states: what a run without ``stats`` is counted by."""
    states = model._fold().get("step_states", {}).values()
    return sum(s.captures for s in states), sum(s.replays for s in states)


def both(model, kv, prompt, stats=True, **kw):
    """The eager run and the replayed run of one call -> (tokens, n, eager stats, replayed stats); equality is asserted.
    ``stats`` False (a model without <|nospeech|>, whose ``stats`` are refused): the counts come from the cached states."""
    se, sg = {}, {}
    if not stats:
        want, n_w = model.generate_from_kv(kv, prompt, **kw)[:2]
        c0, r0 = totals(model)
        got, n_g = model.generate_from_kv(kv, prompt, step_graph=True, **kw)[:2]
        c1, r1 = totals(model)
        assert torch.equal(got, want) and torch.equal(n_g, n_w), (got.tolist(), want.tolist())
        return got, n_g, se, dict(step_graph=dict(captures=c1 - c0, replays=r1 - r0))
    want, n_w = model.generate_from_kv(kv, prompt, stats=se, **kw)[:2]
    got, n_g = model.generate_from_kv(kv, prompt, stats=sg, step_graph=True, **kw)[:2]
    assert torch.equal(got, want) and torch.equal(n_g, n_w), (got.tolist(), want.tolist())
    for name in ("sum_logp", "no_speech_logp", "at_bound"):
        assert (name in se) == (name in sg), name
        if se.get(name) is None:
            assert sg.get(name) is None, name
        else:
            assert torch.equal(sg[name], se[name]), (name, sg[name].tolist(), se[name].tolist())
    assert "step_graph" not in se and set(sg["step_graph"]) == {"captures", "replays"}
    return got, n_g, se, sg


@pytest.mark.parametrize("sync_every", (1, 8))
@pytest.mark.parametrize("name", ("14400", "40000", "48000", "eos"))
def test_greedy_replay_equals_eager_and_the_fixture(name, sync_every):
    fx = gold()
    eos_case = name == "eos"
    n = 14400 if eos_case else int(name)
    model = model_gpu(eos_case)
    tokens, cnt, _, sg = both(model, kv_gpu(n, eos_case), fx["prompt"].tolist(), stats=False, sync_every=sync_every)
    want = fx[f"tokens_{name}"].tolist()
    assert tokens[0, :int(cnt[0])].tolist() == want
    print(f"{name} sync_every={sync_every}: {len(want)} tokens, {sg['step_graph']}")
    assert sg["step_graph"]["replays"] >= len(want) - 4 and sg["step_graph"]["captures"] <= 1


def test_max_new_tokens_and_fresh_results():
    fx, model = gold(), model_gpu()
    tokens, cnt, _, sg = both(model, kv_gpu(40000), fx["prompt"].tolist(), stats=False, max_new_tokens=5, sync_every=3)
    assert tokens.shape == (1, 9) and int(cnt[0]) == 9 and tokens[0].tolist() == fx["tokens_40000"][:9].tolist()
    assert sg["step_graph"]["replays"] == 5 and tokens.is_contiguous()
    keep = tokens.clone()
    both(model, kv_gpu(14400), fx["prompt"].tolist(), stats=False, max_new_tokens=7)      # the same state runs again ...
    assert torch.equal(tokens, keep)                                          # ... and what was returned is not a view of it


def test_generate_from_audio_projects_into_the_state():
    """``generate`` projects the cross keys / values straight into the cached state (``cross_kv(out=)``): nothing is copied, and
    a second recording on the same state decodes as its own eager run."""
    from test_whisper_gpu import wave_gpu
    fx, model = gold(), model_gpu()
    for n in (40000, 14400, 48000):
        want, n_w = model.generate(wave_gpu(n), None, "english", max_new_tokens=9, sync_every=3)
        got, n_g = model.generate(wave_gpu(n), None, "english", max_new_tokens=9, sync_every=3, step_graph=True)
        assert torch.equal(got, want) and torch.equal(n_g, n_w) and got[0].tolist() == fx[f"tokens_{n}"][:13].tolist()
    S = model._fold()["step_states"][(1, "greedy", False, "f32", 150, "cuda:0")]
    kv = model.cross_kv(model.encode_features(model.features(wave_gpu(48000))))
    assert all(torch.equal(buf[..., :64], k) and torch.equal(buf[..., 64:], v) for buf, (k, v) in zip(S.xkv, kv))


def long_kv(name="a"):
    c = case(name)
    model = long_model_gpu(name)
    w = torch.from_numpy(case_wave(c)[:16000].copy()).cuda()[None]
    return model, model.encode(w)


@pytest.mark.parametrize("sync_every", (1, 8))
def test_ruled_replay_equals_eager(sync_every):
    model, kv = long_kv()
    tokens, cnt, se, sg = both(model, kv, [101, 102, 106], return_timestamps=True, sync_every=sync_every)
    seq = tokens[0, 3:int(cnt[0])].tolist()
    print(f"ruled: {seq}, sum_logp {se['sum_logp'].tolist()}, {sg['step_graph']}")
    assert seq[0] >= model.cfg.timestamp_begin and len(seq) > 4 and se["sum_logp"] is not None


@pytest.mark.parametrize("ts", (False, True))
def test_sampled_replay_equals_eager(ts):
    model, kv = long_kv()
    kw = dict(return_timestamps=ts, temperature=0.6, seed=(7 << 40) | 12345, max_new_tokens=14)
    tokens, cnt, se, _ = both(model, kv, [101, 102, 106] if ts else [101, 102, 106, 110], **kw)
    prompt = [101, 102, 106] if ts else [101, 102, 106, 110]
    # the seed, the temperature and the rows' keys are read on the device: other values, no new capture, the eager run's draws
    other, _, _, s2 = both(model, kv, prompt, **dict(kw, seed=99))
    print(f"sampled ts={ts}: {tokens[0].tolist()} / seed 99: {other[0].tolist()}")
    keys = dict(row_key=torch.tensor([5], dtype=I32).cuda(), serial=torch.tensor([2], dtype=I32).cuda())
    _, _, _, s3 = both(model, kv, prompt, **kw, **keys)
    _, _, _, s4 = both(model, kv, prompt, **dict(kw, temperature=1.1))
    assert s2["step_graph"]["captures"] == s3["step_graph"]["captures"] == s4["step_graph"]["captures"] == 0


@pytest.mark.parametrize("prefill", (False, True))
def test_ragged_pair_with_begin_and_prefill(prefill):
    fx, model = gold(), model_gpu()
    forced = [int(t) for t in fx["prompt"]]
    kvs = [kv_gpu(40000), kv_gpu(14400)]
    kv2 = [(torch.cat((a[0], b[0])), torch.cat((a[1], b[1]))) for a, b in zip(*kvs)]
    g = np.random.default_rng(4)
    prompts = [[int(t) for t in g.integers(10, 60, 11)] + forced, [int(t) for t in g.integers(10, 60, 2)] + forced]
    n0 = max(len(p) for p in prompts)
    begin = [n0 - len(p) for p in prompts]
    padded = [[model.cfg.eos_token_id] * b + p for b, p in zip(begin, prompts)]
    tokens, cnt, se, sg = both(model, kv2, padded, stats=False, max_new_tokens=12, begin=begin, prefill=prefill)
    assert sg["step_graph"]["replays"] == 12 and tokens.shape == (2, n0 + 12)


def test_ruled_pair_with_begin_prefill_and_stats():
    model, kv = long_kv()
    kv2 = [(torch.cat((k, k)), torch.cat((v, v))) for k, v in kv]
    prompts = [[108, 20, 21, 22, 23, 24, 101, 102, 106], [101, 102, 106]]
    begin = [0, 6]
    padded = [[model.cfg.eos_token_id] * b + p for b, p in zip(begin, prompts)]
    _, _, se, _ = both(model, kv2, padded, return_timestamps=True, begin=begin, prefill=True)
    assert "at_bound" in se and se["no_speech_logp"].shape == (2,)
    both(model, kv2, padded, return_timestamps=True, begin=begin, prefill=False, max_new_tokens=6)


# ---- reuse: where a captured step goes wrong -------------------------------------------------------------------------------------------

def test_a_cached_state_is_reused_with_other_audio_prompt_length_and_bound():
    fx = gold()
    model = tiny_model().cuda()                                               # its own cache: the counts below are this test's
    forced = fx["prompt"].tolist()
    _, _, _, s1 = both(model, kv_gpu(40000), forced, stats=False, max_new_tokens=12)
    assert s1["step_graph"] == dict(captures=1, replays=12)
    t2, n2, _, s2 = both(model, kv_gpu(14400), [17] + forced, stats=False, max_new_tokens=20)      # other audio, n0 and bound
    assert s2["step_graph"]["captures"] == 0 and s2["step_graph"]["replays"] >= 1 and t2.shape == (1, 25)
    kv2 = [(torch.cat((a[0], b[0])), torch.cat((a[1], b[1]))) for a, b in zip(kv_gpu(40000), kv_gpu(48000))]
    t3, n3, _, s3 = both(model, kv2, forced, stats=False)                                 # another row count: one more capture
    assert s3["step_graph"]["captures"] == 1
    for b, name in enumerate(("40000", "48000")):
        assert t3[b, :int(n3[b])].tolist() == fx[f"tokens_{name}"].tolist()
    t4, n4, _, s4 = both(model, kv_gpu(48000), forced, stats=False)                       # the first state is still usable
    assert s4["step_graph"]["captures"] == 0 and t4[0, :int(n4[0])].tolist() == fx["tokens_48000"].tolist()


def test_the_cache_keeps_four_states_and_survives_eviction():
    from f5e_tts_amd.eval import whisper as W
    fx = gold()
    model = tiny_model().cuda()
    forced, kv = fx["prompt"].tolist(), kv_gpu(40000)
    for B in (1, 2, 3, 4, 5):
        kvb = [(k.expand(B, -1, -1).contiguous(), v.expand(B, -1, -1).contiguous()) for k, v in kv]
        c0 = totals(model)[0]
        tokens = model.generate_from_kv(kvb, forced, max_new_tokens=6, step_graph=True)[0]
        assert all(row == fx["tokens_40000"][:10].tolist() for row in tokens.tolist())
        assert totals(model)[0] - c0 == (1 if B < 5 else 1 - 1)              # B = 5 evicts B = 1 and its one capture
    cache = model._fold()["step_states"]
    assert W.STEP_STATES == 4 and len(cache) == 4 and [k[0] for k in cache] == [2, 3, 4, 5]
    assert all(s.captures == 1 and s.graph is not None for s in cache.values())
    tokens = model.generate_from_kv(kv, forced, max_new_tokens=6, step_graph=True)[0]                # B = 1 was evicted
    assert [k[0] for k in cache] == [3, 4, 5, 1] and cache[next(reversed(cache))].captures == 1
    assert tokens[0].tolist() == fx["tokens_40000"][:10].tolist()
    model.float()                                                             # the weights are folded again: no stale graph
    assert model._folded is None
    model.generate_from_kv(kv, forced, max_new_tokens=3, step_graph=True)
    assert totals(model) == (1, 3)
    torch.cuda.synchronize()


# ---- step_gemm = "skinny" ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("14400", "40000", "48000", "eos"))
def test_skinny_tokens_equal_the_fixture(name):
    fx = gold()
    eos_case = name == "eos"
    n = 14400 if eos_case else int(name)
    model = model_gpu(eos_case)
    r0 = totals(model)[1]
    tokens, cnt = model.generate_from_kv(kv_gpu(n, eos_case), fx["prompt"].tolist(), step_graph=True, step_gemm="skinny")
    assert tokens[0, :int(cnt[0])].tolist() == fx[f"tokens_{name}"].tolist() and fx[f"margin_{name}"].min() >= 1e-2
    assert totals(model)[1] - r0 >= len(fx[f"tokens_{name}"]) - 4


def test_skinny_sum_logp_within_the_gate_of_the_eager_run():
    model, kv = long_kv()
    se, sk = {}, {}
    want, n_w = model.generate_from_kv(kv, [101, 102, 106], return_timestamps=True, stats=se)
    got, n_g = model.generate_from_kv(kv, [101, 102, 106], return_timestamps=True, stats=sk, step_graph=True, step_gemm="skinny")
    err = float((sk["sum_logp"] - se["sum_logp"]).abs().max() / se["sum_logp"].abs().max())
    print(f"skinny: sum_logp {sk['sum_logp'].tolist()} vs eager {se['sum_logp'].tolist()}: relative {err:.2e} (gate {GATE:g}); "
          f"{int(n_w[0]) - 3} picks")
    assert torch.equal(got, want) and torch.equal(n_g, n_w)                   # the same tokens: the sums are of the same picks
    assert err < GATE


def test_skinny_is_refused_above_sixteen_rows():
    from f5e_tts_amd._C import F5EError
    kv = [(k.expand(17, -1, -1), v.expand(17, -1, -1)) for k, v in kv_gpu(40000)]
    with pytest.raises(F5EError, match="at most 16 rows"):
        model_gpu().generate_from_kv(kv, gold()["prompt"].tolist(), step_graph=True, step_gemm="skinny")


# ---- long-form -------------------------------------------------------------------------------------------------------------------------

def test_transcribe_long_replayed_equals_eager_and_the_fixture():
    c = case("f")                                                             # two rows, four and two windows: B = 2, then B = 1
    eager, replayed = run_long("f"), run_long("f", step_graph=True)
    assert replayed == eager                                                  # dataclass equality: every float bit for bit
    for b in range(2):
        assert len(replayed[b]) >= 2 and len({s.seek for s in replayed[b]}) >= 2
        check_row(c, b, replayed[b])


def test_transcribe_long_with_fallback_and_context_replayed_equals_eager():
    from f5e_tts_amd.eval.whisper import Context, Fallback
    fb = Fallback(temperatures=(0.0, 0.4), logprob_threshold=0.0, seed=3)    # every window falls back to a sampled attempt
    te, tg = [], []
    eager, replayed = run_long("a", fallback=fb, trace=te), run_long("a", fallback=fb, trace=tg, step_graph=True)
    assert replayed == eager and te == tg and any(t["temperature"] > 0 for t in tg)
    ctx = Context(condition_on_prev_tokens=True)
    assert run_long("f", context=ctx, step_graph=True) == run_long("f", context=ctx)
