"""The attention decoder's beam search on the GPU (csrc/attn_decode.hip through ops.attn_decode_f32 / ops.beam_step,
``ConformerEngine.decode_step`` and ``ConformerPPG.recognize``) against
  * the REFERENCE's own ``recognize`` outputs (tests/golden/asr_attention.npz; the generator asserts that no stored decision is
    fragile), and
  * the restatement (tests/asr_attention_ref.py, pinned by the same fixture).
Beams are discrete: they are compared exactly, and only on cases that satisfy the margin rule of asr_attention_ref (the
smallest decisive gap is at least 100 x the fp32 / fp64 score difference), which every test asserts as a condition on the
very numbers it hands to the device."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import asr_attention_ref as AR

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
I32, F32 = torch.int32, torch.float32
SENT = -7


@pytest.fixture(scope="module")
def ops():
    import f5e_tts_amd.ops as ops_mod
    ops_mod.require_device()
    return ops_mod


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "asr_attention.npz"))


def dev_state(B, beam, width, sos):
    """The start state on the device, output tables sentinel-filled: a SimpleNamespace in the layout of ``decode_state``."""
    R = B * beam
    S = SimpleNamespace(B=B, beam=beam, R=R, p=0, umax=width - 1,
                        hyp=[torch.full((R, width), SENT, dtype=I32).cuda() for _ in range(2)],
                        anc=[torch.full((R, width), SENT, dtype=I32).cuda() for _ in range(2)],
                        score=torch.tensor([0.0] + [-float("inf")] * (beam - 1)).repeat(B).cuda(),
                        last=torch.full((R,), sos, dtype=I32).cuda(), alive=torch.full((B,), SENT, dtype=I32).cuda(),
                        done_at=torch.full((B,), -1, dtype=I32).cuda())
    S.hyp[0][:, 0] = sos
    return S


# ------------------------------------------------------------------ 1. f5e_beam_step

@pytest.mark.parametrize("case", range(len(AR.LOOP_CASES)))
def test_beam_step_follows_the_restatement_on_every_loop_case(ops, gold, case):
    B, maxlen, V, beam, plant = AR.LOOP_CASES[case]
    table = AR.loop_table(maxlen, V, int(gold[f"loop{case}_seed"]), plant)
    eos = V - 1
    # every step, also those the reference's early stop would skip: the margin rule is a condition on all of them
    ref, delta, E, same = AR.margin(lambda dt: AR.table_fn(table.astype(dt)), B, beam, maxlen, eos, eos, early_stop=False)
    print(f"loop {case}: delta {delta:.3e}, E {E:.3e}")
    assert same and AR.usable(delta, E)
    S = dev_state(B, beam, maxlen + 1, eos)
    ld = V + 3                                                     # ld > V; the pad columns hold huge values
    tab = torch.full((maxlen, V, ld), 1e30).cuda()
    tab[:, :, :V] = torch.from_numpy(table).cuda()
    for p in range(maxlen):
        cur, nxt = p & 1, (p & 1) ^ 1
        S.hyp[nxt].fill_(SENT), S.anc[nxt].fill_(SENT)
        before = S.hyp[cur].clone(), S.anc[cur].clone()
        logits = tab[p][S.last.long()][:, :V]                      # a view: the row stride stays ld
        ops.beam_step(logits, S.score, S.hyp[cur], S.anc[cur], S.hyp[nxt], S.anc[nxt], S.last, S.alive, S.done_at, p, beam, eos)
        score, hyp, anc, alive, done_at = ref["trace"][p]
        assert np.array_equal(S.hyp[nxt][:, :p + 2].cpu().numpy(), hyp), f"step {p}: hypotheses"
        assert np.array_equal(S.anc[nxt][:, :p + 1].cpu().numpy(), anc), f"step {p}: ancestry"
        assert np.array_equal(S.last.cpu().numpy(), hyp[:, p + 1])
        assert np.array_equal(S.alive.cpu().numpy(), alive) and np.array_equal(S.done_at.cpu().numpy(), done_at), f"step {p}"
        got = S.score.cpu().numpy().astype(np.float64)
        fin = np.isfinite(score)
        assert np.array_equal(np.isfinite(got), fin)
        assert np.abs(got[fin] - score[fin]).max() <= 10 * max(E, 1e-6 * (p + 1)), f"step {p}: scores"
        # containment: the columns behind the step and the input tables
        assert bool((S.hyp[nxt][:, p + 2:] == SENT).all()) and bool((S.anc[nxt][:, p + 1:] == SENT).all())
        assert torch.equal(S.hyp[cur], before[0]) and torch.equal(S.anc[cur], before[1])
    if plant == "early":
        assert int(S.done_at.max()) + 1 == gold[f"loop{case}_best"].shape[1] < maxlen // 2
    if plant == "never":
        assert bool((S.done_at < 0).all())


@pytest.mark.parametrize("beam", [1, 4, 10, 16])
@pytest.mark.parametrize("V", ["beam", 63, 64, 65, 5000])
def test_beam_step_class_count_and_beam_edges(ops, beam, V):
    """One step at p = 3 from a random state with finished rows, guard rows around every table, a row stride > V."""
    V = beam if V == "beam" else V
    B, p, ld, eos = 3, 3, 8, V - 1
    R = B * beam
    for seed in range(100):                                        # a seeded state whose decisions are not fragile
        rng = np.random.default_rng(1000 * beam + V + 7919 * seed)
        logits = (4.0 * rng.standard_normal((R, V))).astype(np.float32)
        hyp = np.full((R, ld), SENT, np.int64)
        hyp[:, 0], hyp[:, 1:p + 1] = eos, rng.integers(0, V, size=(R, p))
        hyp[rng.random(R) < 0.3, p] = eos                          # finished rows
        anc = np.full((R, ld), SENT, np.int64)
        anc[:, :p] = (np.arange(R) // beam * beam)[:, None] + rng.integers(0, beam, size=(R, p))
        score = -np.sort(rng.random((B, beam)) * 8.0, axis=1).reshape(R).astype(np.float32)
        x = logits.astype(np.float64)
        logp = x - x.max(1, keepdims=True)
        logp = logp - np.log(np.exp(logp).sum(1, keepdims=True))
        w_score, w_hyp, w_anc, w_alive, gaps = AR.beam_step(logp, score.astype(np.float64), hyp, anc, p, beam, eos)
        if min(gaps + [np.inf]) >= 100 * 1e-5:                    # fp32 log-softmax + one add at |score| < 32: E <= 1e-5
            break
    else:
        raise AssertionError("no seed gives a state with clear decisions")
    pad = 5
    dl = torch.full((R, V + pad), 1e30).cuda()
    dl[:, :V] = torch.from_numpy(logits).cuda()
    tabs = {n: torch.full((R + 2, ld), SENT, dtype=I32).cuda() for n in ("hyp_in", "anc_in", "hyp_out", "anc_out")}
    tabs["hyp_in"][1:-1], tabs["anc_in"][1:-1] = torch.from_numpy(hyp).int().cuda(), torch.from_numpy(anc).int().cuda()
    sc = torch.full((R + 2,), 123.0).cuda()
    sc[1:-1] = torch.from_numpy(score).cuda()
    last, alive, done_at = torch.full((R + 2,), SENT, dtype=I32).cuda(), torch.full((B + 2,), SENT, dtype=I32).cuda(), \
        torch.full((B + 2,), -1, dtype=I32).cuda()
    ops.beam_step(dl[:, :V], sc[1:-1], tabs["hyp_in"][1:-1], tabs["anc_in"][1:-1], tabs["hyp_out"][1:-1], tabs["anc_out"][1:-1],
                  last[1:-1], alive[1:-1], done_at[1:-1], p, beam, eos)
    assert np.array_equal(tabs["hyp_out"][1:-1, :p + 2].cpu().numpy(), w_hyp[:, :p + 2])
    assert np.array_equal(tabs["anc_out"][1:-1, :p + 1].cpu().numpy(), w_anc[:, :p + 1])
    assert np.array_equal(last[1:-1].cpu().numpy(), w_hyp[:, p + 1]) and np.array_equal(alive[1:-1].cpu().numpy(), w_alive)
    assert np.array_equal(done_at[1:-1].cpu().numpy(), np.where(w_alive == 0, p, -1))
    assert np.abs(sc[1:-1].cpu().numpy().astype(np.float64) - w_score).max() <= 10 * 1e-5
    for n in ("hyp_out", "anc_out"):
        t = tabs[n]
        assert bool((t[0] == SENT).all()) and bool((t[-1] == SENT).all())
        assert bool((t[:, (p + 2 if n == "hyp_out" else p + 1):] == SENT).all())
    assert np.array_equal(tabs["hyp_in"][1:-1].cpu().numpy(), hyp) and np.array_equal(tabs["anc_in"][1:-1].cpu().numpy(), anc)
    assert float(sc[0]) == 123.0 == float(sc[-1]) and int(last[0]) == SENT == int(last[-1])
    assert int(alive[0]) == SENT == int(alive[-1]) and int(done_at[0]) == -1 == int(done_at[-1])


def test_beam_step_refuses_bad_arguments(ops):
    from f5e_tts_amd._C import F5EError
    S = dev_state(1, 4, 6, 3)
    lg = torch.zeros(4, 9).cuda()
    args = (S.score, S.hyp[0], S.anc[0], S.hyp[1], S.anc[1], S.last, S.alive, S.done_at)
    with pytest.raises(F5EError):
        ops.beam_step(lg, *args, 0, 17, 3)                         # beam > 16
    with pytest.raises(F5EError):
        ops.beam_step(lg[:, :3], *args, 0, 4, 2)                   # beam > V
    with pytest.raises(F5EError):
        ops.beam_step(lg, *args, 5, 4, 3)                          # p + 2 > ld
    with pytest.raises(F5EError):
        ops.beam_step(lg, S.score, S.hyp[0], S.anc[0], S.hyp[0], S.anc[1], S.last, S.alive, S.done_at, 0, 4, 3)


# ------------------------------------------------------------------ 2. f5e_attn_decode_f32

@pytest.mark.parametrize("R", [1, 10, 33])
@pytest.mark.parametrize("dk", [16, 64])
def test_attn_decode_equals_dense_attention_on_gathered_keys(ops, dk, R):
    H, Umax, padc = 4, 132, 4
    D = H * dk
    g = torch.Generator().manual_seed(100 * dk + R)
    scale = 1.0 / math.sqrt(dk)
    for p in (0, 1, 15, 16, 63, 64, 65, 130):
        for with_anc in (True, False):
            kc_full, vc_full = torch.randn(R, Umax, D + padc, generator=g).cuda(), torch.randn(R, Umax, D + padc, generator=g).cuda()
            kc, vc = kc_full[:, :, :D], vc_full[:, :, :D]                      # padded position stride
            qkv_full = torch.randn(R, 3 * D + 4, generator=g).cuda()
            qkv = qkv_full[:, :3 * D]                                          # padded row stride
            anc_h = torch.randint(0, R, (R, Umax), generator=g)
            anc = anc_h.int().cuda() if with_anc else None
            k0, v0 = kc_full.clone(), vc_full.clone()
            out = ops.attn_decode_f32(qkv, kc, vc, p, H, scale, anc=anc)
            # dense fp64 attention on the gathered keys
            src = anc_h[:, :p] if with_anc else torch.arange(R)[:, None].expand(-1, p)
            q, kn, vn = (qkv_full[:, i * D:(i + 1) * D].cpu().double() for i in range(3))
            pos = torch.arange(p)[None, :]
            K = torch.cat((k0[:, :, :D].cpu().double()[src, pos], kn[:, None]), 1).view(R, p + 1, H, dk).transpose(1, 2)
            Vv = torch.cat((v0[:, :, :D].cpu().double()[src, pos], vn[:, None]), 1).view(R, p + 1, H, dk).transpose(1, 2)
            a = torch.softmax((q.view(R, H, 1, dk) @ K.transpose(-2, -1)) * scale, -1)
            want = (a @ Vv).transpose(1, 2).reshape(R, D)
            err = float((out.cpu().double() - want).norm() / want.norm())
            assert err < 2e-4, f"p={p} anc={with_anc}: rel L2 {err:.2e}"
            # only slot [r][p] changed, and it holds the new k / v exactly
            k0[:, p, :D], v0[:, p, :D] = qkv_full[:, D:2 * D], qkv_full[:, 2 * D:3 * D]
            assert torch.equal(kc_full, k0) and torch.equal(vc_full, v0), f"p={p} anc={with_anc}: cache containment"


def test_attn_decode_refuses_bad_arguments(ops):
    from f5e_tts_amd._C import F5EError
    kc, vc, qkv = torch.zeros(2, 8, 64).cuda(), torch.zeros(2, 8, 64).cuda(), torch.zeros(2, 192).cuda()
    with pytest.raises(F5EError):
        ops.attn_decode_f32(qkv, kc, vc, 8, 4, 1.0)                # p == Umax
    with pytest.raises(F5EError):
        ops.attn_decode_f32(qkv, kc, vc, 0, 16, 1.0)               # head dim 4
    with pytest.raises(F5EError):
        ops.attn_decode_f32(qkv[:, :100], kc, vc, 0, 4, 1.0)       # qkv narrower than 3 D
    with pytest.raises(F5EError):
        ops.attn_decode_f32(qkv, kc, vc, 3, 4, 1.0, anc=torch.zeros(2, 2, dtype=I32).cuda())      # fewer than p columns


# ------------------------------------------------------------------ 3. / 4. the cached step and the whole search

KINDS = {"tf": ("transformer", dict(attention_heads=4, linear_units=64, num_blocks=2), "decoder."),
         "bi": ("bitransformer", dict(attention_heads=4, linear_units=64, num_blocks=3, r_num_blocks=1), "decoder.left_decoder.")}


def build_asr(tag, gold):
    from f5e_tts_amd.ppg.ppg_model import ConformerPPG
    base = np.load(os.path.join(GOLD, "ppg_conformer.npz"))
    sd = {k[2:]: torch.from_numpy(base[k]) for k in base.files if k.startswith("w/encoder.")}
    pre = f"{tag}/w/"
    sd.update({k[len(pre):]: torch.from_numpy(gold[k].astype(np.float32)) for k in gold.files if k.startswith(pre)})
    kind, conf, _ = KINDS[tag]
    m = ConformerPPG(80, 40, 64, 4, 128, 2, 15, global_cmvn=(sd["encoder.global_cmvn.mean"], sd["encoder.global_cmvn.istd"]),
                     ctc=True, decoder=kind, decoder_conf=conf)
    full = m.state_dict()
    assert set(sd) <= set(full) and any(k.startswith("decoder.") for k in sd)
    full.update(sd)
    m.load_state_dict(full)
    return m.cuda().eval(), sd


@pytest.fixture(scope="module", params=["tf", "bi"])
def asr(request, gold, ops):
    """(tag, model, state dict, features, lengths, the device's encoder output and frame counts, and -- measured once -- the
    worst relative L2 and log-probability difference between a cached step and the full decoder)."""
    tag = request.param
    m, sd = build_asr(tag, gold)
    feats, lens = torch.from_numpy(gold[f"{tag}/feats"]).cuda(), torch.from_numpy(gold[f"{tag}/lens"]).cuda()
    eng = m.engine()
    enc, len2 = eng.encode(feats, lens)
    beam, eos = 10, m.eos
    S = eng.decode_state("left", enc, len2, beam, m.sos, eos)
    worst_rel = worst_lp = 0.0
    for p in range(S.umax):
        prefix = S.hyp[p & 1][:, :p + 1].contiguous()
        step = eng.decode_step(S, reorder_cache=True).clone()
        full = eng.decode("left", enc, len2, prefix, torch.full((S.R,), p + 1, dtype=I32).cuda(), beam).view(S.R, p + 1, -1)[:, -1]
        worst_rel = max(worst_rel, float((step - full).norm() / full.norm()))
        worst_lp = max(worst_lp, float((torch.log_softmax(step.double(), -1) - torch.log_softmax(full.double(), -1)).abs().max()))
    print(f"{tag}: cached step vs full decoder over {S.umax} steps: worst rel L2 {worst_rel:.3e}, worst |d logp| {worst_lp:.3e}")
    return SimpleNamespace(tag=tag, m=m, sd=sd, feats=feats, lens=lens, enc=enc.cpu().numpy(), len2=len2.cpu().numpy(),
                           worst_rel=worst_rel, worst_lp=worst_lp)


def test_one_cached_step_is_the_full_decoder(asr):
    assert asr.worst_rel < 2e-4, f"{asr.tag}: rel L2 {asr.worst_rel:.3e}"


def restate(asr, rows, beam, reorder):
    """The restatement on the DEVICE's own encoder output (utterances ``rows``): the margin rule is a condition on it."""
    pre = KINDS[asr.tag][2]
    enc, n = asr.enc[rows], asr.len2[rows]
    mem_len = None if int(n.min()) == enc.shape[1] else n
    eos = asr.m.eos
    r, delta, E, same = AR.margin(AR.model_fn(asr.sd, pre, enc, mem_len, 4, beam, enc.shape[1], reorder), len(rows), beam,
                                  enc.shape[1], eos, eos)
    print(f"{asr.tag} rows {rows} beam {beam} reorder {reorder}: delta {delta:.3e}, E {E:.3e}, steps {r['steps']}")
    assert same and AR.usable(delta, E), f"the device's encoder output misses the margin rule: delta {delta:.3e}, E {E:.3e}"
    return r


@pytest.mark.parametrize("beam", [10, 4])
def test_recognize_equals_the_reference(asr, gold, beam):
    m, tag = asr.m, asr.tag
    r = restate(asr, [0, 1], beam, False)
    tol = 2 * r["steps"] * max(asr.worst_lp, 1e-6)
    hyps, scores = m.recognize(asr.feats, asr.lens, beam)
    assert hyps.dtype == torch.int64 and scores.dtype == F32 and hyps.is_cuda and scores.is_cuda
    want, want_s = gold[f"{tag}/b{beam}/best"], gold[f"{tag}/b{beam}/best_score"]
    assert hyps.shape == want.shape and np.array_equal(hyps.cpu().numpy(), want)
    assert np.abs(scores.cpu().numpy() - want_s).max() <= tol
    # the whole beam, both cache modes: the restatement's (on the device's encoder output) and the stored one
    for reorder, name in ((False, "stale"), (True, "reorder")):
        rr = r if not reorder else restate(asr, [0, 1], beam, True)
        nb, nb_s = m.recognize(asr.feats, asr.lens, beam, reorder_cache=reorder, nbest=True)
        assert nb.shape == (2, beam, rr["steps"]) and np.array_equal(nb.cpu().numpy().reshape(2 * beam, -1), rr["hyp"][:, 1:])
        assert np.array_equal(rr["hyp"], gold[f"{tag}/b{beam}/{name}_hyp"])
        assert np.abs(nb_s.cpu().numpy().reshape(-1) - rr["score"]).max() <= 2 * rr["steps"] * max(asr.worst_lp, 1e-6)
        # the result does not depend on how often the host looks
        a, a_s = m.recognize(asr.feats, asr.lens, beam, reorder_cache=reorder, nbest=True, sync_every=1)
        b, b_s = m.recognize(asr.feats, asr.lens, beam, reorder_cache=reorder, nbest=True, sync_every=5)
        assert torch.equal(a, nb) and torch.equal(b, nb) and torch.equal(a_s, nb_s) and torch.equal(b_s, nb_s)
    # each utterance alone
    for j, n in enumerate(asr.lens.tolist()):
        f_, l_ = asr.feats[j:j + 1, :n], asr.lens[j:j + 1]
        enc_j, len_j = m.engine().encode(f_, l_)
        solo = SimpleNamespace(**{**vars(asr), "enc": enc_j.cpu().numpy(), "len2": len_j.cpu().numpy()})
        rj = restate(solo, [0], beam, False)
        hj, sj = m.recognize(f_, l_, beam)
        want, want_s = gold[f"{tag}/b{beam}/u{j}_best"], gold[f"{tag}/b{beam}/u{j}_best_score"]
        assert hj.shape == want.shape and np.array_equal(hj.cpu().numpy(), want)
        assert np.abs(sj.cpu().numpy() - want_s).max() <= 2 * rj["steps"] * max(asr.worst_lp, 1e-6)


def test_the_flag_is_observable_and_rows_finish_at_different_steps(gold):
    differ = ragged = False
    for tag in KINDS:
        for beam in (10, 4):
            s, r = gold[f"{tag}/b{beam}/stale_hyp"], gold[f"{tag}/b{beam}/reorder_hyp"]
            differ |= s.shape != r.shape or not np.array_equal(s[::beam], r[::beam])
            ends = {int((row[1:] == 39).argmax()) for row in s if (row[1:] == 39).any()}
            ragged |= len(ends) > 1
    assert differ and ragged


@pytest.mark.parametrize("sync_every", [1, 4, 7])
def test_an_early_finish_gives_the_stored_width(ops, gold, sync_every):
    """The loop control of the engine (ppg_model.beam_loop) around a table-driven step: the loop case in which every row
    finishes well before maxlen returns the reference's width, whatever the number of steps run beyond it."""
    from f5e_tts_amd.ppg.ppg_model import beam_loop
    case = next(i for i, c in enumerate(AR.LOOP_CASES) if c[4] == "early")
    B, maxlen, V, beam, plant = AR.LOOP_CASES[case]
    tab = torch.from_numpy(AR.loop_table(maxlen, V, int(gold[f"loop{case}_seed"]), plant)).cuda()
    S = dev_state(B, beam, maxlen + 1, V - 1)
    for t in S.hyp:
        t[:, 1:] = V - 1

    def step(S):
        p = S.p
        ops.beam_step(tab[p][S.last.long()], S.score, S.hyp[p & 1], S.anc[p & 1], S.hyp[(p & 1) ^ 1], S.anc[(p & 1) ^ 1], S.last,
                      S.alive, S.done_at, p, beam, V - 1)
        S.p = p + 1
    hyps, scores = beam_loop(S, step, sync_every)
    want, want_s = gold[f"loop{case}_best"], gold[f"loop{case}_best_score"]
    assert hyps.shape == (B, beam, want.shape[1]) and want.shape[1] < maxlen // 2
    best = scores.argmax(1)
    assert np.array_equal(hyps[torch.arange(B).cuda(), best].cpu().numpy(), want)
    assert np.abs(scores.max(1).values.cpu().numpy() - want_s).max() <= 10 * max(float(gold[f"loop{case}_E"]), 1e-6 * maxlen)
    assert np.array_equal(hyps.cpu().numpy().reshape(B * beam, -1), gold[f"loop{case}_hyp"][:, 1:])


def test_recognize_refuses_bad_arguments(asr):
    from f5e_tts_amd._C import F5EError
    for bad in (0, 17, 41):
        with pytest.raises(F5EError):
            asr.m.recognize(asr.feats, asr.lens, bad)
    with pytest.raises(F5EError):
        asr.m.recognize(asr.feats, asr.lens, 4, sync_every=0)


# ------------------------------------------------------------------ 5. the aligner

def test_aligner_recognize_returns_a_string_and_transcribe_keeps_its_modes(asr):
    from f5e_tts_amd._C import F5EError
    from f5e_tts_amd.ppg.ctc_align import CTCAligner
    table = {"<blank>": 0, **{chr(96 + i): i for i in range(1, 27)}, **{f"<{i}>": i for i in range(27, 39)}, "<sos/eos>": 39}
    al = CTCAligner(model=asr.m, symbol_table=table, device="cuda")
    wav = 0.1 * torch.randn(1, 8000, generator=torch.Generator().manual_seed(3))
    for reorder in (False, True):
        text = al.recognize(wav, 16000, beam_size=4, reorder_cache=reorder)
        assert isinstance(text, str) and "<sos/eos>" not in text
    with pytest.raises(F5EError, match="unknown mode"):
        al.transcribe(wav, 16000, mode="attention")
