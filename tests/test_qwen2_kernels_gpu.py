"""The Qwen2 kernels on the GPU (csrc/llm.hip) against the restatement of tests/qwen2_ref.py.

Bounds: the project's 10 sqrt(K) 2^-24 relative L2 against float64 (K = D for RMSNorm, 1 for SwiGLU's element-wise product, dk
for the attention's scores).  Bit-level claims are held with ``torch.equal``: a row against its own 1-row call, the values filed
in the cache, the rotated keys against the restated fp32 rotation, every byte a launch does not own.  The pick is held against
the ``transformers`` fixture (tests/golden/qwen2_sample.npz): survivor sets equal, probabilities within 1e-5, the drawn id equal
to the restatement's wherever u * total lies further than 1e-5 (relative) from a cumulative boundary, which may exclude at most
1 % of the draws."""
import math

import numpy as np
import pytest
import torch

import qwen2_ref as Q

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
EPS24 = 2.0 ** -24


def bound(K):
    return 10.0 * math.sqrt(K) * EPS24


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def rec_of(p, seed=0):
    from f5e_tts_amd import ops
    return ops.whisper_step_record(p, 1, seed, 0.0).cuda()


# ---- RMSNorm, SwiGLU ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", (4, 128, 896, 2048))
def test_rmsnorm_parity_rows_and_containment(D):
    from f5e_tts_amd import ops
    g = torch.Generator().manual_seed(D)
    w = (1.0 + 0.2 * torch.randn(D, generator=g)).cuda()
    for M in (1, 3, 17):
        x = (torch.randn(M, D + 4, generator=g) * 3.0).cuda()[:, :D]
        pad = torch.full((M + 2, D + 8), -7.0).cuda()
        ops.rmsnorm_f32(x, w, 1e-6, out=pad[1:M + 1, :D])
        got = pad[1:M + 1, :D]
        want = Q.rmsnorm(x.cpu().numpy(), w.cpu().numpy(), 1e-6)
        e = rel(got.cpu().numpy(), want)
        print(f"rmsnorm D={D} M={M}: rel L2 {e:.3e} (bound {bound(D):.3e})")
        assert e <= bound(D)
        assert (pad[0] == -7.0).all() and (pad[M + 1] == -7.0).all() and (pad[:, D:] == -7.0).all()
        for m in range(M):                                       # a row equals its own 1-row call
            assert torch.equal(ops.rmsnorm_f32(x[m:m + 1], w, 1e-6), got[m:m + 1])
        y = x.contiguous().clone()                               # in place
        ops.rmsnorm_f32(y, w, 1e-6, out=y)
        assert torch.equal(y, got)


@pytest.mark.parametrize("I", (4, 128, 896, 2048))
def test_swiglu_parity_rows_and_containment(I):
    from f5e_tts_amd import ops
    g = torch.Generator().manual_seed(I + 1)
    for M in (1, 3, 17):
        gu = (torch.randn(M, 2 * I + 4, generator=g) * 4.0).cuda()[:, :2 * I]
        pad = torch.full((M + 2, I + 8), -7.0).cuda()
        ops.swiglu_f32(gu, out=pad[1:M + 1, :I])
        got = pad[1:M + 1, :I]
        e = rel(got.cpu().numpy(), Q.swiglu(gu.cpu().numpy()))
        print(f"swiglu I={I} M={M}: rel L2 {e:.3e} (bound {bound(1):.3e})")
        assert e <= bound(1)
        assert (pad[0] == -7.0).all() and (pad[M + 1] == -7.0).all() and (pad[:, I:] == -7.0).all()
        for m in range(M):
            assert torch.equal(ops.swiglu_f32(gu[m:m + 1]), got[m:m + 1])


def test_embed_widens_exactly_and_clamps():
    from f5e_tts_amd import ops
    g = torch.Generator().manual_seed(3)
    table = torch.randn(50, 24, generator=g)
    ids = torch.tensor([0, 49, 7, 7, -3, 99], dtype=I32).cuda()
    want_ids = torch.tensor([0, 49, 7, 7, 0, 49])
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        emb = table.to(dt).cuda()
        out = torch.full((7, 24), -7.0).cuda()
        ops.llm_embed(ids, emb, out[:6])
        assert torch.equal(out[:6].cpu(), table.to(dt).float()[want_ids]) and (out[6] == -7.0).all()


# ---- attention ---------------------------------------------------------------------------------------------------------------------

SHAPES = ((4, 2, 32), (14, 2, 64), (16, 2, 128), (28, 4, 128), (2, 2, 64))
_tables = {}


def tables(dk, n=4096):
    if dk not in _tables:
        cos, sin = Q.rotary_table(dk, 1e6, n)
        _tables[dk] = (cos, sin, torch.from_numpy(cos).cuda(), torch.from_numpy(sin).cuda())
    return _tables[dk]


def attn_case(H, Hkv, dk, R, U, P, seed, guard=2):
    g = torch.Generator().manual_seed(seed)
    W = (H + 2 * Hkv) * dk
    qkv = torch.randn(R * U, W + 4, generator=g).cuda()[:, :W]
    kc = torch.randn(R, P + guard, Hkv * dk + 4, generator=g).cuda()
    vc = torch.randn(R, P + guard, Hkv * dk + 4, generator=g).cuda()
    return qkv, kc, vc


def run_append(qkv, kc, vc, H, Hkv, dk, U, p0, P, begin):
    from f5e_tts_amd import ops
    cos, sin, cg, sg = tables(dk)
    R = kc.shape[0]
    bt = None if begin is None else torch.tensor(begin, dtype=I32).cuda()
    pad = torch.full((R * U + 1, H * dk + 4), -7.0).cuda()
    ops.gqa_rope_append_f32(qkv, kc[:, :P, :Hkv * dk], vc[:, :P, :Hkv * dk], cg, sg, U, p0, H, Hkv, dk ** -0.5, begin=bt,
                            out=pad[:R * U, :H * dk])
    assert (pad[R * U] == -7.0).all() and (pad[:, H * dk:] == -7.0).all()
    return pad[:R * U, :H * dk]


@pytest.mark.parametrize("H,Hkv,dk", SHAPES)
def test_gqa_rope_append_parity_cache_and_containment(H, Hkv, dk):
    cos, sin, _, _ = tables(dk)
    R, P, Dkv = 3, 80, Hkv * dk
    worst = 0.0
    for U in (1, 15, 16, 17, 40):
        for p0 in (0, 1, 16, 33):
            begin = [0, min(3, p0 + U), p0 + U + 5 if U == 15 else (p0 + U) // 2 + 1]     # ragged; U = 15: a row wholly below begin
            qkv, kc, vc = attn_case(H, Hkv, dk, R, U, P, 1000 * U + p0)
            kc0, vc0 = kc.clone(), vc.clone()
            got = run_append(qkv, kc, vc, H, Hkv, dk, U, p0, P, begin)
            rk, rv = kc0[:, :P, :Dkv].cpu().numpy().copy(), vc0[:, :P, :Dkv].cpu().numpy().copy()
            want = Q.gqa_append(qkv.cpu().numpy(), rk, rv, begin, cos, sin, p0, U, H, Hkv, dk, dk ** -0.5)
            e = rel(got.cpu().numpy(), want)
            worst = max(worst, e)
            assert e <= bound(dk), (U, p0, e)
            # the slots written: V bit for bit, K the restated rotation bit for bit; every other byte of the caches untouched
            assert torch.equal(vc[:, p0:p0 + U, :Dkv].cpu(), torch.from_numpy(rv[:, p0:p0 + U]))
            assert torch.equal(kc[:, p0:p0 + U, :Dkv].cpu(), torch.from_numpy(rk[:, p0:p0 + U]))
            for c, c0 in ((kc, kc0), (vc, vc0)):
                keep = torch.ones_like(c, dtype=torch.bool)
                keep[:, p0:p0 + U, :Dkv] = False
                assert torch.equal(c[keep], c0[keep])
            below = [r for r in range(R) if begin[r] > p0]
            for r in below:                                       # a query below begin[r]: exact zeros
                nz = min(begin[r] - p0, U)
                assert (got[r * U:r * U + nz] == 0).all()
            if U == 17 and p0 == 16:                              # a row equals its own R = 1 call
                for r in range(R):
                    one = run_append(qkv[r * U:(r + 1) * U], kc0[r:r + 1].clone(), vc0[r:r + 1].clone(), H, Hkv, dk, U, p0, P,
                                     [begin[r]])
                    assert torch.equal(one, got[r * U:(r + 1) * U])
    print(f"gqa_rope_append H={H} Hkv={Hkv} dk={dk}: worst rel L2 {worst:.3e} (bound {bound(dk):.3e})")


@pytest.mark.parametrize("H,Hkv,dk", SHAPES)
def test_gqa_rope_prefill_then_append_equals_one_longer_prefill(H, Hkv, dk):
    R, P, U1, U2 = 2, 64, 21, 19
    begin = [0, 6]
    qkv, kc, vc = attn_case(H, Hkv, dk, R, U1 + U2, P, 77)
    q3 = qkv.view(R, U1 + U2, -1)
    whole = run_append(qkv, kc.clone(), vc.clone(), H, Hkv, dk, U1 + U2, 0, P, begin).view(R, U1 + U2, -1)
    run_append(q3[:, :U1].reshape(R * U1, -1), kc, vc, H, Hkv, dk, U1, 0, P, begin)
    second = run_append(q3[:, U1:].reshape(R * U2, -1), kc, vc, H, Hkv, dk, U2, U1, P, begin).view(R, U2, -1)
    e = rel(second.cpu().numpy(), whole[:, U1:].cpu().numpy())
    print(f"prefill + append vs one prefill, dk={dk}: rel L2 {e:.3e}")
    assert e <= bound(dk)


@pytest.mark.parametrize("H,Hkv,dk", SHAPES)
def test_gqa_rope_decode_dev_equals_append_rows_and_clamp(H, Hkv, dk):
    from f5e_tts_amd import ops
    _, _, cg, sg = tables(dk)
    P, Dkv = 4096, Hkv * dk
    worst = 0.0
    for R in (1, 3):
        qkv, kc, vc = attn_case(H, Hkv, dk, R, 1, P, 5 + R)
        for p in (0, 1, 15, 16, 63, 64, 1000, 4095):
            begin = [0, min(p, 7), p][:R]
            bt = torch.tensor(begin, dtype=I32).cuda()
            k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
            rec = rec_of(p)
            got = ops.gqa_rope_decode_dev_f32(qkv, k1[:, :P, :Dkv], v1[:, :P, :Dkv], cg, sg, rec, H, Hkv, dk ** -0.5, begin=bt)
            want = run_append(qkv, k2, v2, H, Hkv, dk, 1, p, P, begin)
            assert int(rec[0]) == p
            e = rel(got.cpu().numpy(), want.cpu().numpy())
            worst = max(worst, e)
            assert e <= bound(dk), (R, p, e)
            assert torch.equal(k1, k2) and torch.equal(v1, v2)    # slot p as append files it, every other byte untouched
            if R == 3:
                for r in range(R):
                    ka, va = kc[r:r + 1].clone(), vc[r:r + 1].clone()
                    one = ops.gqa_rope_decode_dev_f32(qkv[r:r + 1], ka[:, :P, :Dkv], va[:, :P, :Dkv], cg, sg, rec, H, Hkv, dk ** -0.5,
                                                      begin=bt[r:r + 1].clone())
                    assert torch.equal(one, got[r:r + 1])
        # a record outside the caches is clamped: nothing outside slot P - 1 (resp. 0) is written
        for rec_p, p in ((P + 5, P - 1), (2 ** 31 - 1, P - 1), (-4, 0)):
            k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
            got = ops.gqa_rope_decode_dev_f32(qkv, k1[:, :P, :Dkv], v1[:, :P, :Dkv], cg, sg, rec_of(rec_p), H, Hkv, dk ** -0.5)
            want = ops.gqa_rope_decode_dev_f32(qkv, k2[:, :P, :Dkv], v2[:, :P, :Dkv], cg, sg, rec_of(p), H, Hkv, dk ** -0.5)
            assert torch.equal(got, want) and torch.equal(k1, k2) and torch.equal(v1, v2)
            keep = torch.ones_like(kc, dtype=torch.bool)
            keep[:, p, :Dkv] = False
            assert torch.equal(k1[keep], kc[keep]) and torch.equal(v1[keep], vc[keep])
    print(f"gqa_rope_decode_dev H={H} Hkv={Hkv} dk={dk}: worst rel L2 vs append {worst:.3e} (bound {bound(dk):.3e})")


def test_attention_refusals():
    from f5e_tts_amd import ops
    from f5e_tts_amd._C import F5EError
    _, _, cg, sg = tables(32)
    for H, Hkv, dk, match in ((18, 2, 32, "more than 8"), (2, 2, 16, "head dim 16")):
        qkv, kc, vc = attn_case(H, Hkv, dk, 1, 1, 8, 0)
        c = torch.zeros(4096, dk // 2).cuda()
        with pytest.raises(F5EError, match=match):
            ops.gqa_rope_append_f32(qkv, kc[:, :8, :Hkv * dk], vc[:, :8, :Hkv * dk], c, c, 1, 0, H, Hkv, 1.0)
        with pytest.raises(F5EError, match=match):
            ops.gqa_rope_decode_dev_f32(qkv, kc[:, :8, :Hkv * dk], vc[:, :8, :Hkv * dk], c, c, rec_of(0), H, Hkv, 1.0)


# ---- the pick ----------------------------------------------------------------------------------------------------------------------

_sample = {}


def sample_fixture():
    import os
    if not _sample:
        _sample.update(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qwen2_sample.npz")))
    return _sample


def pick_inputs(V):
    fx = sample_fixture()
    rows, hist = fx[f"rows_{V}"], fx[f"hist_{V}"]
    x = np.stack([Q.logits_row(V, int(k)) for k in rows])
    return x, hist


def run_pick(x, hist, p_extra=0, seed=0, **kw):
    """The rows' histories stand in columns begin .. p of a table with guard columns; -> (tokens, last, done, alive, rec, keeps)."""
    from f5e_tts_amd import ops
    R, V = x.shape
    n = hist.shape[1]
    begin = np.arange(R) % 3
    width = n + 3 + p_extra + 4
    table = np.full((R, width), -9, np.int32)
    p = n + 2 + p_extra
    for r in range(R):
        table[r, begin[r]:p + 1] = np.resize(hist[r], p + 1 - begin[r])      # the history, repeated: the same set of classes
        table[r, :begin[r]] = int(np.argsort(-x[r].astype(np.float64), kind="stable")[4])   # padding: a class that must not count
    tokens = torch.from_numpy(table).cuda()
    logits = torch.from_numpy(np.concatenate([x, np.full((R, 3), 50.0, np.float32)], 1)).cuda()[:, :V]
    last, done, alive = torch.zeros(R, dtype=I32).cuda(), torch.zeros(R, dtype=I32).cuda(), torch.zeros(1, dtype=I32).cuda()
    keep_id = torch.full((R, 64), -5, dtype=I32).cuda()
    keep_p = torch.full((R, 64), -5.0).cuda()
    keep_n = torch.zeros(R, dtype=I32).cuda()
    rec = rec_of(p, seed)
    rec0 = rec.clone()
    row_key, serial = torch.arange(R, dtype=I32).cuda(), (torch.arange(R, dtype=I32) * 3 + 1).cuda()
    lg0 = logits.clone()
    ops.llm_pick_dev(logits, tokens[:, :p + 2], last, done, alive, rec, begin=torch.from_numpy(begin.astype(np.int32)).cuda(),
                     row_key=row_key, serial=serial, keep_id=keep_id, keep_p=keep_p, keep_n=keep_n, **kw)
    assert int(rec[0]) == p + 1 and torch.equal(rec[1:], rec0[1:])          # the position advances by exactly one
    assert torch.equal(logits, lg0)
    t = tokens.cpu().numpy()
    untouched = np.ones_like(table, dtype=bool)
    untouched[:, p + 1] = False
    assert np.array_equal(t[untouched], table[untouched])
    assert torch.equal(tokens[:, p + 1], last)
    return t[:, p + 1], done.cpu().numpy(), int(alive), p, keep_id.cpu().numpy(), keep_p.cpu().numpy(), keep_n.cpu().numpy()


@pytest.mark.parametrize("V", (384, 151936))
def test_llm_pick_survivors_probabilities_and_greedy(V):
    fx = sample_fixture()
    x, hist = pick_inputs(V)
    for si, (pen, T, k, tp) in enumerate(fx["settings"]):
        _, _, _, _, kid, kp, kn = run_pick(x, hist, eos=[], pad=0, do_sample=True, penalty=pen, temperature=T, top_k=int(k), top_p=tp)
        want_id, want_p = fx[f"keep_id_{V}_{si}"], fx[f"keep_p_{V}_{si}"]
        worst = 0.0
        for r in range(x.shape[0]):
            n = int((want_id[r] >= 0).sum())
            assert kn[r] == n and np.array_equal(kid[r, :n], want_id[r, :n]), (si, r)
            assert (kid[r, n:] == -5).all() and (kp[r, n:] == -5.0).all()
            worst = max(worst, float(np.abs(kp[r, :n] - want_p[r, :n]).max()))
        print(f"llm_pick V={V} setting {si}: survivors equal, max |p - fixture| {worst:.2e}")
        assert worst <= 1e-5
        got, _, _, _, kid, _, kn = run_pick(x, hist, eos=[], pad=0, do_sample=False, penalty=pen)
        want = [int(np.argmax(Q.penalise(x[r], hist[r], pen))) for r in range(x.shape[0])]
        assert got.tolist() == want and (kn == 1).all() and kid[:, 0].tolist() == want
    # the fixture's own greedy pick: the first survivor of the top_k = 1 setting
    got, *_ = run_pick(x, hist, eos=[], pad=0, do_sample=False, penalty=1.3)
    assert got.tolist() == fx[f"keep_id_{V}_3"][:, 0].tolist()


@pytest.mark.parametrize("V", (384, 151936))
def test_llm_pick_draw_equals_the_restatement(V):
    fx = sample_fixture()
    x, hist = pick_inputs(V)
    R = x.shape[0]
    total = excluded = 0
    for si in (0, 1, 2):
        pen, T, k, tp = fx["settings"][si]
        surv = [Q.survivors(x[r], hist[r], pen, T, int(k), tp) for r in range(R)]
        for seed, extra in ((0, 0), (12345, 1), (2 ** 40 + 17, 2), (2 ** 63 + 5, 3)):
            got, _, _, p, *_ = run_pick(x, hist, p_extra=extra, seed=seed, eos=[], pad=0, do_sample=True, penalty=pen, temperature=T,
                                        top_k=int(k), top_p=tp)
            for r in range(R):
                ids, e = surv[r]
                pick, margin = Q.draw(e, Q.draw_u(seed, r, 3 * r + 1, p))
                total += 1
                if margin <= 1e-5:
                    excluded += 1
                    continue
                assert got[r] == ids[pick], (si, seed, r)
    print(f"llm_pick draws V={V}: {total} compared, {excluded} excluded near a boundary")
    assert excluded <= 0.01 * total


def test_llm_pick_eos_pad_done_alive():
    x, hist = pick_inputs(384)
    x = x[:6].copy()
    hist = hist[:6]
    want = [int(np.argmax(Q.penalise(x[r], hist[r], 1.05))) for r in range(6)]
    eos = [want[1], want[4]]                                      # two eos ids: rows 1 and 4 close
    got, done, alive, *_ = run_pick(x, hist, eos=eos, pad=3, do_sample=False, penalty=1.05)
    assert got.tolist() == want
    assert done.tolist() == [1 if w in eos else 0 for w in want] and alive == 6 - sum(done.tolist())
    # a done row writes the pad id and stays done
    from f5e_tts_amd import ops
    logits = torch.from_numpy(x).cuda()
    tokens = torch.zeros(6, 8, dtype=I32).cuda()
    last, alive_t = torch.zeros(6, dtype=I32).cuda(), torch.zeros(1, dtype=I32).cuda()
    done_t = torch.tensor([0, 1, 0, 0, 1, 0], dtype=I32).cuda()
    rec = rec_of(2)
    ops.llm_pick_dev(logits, tokens, last, done_t, alive_t, rec, eos=eos, pad=3)
    raw = [int(np.argmax(x[r])) for r in range(6)]                # the history is class 0 at penalty 1: nothing changes
    want_done = [1 if r in (1, 4) or raw[r] in eos else 0 for r in range(6)]
    assert tokens[:, 3].tolist() == [3 if r in (1, 4) else raw[r] for r in range(6)] and torch.equal(last, tokens[:, 3])
    assert done_t.tolist() == want_done and int(alive_t) == 6 - sum(want_done) and int(rec[0]) == 3
