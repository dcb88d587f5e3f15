"""The kernels of Whisper's decoder prefill (csrc/whisper_prefill.hip, and the FROM instantiation of attn_decode_kernel) through
ops.attn_prefill_f32 / ops.attn_decode_f32(begin=) / ops.whisper_embed, against float64 NumPy / torch on the same fp32 operands.

Gates (none invented here):
  * f5e_attn_prefill_f32: relative L2 < 1e-5, the gate of f5e_mha_f32's own parity test (tests/test_ctc_beam_gpu.py,
    test_mha_equals_dense_attention_...): the same wave tile and arithmetic.  tests/test_asr_attention_gpu.py gates the cached
    step at 2e-4; the stricter of the two is used.  Measured on an MI355X: 1.1e-7 .. 1.6e-7 over all cases.
  * f5e_attn_decode_from_f32: relative L2 < 2e-4, the gate of f5e_attn_decode_f32 (tests/test_asr_attention_gpu.py), and
    bit-equal to it with ``begin`` null or all zeros.
  * f5e_whisper_embed: exact (one fp32 add per element, the one NumPy makes).
Cache slots are compared bit for bit, everything a launch must not write by equality with a copy taken before it."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

I32, F32 = torch.int32, torch.float32
GUARD = -7.0


@pytest.fixture(scope="module")
def ops():
    import f5e_tts_amd.ops as ops_mod
    ops_mod.require_device()
    return ops_mod


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def dense_prefill(qkv, R, U, H, dk, begin, scale):
    """fp64: qkv [R * U, 3 D] -> [R * U, D]; query i of row r sees keys begin[r] .. i, a query below begin[r] gives zeros."""
    D = H * dk
    q, k, v = (qkv[:, i * D:(i + 1) * D].double().view(R, U, H, dk).transpose(1, 2) for i in range(3))
    pos = torch.arange(U)
    vis = (pos[None, :] <= pos[:, None])[None] & (pos[None, None, :] >= torch.as_tensor(begin)[:, None, None])
    vis = vis[:, None]
    s = (q @ k.transpose(-2, -1) * scale).masked_fill(~vis, -float("inf"))
    p = torch.softmax(s, -1).masked_fill(~vis, 0.0)
    return torch.nan_to_num(p, nan=0.0).matmul(v).transpose(1, 2).reshape(R * U, D)


def begins(U, R, rot=0):
    """Per-row pad counts out of 0, 1, 15, 16, U - 1 that fit U, mixed in one launch; rotation ``rot`` of the pool, so that over
    ``rotations(U, R)`` every value is run at every U and R."""
    pool = sorted({b for b in (0, 1, 15, 16, U - 1) if 0 <= b < U})
    return [pool[(rot + r) % len(pool)] for r in range(R)]


def rotations(U, R):
    n = len({b for b in (0, 1, 15, 16, U - 1) if 0 <= b < U})
    return range(0, n, min(R, n)) if n > R else range(1)


def prefill_case(ops, R, U, dk, begin, beam_layout=False, seed=0):
    H, Umax, padc = 2, U + 3, 4
    D = H * dk
    g = torch.Generator().manual_seed(1000 * U + 10 * R + dk + seed)
    qkv_full = torch.randn(R * U, 3 * D + 4, generator=g)
    if beam_layout:                                    # the first row of every group of 3: a free row stride
        kc_full = torch.full((3 * R, Umax, D + padc), GUARD).cuda()
        vc_full = torch.full((3 * R, Umax, D + padc), GUARD).cuda()
        kc, vc = kc_full[::3, :, :D], vc_full[::3, :, :D]
    else:
        kc_full, vc_full = torch.full((R, Umax, D + padc), GUARD).cuda(), torch.full((R, Umax, D + padc), GUARD).cuda()
        kc, vc = kc_full[:, :, :D], vc_full[:, :, :D]
    qd = qkv_full.cuda()
    q0 = qd.clone()
    out_full = torch.full((R * U, D + 8), GUARD).cuda()
    bd = None if begin is None else torch.tensor(begin, dtype=I32).cuda()
    out = ops.attn_prefill_f32(qd[:, :3 * D], kc, vc, U, H, dk ** -0.5, begin=bd, out=out_full[:, :D])
    torch.cuda.synchronize()
    assert torch.equal(qd, q0), "qkv was written"
    assert bool((out_full[:, D:] == GUARD).all()), "the gap of out's row stride was written"
    # the caches: slots [r][:U] hold the k / v columns bit for bit, every other byte is untouched
    wk, wv = torch.full_like(kc_full, GUARD), torch.full_like(vc_full, GUARD)
    step = 3 if beam_layout else 1
    wk[::step, :U, :D] = qd[:, D:2 * D].view(R, U, D)
    wv[::step, :U, :D] = qd[:, 2 * D:3 * D].view(R, U, D)
    assert torch.equal(kc_full, wk) and torch.equal(vc_full, wv), "cache slots / containment"
    return qkv_full[:, :3 * D], out.clone(), (kc_full, vc_full)


@pytest.mark.parametrize("dk", [16, 64])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("U", [1, 15, 16, 17, 33])
def test_prefill_equals_dense_causal_attention_and_files_the_caches(ops, U, R, dk):
    """Measured on an MI355X: relative L2 at most 1.6e-7 over these cases (gate 1e-5)."""
    seen = set()
    for begin in [None] + [begins(U, R, rot) for rot in rotations(U, R)]:
        seen |= set(begin or [0])
        qkv, out, _ = prefill_case(ops, R, U, dk, begin)
        b = [0] * R if begin is None else begin
        want = dense_prefill(qkv, R, U, 2, dk, b, dk ** -0.5)
        got = out.cpu().view(R, U, -1)
        for r in range(R):
            assert bool((got[r, :b[r]] == 0).all()), f"row {r}: queries below begin = {b[r]} must be exact zeros"
        err = rel_l2(got.reshape(R * U, -1), want)
        print(f"prefill U={U} R={R} dk={dk} begin={begin}: rel L2 {err:.3e}")
        assert err < 1e-5
        again = prefill_case(ops, R, U, dk, begin)[1]
        assert torch.equal(out, again), "two launches differ"
    assert seen == {b for b in (0, 1, 15, 16, U - 1) if 0 <= b < U}, seen       # every pad count that fits U was run


@pytest.mark.parametrize("dk", [16, 64])
def test_prefill_row_of_a_batch_equals_its_own_launch_bit_for_bit(ops, dk):
    U, R, H = 33, 3, 2
    D = H * dk
    begin = begins(U, R)
    qkv, out, _ = prefill_case(ops, R, U, dk, begin)
    for r in range(R):
        kc, vc = torch.zeros(1, U, D).cuda(), torch.zeros(1, U, D).cuda()
        one = ops.attn_prefill_f32(qkv[r * U:(r + 1) * U].cuda().contiguous(), kc, vc, U, H, dk ** -0.5,
                                   begin=torch.tensor(begin[r:r + 1], dtype=I32).cuda())
        assert torch.equal(one, out[r * U:(r + 1) * U]), f"row {r}"


def test_prefill_on_non_contiguous_cache_views(ops):
    qkv, out, _ = prefill_case(ops, 3, 17, 16, begins(17, 3), beam_layout=True)
    assert rel_l2(out, dense_prefill(qkv, 3, 17, 2, 16, begins(17, 3), 0.25)) < 1e-5


@pytest.mark.parametrize("dk", [16, 64])
def test_decode_from_reads_keys_from_begin_and_equals_the_plain_step_without(ops, dk):
    R, H, Umax, padc = 3, 2, 70, 4
    D = H * dk
    g = torch.Generator().manual_seed(dk)
    scale = 1.0 / math.sqrt(dk)
    for p in (0, 5, 64, 65):
        for with_anc in (True, False):
            kc_full, vc_full = torch.randn(R, Umax, D + padc, generator=g).cuda(), torch.randn(R, Umax, D + padc, generator=g).cuda()
            qkv_full = torch.randn(R, 3 * D + 4, generator=g).cuda()
            qkv = qkv_full[:, :3 * D]
            anc_h = torch.randint(0, R, (R, Umax), generator=g)
            anc = anc_h.int().cuda() if with_anc else None
            k0, v0 = kc_full.clone(), vc_full.clone()
            plain = ops.attn_decode_f32(qkv, kc_full.clone()[:, :, :D], vc_full.clone()[:, :, :D], p, H, scale, anc=anc)
            for begin in ([0, 0, 0], [min(3, p), p, 0], [p, 0, min(3, p)]):
                kc_f, vc_f = k0.clone(), v0.clone()
                out = ops.attn_decode_f32(qkv, kc_f[:, :, :D], vc_f[:, :, :D], p, H, scale, anc=anc,
                                          begin=torch.tensor(begin, dtype=I32).cuda())
                if not any(begin):
                    assert torch.equal(out, plain), f"p={p} anc={with_anc}: begin = 0 must give f5e_attn_decode_f32's bits"
                src = anc_h[:, :p] if with_anc else torch.arange(R)[:, None].expand(-1, p)
                q, kn, vn = (qkv_full[:, i * D:(i + 1) * D].cpu().double() for i in range(3))
                pos = torch.arange(p)[None, :]
                K = torch.cat((k0[:, :, :D].cpu().double()[src, pos], kn[:, None]), 1).view(R, p + 1, H, dk).transpose(1, 2)
                Vv = torch.cat((v0[:, :, :D].cpu().double()[src, pos], vn[:, None]), 1).view(R, p + 1, H, dk).transpose(1, 2)
                s = (q.view(R, H, 1, dk) @ K.transpose(-2, -1)) * scale
                hidden = torch.arange(p + 1)[None, :] < torch.tensor(begin)[:, None]
                a = torch.softmax(s.masked_fill(hidden[:, None, None, :], -float("inf")), -1)
                want = (a @ Vv).transpose(1, 2).reshape(R, D)
                err = rel_l2(out, want)
                assert err < 2e-4, f"p={p} anc={with_anc} begin={begin}: rel L2 {err:.2e}"
                w_k, w_v = k0.clone(), v0.clone()
                w_k[:, p, :D], w_v[:, p, :D] = qkv_full[:, D:2 * D], qkv_full[:, 2 * D:3 * D]
                assert torch.equal(kc_f, w_k) and torch.equal(vc_f, w_v), f"p={p} begin={begin}: cache containment"


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("U", [1, 5])
def test_whisper_embed_is_exact(ops, R, U):
    V, P, D = 11, 9, 8
    g = torch.Generator().manual_seed(R * 10 + U)
    emb, pos = torch.randn(V, D, generator=g), torch.randn(P, D, generator=g)
    ids = torch.randint(0, V, (R, U), generator=g).int()
    for p0 in (0, 3):
        for begin in (None, [(2 * r + 1) % (p0 + U + 1) for r in range(R)]):
            buf = torch.full((R * U * D + 8,), GUARD).cuda()
            out = buf[4:4 + R * U * D].view(R, U, D)
            ops.whisper_embed(ids.cuda(), emb.cuda(), pos.cuda(), out, p0, None if begin is None else torch.tensor(begin, dtype=I32).cuda())
            b = np.zeros(R, np.int64) if begin is None else np.asarray(begin)
            at = np.maximum(p0 + np.arange(U)[None, :] - b[:, None], 0)
            want = emb.numpy()[ids.numpy()] + pos.numpy()[at]
            assert np.array_equal(out.cpu().numpy(), want), f"p0={p0} begin={begin}"
            assert bool((buf[:4] == GUARD).all()) and bool((buf[-4:] == GUARD).all())
    # an id outside the table handed over on the device is clamped
    bad = torch.tensor([[-3] * U] * R, dtype=I32).cuda()
    got = ops.whisper_embed(bad, emb.cuda(), pos.cuda(), torch.empty(R, U, D).cuda())
    assert np.array_equal(got.cpu().numpy(), np.broadcast_to(emb.numpy()[0][None, None] + pos.numpy()[None, :U], (R, U, D)))


def test_refusals_leave_the_outputs_untouched(ops):
    from f5e_tts_amd._C import F5EError
    R, U, H, dk = 2, 4, 2, 16
    D = H * dk
    qkv = torch.zeros(R * U, 3 * D).cuda()
    kc, vc, out = (torch.full(s, GUARD).cuda() for s in ((R, 6, D), (R, 6, D), (R * U, D)))

    def untouched():
        torch.cuda.synchronize()
        return bool((kc == GUARD).all()) and bool((vc == GUARD).all()) and bool((out == GUARD).all())
    for call in (lambda: ops.attn_prefill_f32(qkv[:0], kc, vc, 0, H, 1.0, out=out),                       # U < 1
                 lambda: ops.attn_prefill_f32(torch.zeros(R * 7, 3 * D).cuda(), kc, vc, 7, H, 1.0),      # U beyond the cache
                 lambda: ops.attn_prefill_f32(qkv[:, :2 * D], kc, vc, U, H, 1.0, out=out),                # qkv narrower than 3 D
                 lambda: ops.attn_prefill_f32(qkv, torch.as_strided(kc, (R, 6, D), (6 * D, D // 2, 1)),    # a position stride
                                              torch.as_strided(vc, (R, 6, D), (6 * D, D // 2, 1)), U, H, 1.0, out=out),   # below H dk
                 lambda: ops.attn_prefill_f32(qkv, kc, vc, U, 8, 1.0, out=out)):                          # head dim 4
        with pytest.raises(F5EError):
            call()
        assert untouched()
    mis = torch.full((R * 6 * D + 4,), GUARD).cuda()
    with pytest.raises(F5EError):                                                                         # misaligned cache
        ops.attn_prefill_f32(qkv, mis[1:1 + R * 6 * D].view(R, 6, D), vc, U, H, 1.0, out=out)
    with pytest.raises(F5EError):                                                                         # begin on the host
        ops.attn_prefill_f32(qkv, kc, vc, U, H, 1.0, begin=torch.zeros(R, dtype=I32), out=out)
    assert untouched() and bool((mis == GUARD).all())
    q1 = torch.zeros(R, 3 * D).cuda()
    o1 = torch.full((R, D), GUARD).cuda()
    with pytest.raises(F5EError):
        ops.attn_decode_f32(q1, kc, vc, 6, H, 1.0, out=o1, begin=torch.zeros(R, dtype=I32).cuda())       # p == Umax
    with pytest.raises(F5EError):
        ops.attn_decode_f32(q1, kc, vc, 0, H, 1.0, out=o1, begin=torch.zeros(R + 1, dtype=I32).cuda())   # begin of another length
    assert untouched() and bool((o1 == GUARD).all())
    emb, pos, x = torch.zeros(5, 8).cuda(), torch.zeros(4, 8).cuda(), torch.full((R, 2, 8), GUARD).cuda()
    ids = torch.zeros(R, 2, dtype=I32).cuda()
    with pytest.raises(F5EError):
        ops.whisper_embed(ids, emb, pos, x, 3)                                                            # position 4 of 4
    with pytest.raises(F5EError):
        ops.whisper_embed(ids, emb, pos[:, :4], x)                                                        # pos of another width
    with pytest.raises(F5EError):
        ops.whisper_embed(ids.cpu(), emb, pos, x)                                                         # ids on the host
    torch.cuda.synchronize()
    assert bool((x == GUARD).all())
