"""Whisper's assisted generation (speculative decoding) on the GPU: the four kernels (csrc/whisper_append.hip,
csrc/gemm_f32_skinny.hip) against float64 / the single-step kernels, and ``generate`` / ``transcribe_long`` with an assistant
against the same calls without one.

Gates (none invented here):
  * f5e_attn_append_f32: relative L2 <= 1e-5 against float64, the gate of f5e_attn_prefill_f32 (tests/test_whisper_prefill_gpu.py):
    the same wave tile and arithmetic.  Cache slots bit for bit; everything a launch must not write by equality with a copy.
  * f5e_gemm_f32_skinny: integer-valued operands exactly, on the whole sentinel-filled buffer; random ones within the standard
    summation bound of tests/test_fp32_ops_gpu.py, (K + 8) 2^-24 (|A| |W|^T + |bias|), plus that file's 1e-5 relative / 3e-5
    absolute behind a GELU.
  * f5e_whisper_verify: bit-equal to f5e_greedy_pick / f5e_whisper_ts_pick on the same logits row and history (one body).
  * f5e_whisper_accept: the hand-made cases of tests/whisper_assist_ref.py, exactly.
  * the model: tokens, lengths, segments and seeks EQUAL to the run without an assistant (the fixtures' steps keep margins of at
    least 1e-2 of the logits' RMS, so the fp32 summation order of the append pass cannot flip a pick); sum_logp, no_speech_logp
    and avg_logprob within 2e-4 relative, the gate these figures have in tests/test_whisper_long_gpu.py."""
import numpy as np
import pytest
import torch

import test_whisper_cpu as WC
import test_whisper_long_cpu as LC
import whisper_assist_ref as AR

pytestmark = pytest.mark.gpu

I32, F32 = torch.int32, torch.float32
GUARD, SENT, GATE = -7.0, -77.0, 2e-4
_dev = {}


@pytest.fixture(scope="module")
def ops():
    import f5e_tts_amd.ops as ops_mod
    ops_mod.require_device()
    return ops_mod


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


# ---- f5e_attn_append_f32 ------------------------------------------------------------------------------------------------------------

def dense_append(qkv, kc, vc, R, U, H, dk, p0, begin, scale):
    """fp64: query u of row r (position p0 + u) sees the cached positions begin[r] .. p0 - 1 of kc / vc and the new keys 0 .. u
    of qkv; a query below begin[r] gives zeros.  qkv [R * U, 3 D], kc / vc [R, >= p0, D] -> [R * U, D]."""
    D = H * dk
    out = torch.zeros(R, U, D, dtype=torch.float64)
    q, kn, vn = (qkv[:, i * D:(i + 1) * D].double().view(R, U, D) for i in range(3))
    for r in range(R):
        K = torch.cat((kc[r, :p0].double(), kn[r]), 0).view(p0 + U, H, dk)
        V = torch.cat((vc[r, :p0].double(), vn[r]), 0).view(p0 + U, H, dk)
        for u in range(U):
            lo, hi = begin[r], p0 + u + 1
            if p0 + u < lo:
                continue
            s = torch.einsum("hd,jhd->hj", q[r, u].view(H, dk), K[lo:hi]) * scale
            out[r, u] = torch.einsum("hj,jhd->hd", torch.softmax(s, -1), V[lo:hi]).reshape(D)
    return out.view(R * U, D)


def append_case(ops, R, U, dk, p0, begin, beam_layout=False, seed=0):
    """One launch on padded strides (or the beam view: the first row of every group of 3) -> (qkv, out, the caches before)."""
    H, Umax, padc = 2, p0 + U + 2, 4
    D = H * dk
    g = torch.Generator().manual_seed(100000 * p0 + 1000 * U + 10 * R + dk + seed)
    qd = torch.randn(R * U, 3 * D + 4, generator=g).cuda()
    step = 3 if beam_layout else 1
    kc_full, vc_full = (torch.randn(step * R, Umax, D + padc, generator=g).cuda() for _ in range(2))
    kc, vc = kc_full[::step, :, :D], vc_full[::step, :, :D]
    q0, k0, v0 = qd.clone(), kc_full.clone(), vc_full.clone()
    out_full = torch.full((R * U, D + 8), GUARD).cuda()
    bd = None if begin is None else torch.tensor(begin, dtype=I32).cuda()
    out = ops.attn_append_f32(qd[:, :3 * D], kc, vc, U, p0, H, dk ** -0.5, begin=bd, out=out_full[:, :D])
    torch.cuda.synchronize()
    assert torch.equal(qd, q0), "qkv was written"
    assert bool((out_full[:, D:] == GUARD).all()), "the gap of out's row stride was written"
    wk, wv = k0.clone(), v0.clone()                       # slots p0 .. p0 + U - 1 hold the k / v columns; nothing else moved
    wk[::step, p0:p0 + U, :D] = qd[:, D:2 * D].view(R, U, D)
    wv[::step, p0:p0 + U, :D] = qd[:, 2 * D:3 * D].view(R, U, D)
    assert torch.equal(kc_full, wk) and torch.equal(vc_full, wv), "cache slots / containment"
    return qd[:, :3 * D].cpu(), out.clone(), (k0[::step, :, :D].cpu(), v0[::step, :, :D].cpu())


def begin_sets(p0, U, R):
    """None and the per-row pad counts out of 0, 1, 15, 16, p0, p0 + U - 1 that fit, mixed in one launch, every one of them run."""
    pool = sorted({b for b in (0, 1, 15, 16, p0, p0 + U - 1) if 0 <= b < p0 + U})
    sets = [None]
    for s in range(0, len(pool), R):
        sets.append([pool[(s + r) % len(pool)] for r in range(R)])
    return sets


@pytest.mark.parametrize("dk", [16, 64])
@pytest.mark.parametrize("R", [1, 3])
def test_append_equals_dense_attention_and_files_the_caches(ops, R, dk):
    worst = 0.0
    for p0 in (0, 1, 15, 16, 17, 63, 64, 65):
        for U in (1, 2, 6, 16, 17):
            for begin in begin_sets(p0, U, R):
                qkv, out, (k0, v0) = append_case(ops, R, U, dk, p0, begin)
                b = [0] * R if begin is None else begin
                want = dense_append(qkv, k0, v0, R, U, 2, dk, p0, b, dk ** -0.5)
                got = out.cpu().view(R, U, -1)
                for r in range(R):
                    below = max(b[r] - p0, 0)
                    assert bool((got[r, :below] == 0).all()), f"p0={p0} U={U} row {r}: queries below begin = {b[r]} must be exact zeros"
                err = rel_l2(got.reshape(R * U, -1), want)
                worst = max(worst, err)
                assert err <= 1e-5, f"p0={p0} U={U} R={R} dk={dk} begin={begin}: rel L2 {err:.3e}"
    print(f"append R={R} dk={dk}: largest rel L2 {worst:.3e} (gate 1e-5)")


@pytest.mark.parametrize("dk", [16, 64])
def test_append_at_position_zero_is_the_prefill(ops, dk):
    R, H = 3, 2
    D = H * dk
    for U in (1, 6, 17):
        for begin in (None, [0, 1, U - 1]):
            qkv, out, _ = append_case(ops, R, U, dk, 0, begin)
            kc, vc = torch.zeros(R, U, D).cuda(), torch.zeros(R, U, D).cuda()
            bd = None if begin is None else torch.tensor(begin, dtype=I32).cuda()
            pre = ops.attn_prefill_f32(qkv.cuda().contiguous(), kc, vc, U, H, dk ** -0.5, begin=bd)
            live = pre.abs().sum() > 0
            assert (rel_l2(out, pre) <= 1e-5) if live else torch.equal(out, pre), f"U={U} begin={begin}"


@pytest.mark.parametrize("dk", [16, 64])
def test_append_row_of_a_batch_equals_its_own_launch_and_two_launches_agree(ops, dk):
    R, H, U, p0 = 3, 2, 17, 33
    D = H * dk
    begin = [0, 16, p0 + 3]
    qkv, out, (k0, v0) = append_case(ops, R, U, dk, p0, begin)
    again = append_case(ops, R, U, dk, p0, begin)[1]
    assert torch.equal(out, again), "two launches differ"
    for r in range(R):
        kc, vc = k0[r:r + 1].cuda().contiguous(), v0[r:r + 1].cuda().contiguous()
        one = ops.attn_append_f32(qkv[r * U:(r + 1) * U].cuda().contiguous(), kc, vc, U, p0, H, dk ** -0.5,
                                  begin=torch.tensor(begin[r:r + 1], dtype=I32).cuda())
        assert torch.equal(one, out[r * U:(r + 1) * U]), f"row {r}"


def test_append_on_the_beam_view(ops):
    for p0, U in ((17, 6), (64, 17)):
        begin = [1, 16, p0]
        qkv, out, (k0, v0) = append_case(ops, 3, U, 16, p0, begin, beam_layout=True)
        assert rel_l2(out, dense_append(qkv, k0, v0, 3, U, 2, 16, p0, begin, 0.25)) <= 1e-5


def test_append_refusals_leave_the_outputs_untouched(ops):
    from f5e_tts_amd._C import F5EError
    R, U, H, dk = 2, 4, 2, 16
    D = H * dk
    qkv = torch.zeros(R * U, 3 * D).cuda()
    kc, vc, out = (torch.full(s, GUARD).cuda() for s in ((R, 6, D), (R, 6, D), (R * U, D)))
    for call in (lambda: ops.attn_append_f32(qkv, kc, vc, U, -1, H, 1.0, out=out),                        # p0 < 0
                 lambda: ops.attn_append_f32(qkv, kc, vc, U, 3, H, 1.0, out=out),                         # p0 + U > Umax
                 lambda: ops.attn_append_f32(qkv[:0], kc, vc, 0, 0, H, 1.0, out=out),                     # U < 1
                 lambda: ops.attn_append_f32(qkv[:, :2 * D], kc, vc, U, 0, H, 1.0, out=out),              # qkv narrower than 3 D
                 lambda: ops.attn_append_f32(qkv, kc, vc, U, 0, 8, 1.0, out=out),                         # head dim 4
                 lambda: ops.attn_append_f32(qkv, kc, vc, U, 0, H, 1.0, begin=torch.zeros(R, dtype=I32), out=out)):   # begin on the host
        with pytest.raises(F5EError):
            call()
    mis = torch.full((R * 6 * D + 4,), GUARD).cuda()
    with pytest.raises(F5EError):                                                                         # misaligned cache
        ops.attn_append_f32(qkv, mis[1:1 + R * 6 * D].view(R, 6, D), vc, U, 0, H, 1.0, out=out)
    torch.cuda.synchronize()
    assert all(bool((t == GUARD).all()) for t in (kc, vc, out, mis))


# ---- f5e_gemm_f32_skinny --------------------------------------------------------------------------------------------------------------

def skinny_operands(M, N, K, integer, seed, bias=True, addend=True):
    g = torch.Generator().manual_seed(seed)
    if integer:
        draw = lambda *s: torch.randint(-3, 4, s, generator=g).float()   # noqa: E731
    else:
        draw = lambda *s: torch.randn(*s, generator=g)                    # noqa: E731
    return draw(M, K), draw(N, K), draw(N) if bias else None, draw(M, N) if addend else None


def run_skinny(ops, A, W, bias, addend, act=0, alias=False):
    """A and W as views of padded rows, out as a view inside a sentinel-filled buffer -> (the whole buffer, the view's slice)."""
    (M, K), N = A.shape, W.shape[0]
    Ad, Wd = torch.full((M, K + 4), SENT).cuda(), torch.full((N, K + 8), SENT).cuda()
    Ad[:, :K], Wd[:, :K] = A, W
    ldo = N + 3
    buf = torch.full((M + 2, ldo), SENT).cuda()
    out = buf[1:M + 1, 1:N + 1]
    add = None
    if addend is not None:
        if alias:
            out.copy_(addend)
            add = out
        else:
            add = torch.full((M, N + 5), SENT).cuda()
            add[:, :N] = addend
            add = add[:, :N]
    a0, w0 = Ad.clone(), Wd.clone()
    ops.gemm_f32_skinny(Ad[:, :K], Wd[:, :K], None if bias is None else bias.cuda(), out=out, act=act, addend=add)
    torch.cuda.synchronize()
    assert torch.equal(Ad, a0) and torch.equal(Wd, w0), "an input operand changed"
    return buf.cpu(), (slice(1, M + 1), slice(1, N + 1))


def skinny_ref(A, W, bias, addend, act=0):
    y = A.double() @ W.double().t()
    if bias is not None:
        y = y + bias.double()
    if act:
        y = 0.5 * y * (1.0 + torch.erf(y / 2.0 ** 0.5))
    return y if addend is None else y + addend.double()


@pytest.mark.parametrize("K", [4, 60, 1280, 1300])
@pytest.mark.parametrize("N", [1, 4, 63, 64, 65, 1280])
def test_skinny_integer_cases_are_exact_on_the_whole_buffer(ops, N, K):
    """K = 1300 is 82 chunks of 16, which no K split of this launch divides evenly (N = 1280 splits it 5 x 4 ways on 256 CUs)."""
    for M in (1, 2, 6, 16):
        for bias, addend in ((True, True), (False, False)):
            A, W, b, add = skinny_operands(M, N, K, True, 7 * M + N + K, bias, addend)
            buf, sl = run_skinny(ops, A, W, b, add)
            want = torch.full_like(buf, SENT)
            want[sl] = skinny_ref(A, W, b, add).float()
            assert torch.equal(buf, want), f"M={M} N={N} K={K} bias={bias}: {int((buf != want).sum())} elements differ"
    if N >= 1280 and K >= 1280:
        assert ops.gemm_f32_skinny_workspace(N, K) > 0                   # the K split across workgroups really ran


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M,N,K", [(1, 65, 60), (6, 1280, 1280), (16, 1280, 1300), (6, 5120, 1280), (3, 1280, 5120), (16, 63, 1280)])
def test_skinny_random_cases_within_the_summation_bound(ops, M, N, K, act):
    from f5e_tts_amd import ops as O
    A, W, b, add = skinny_operands(M, N, K, False, M + N + K)
    code = O.ACT_GELU_ERF if act else O.ACT_NONE
    buf, sl = run_skinny(ops, A, W, b, add, act=code)
    ref = skinny_ref(A, W, b, add, act)
    gate = (K + 8) * 2.0 ** -24 * (A.double().abs() @ W.double().abs().t() + b.double().abs())
    if act:
        gate = gate + 1e-5 * ref.abs() + 3e-5
    gate = gate + 2.0 ** -24 * ref.abs()                                 # the addend's own rounding
    err = (buf[sl].double() - ref).abs()
    print(f"M={M} N={N} K={K} act={act}: kernel vs fp64 {float(err.max()):.3e}, largest err / gate {float((err / gate).max()):.2e}")
    assert bool((err <= gate).all())
    rest = buf.clone()
    rest[sl] = SENT
    assert bool((rest == SENT).all())


def test_skinny_addend_aliased_to_out_rows_independent_of_m_and_reproducible(ops):
    from f5e_tts_amd import ops as O
    for N, K in ((1280, 1280), (65, 1300), (5120, 1280)):
        A, W, b, add = skinny_operands(16, N, K, False, N + K)
        full, sl = run_skinny(ops, A, W, b, add, act=O.ACT_GELU_ERF)
        again, _ = run_skinny(ops, A, W, b, add, act=O.ACT_GELU_ERF)
        alias, _ = run_skinny(ops, A, W, b, add, act=O.ACT_GELU_ERF, alias=True)
        assert torch.equal(full, again), "two launches differ"
        assert torch.equal(full, alias), "addend aliased to out"
        for m in (0, 5, 15):
            one, s1 = run_skinny(ops, A[m:m + 1], W, b, add[m:m + 1], act=O.ACT_GELU_ERF)
            assert torch.equal(one[s1][0], full[sl][m]), f"N={N} K={K}: row {m} of M = 16 differs from its own M = 1 launch"


def test_skinny_refusals_leave_the_outputs_untouched(ops):
    from f5e_tts_amd._C import F5EError
    from f5e_tts_amd import ops as O
    z = lambda *s: torch.zeros(*s).cuda()   # noqa: E731
    out = torch.full((17, 8), SENT).cuda()
    mis = torch.full((4 * 16 + 4,), SENT).cuda()
    for call in (lambda: ops.gemm_f32_skinny(z(17, 16), z(8, 16), out=out),                               # M = 17
                 lambda: ops.gemm_f32_skinny(z(4, 6), z(8, 6), out=out[:4]),                               # K % 4
                 lambda: ops.gemm_f32_skinny(z(4, 16), z(8, 12), out=out[:4]),                             # K of w
                 lambda: ops.gemm_f32_skinny(z(4, 16), z(8, 16), out=out[:4], act=O.ACT_SILU),            # an activation not built
                 lambda: ops.gemm_f32_skinny(z(4, 16), z(8, 16), out=out[:4, :6]),                         # out narrower than N
                 lambda: ops.gemm_f32_skinny(z(4, 16), z(8, 16), out=out[:3]),                             # out of other rows
                 lambda: ops.gemm_f32_skinny(z(4, 16), z(8, 16), z(4), out=out[:4]),                       # a short bias
                 lambda: ops.gemm_f32_skinny(mis[1:65].view(4, 16), z(8, 16), out=out[:4]),                # a misaligned operand
                 lambda: ops.gemm_f32_skinny(z(4, 16), z(8, 16), out=out[:4], addend=z(3, 8)),             # addend of other rows
                 lambda: ops.gemm_f32_skinny(z(4, 1280), z(1280, 1280), out=z(4, 1280), workspace=z(16))):   # a workspace too small
        with pytest.raises(F5EError):
            call()
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((mis == SENT).all())


# ---- f5e_whisper_verify ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V,ld", ((160, 160), (163, 163), (51866, 51868)))
@pytest.mark.parametrize("rules", (False, True))
def test_verify_equals_the_single_step_kernels_bit_for_bit(ops, V, ld, rules):
    """Rows: the first step (begin_suppress and max_initial count at j = 0 alone), then after one timestamp, after two, text
    behind a pair, text then a timestamp; a row whose logits allow nothing; a row of text only.  V = 163 is no multiple of 4."""
    n_ts = 51 if V <= 1000 else 1501
    no_ts = V - n_ts - 1
    tb, eos = no_ts + 1, no_ts - 10
    n0, U = 3, 4
    p = n0 - 1
    R = 4
    g = np.random.default_rng(V + rules)
    x = (g.standard_normal((R * (U + 1), V)) * 3.0).astype(np.float32)
    x[:, tb:] += np.repeat(np.array([2.0, -6.0, 0.0, 1.0], np.float32), U + 1)[:, None] - np.float32(np.log(n_ts / 51.0))
    x[1 * (U + 1):2 * (U + 1)] = -np.inf                                  # nothing is allowed
    x[2 * (U + 1) + 1, [5, tb + 7]] = 50.0                               # a tie between a text class and a timestamp
    x[3 * (U + 1) + 2, 20] = x[3 * (U + 1) + 2, 40] = 45.0               # a tie among the text classes
    drafts = [[tb + 3, tb + 3, 17, tb + 9], [tb, 17, 18, eos], [17, 18, 19, 20], [tb + 2, 30, tb + 5, tb + 5]]
    wide = torch.full((R * (U + 1) + 2, ld), 1e9)
    wide[1:-1, :V] = torch.from_numpy(x)
    dl = wide.cuda()
    logits = dl[1:-1, :V] if ld > V else dl[1:-1]
    hist = torch.full((R, p + U + 3), -5, dtype=I32)
    hist[:, :n0] = torch.tensor([7, 8, 9], dtype=I32)
    hist[:, n0:n0 + U] = torch.tensor(drafts, dtype=I32)
    hd = hist.cuda()
    sup = torch.tensor([2, 3, -1, V + 5, eos + 1, tb + 5], dtype=I32).cuda()
    beg = torch.tensor([4, eos, tb + 1], dtype=I32).cuda()
    cand_buf, logp_buf = torch.full((R + 2, U + 1), -9, dtype=I32).cuda(), torch.full((R + 2, U + 1), 0.5).cuda()
    kw = dict(V=V, suppress=sup, begin_suppress=beg)
    if rules:
        kw["max_initial"] = 25
    ops.whisper_verify(logits, hd, cand_buf[1:-1], logp_buf[1:-1], p, n0, eos, no_ts if rules else None, **kw)
    torch.cuda.synchronize()
    assert torch.equal(dl.cpu(), wide) and torch.equal(hd.cpu(), hist), "an input changed"
    assert bool((cand_buf[[0, -1]] == -9).all()) and bool((logp_buf[[0, -1]] == 0.5).all())
    seen = set()
    for r in range(R):
        for j in range(U + 1):
            row = logits[r * (U + 1) + j:r * (U + 1) + j + 1]
            table = hd[r:r + 1].clone()
            last, done, alive = (torch.zeros(1, dtype=I32).cuda() for _ in range(3))
            slp = torch.zeros(1).cuda()
            if rules:
                ops.whisper_ts_pick(row, table, last, done, alive, slp, p + j, n0, eos, no_ts, **kw)
            else:
                ops.greedy_pick(row, table, last, done, alive, p + j, eos, first_step=p + j + 1 == n0, **kw)
            assert int(cand_buf[1 + r, j]) == int(table[0, p + j + 1]) == int(last[0]), (r, j)
            assert torch.equal(logp_buf[1 + r, j:j + 1], slp), (r, j, float(logp_buf[1 + r, j]), float(slp))
            seen.add(int(last[0]) >= tb)
    if rules:
        assert seen == {True, False}                                       # text and timestamps were both picked
        assert int(cand_buf[1, 0]) >= tb and float(logp_buf[1, 0]) < 0.0    # the first step picks a timestamp under the rules
        assert bool((cand_buf[2] == 0).all()) and bool((logp_buf[2] == 0).all())   # nothing allowed: 0, nothing added
    else:
        assert bool((logp_buf[1:-1] == 0).all())


def test_verify_refusals(ops):
    from f5e_tts_amd._C import F5EError
    lg, hist = torch.zeros(6, 16).cuda(), torch.zeros(2, 8, dtype=I32).cuda()
    cand, logp = torch.full((2, 3), -9, dtype=I32).cuda(), torch.full((2, 3), 0.5).cuda()
    for call in (lambda: ops.whisper_verify(lg, hist, cand, logp, 1, 3, 1),                 # p < n0 - 1
                 lambda: ops.whisper_verify(lg, hist, cand, logp, 6, 3, 1),                 # the history is too short
                 lambda: ops.whisper_verify(lg, hist, cand, logp, 3, 3, 16),                # eos outside the vocabulary
                 lambda: ops.whisper_verify(lg, hist, cand, logp, 3, 3, 1, 15),             # no timestamp classes
                 lambda: ops.whisper_verify(lg[:5], hist, cand, logp, 3, 3, 1),             # logits of other rows
                 lambda: ops.whisper_verify(lg, hist, cand, logp, 3, 3, 1, V=17)):          # V beyond the columns
        with pytest.raises(F5EError):
            call()
    torch.cuda.synchronize()
    assert bool((cand == -9).all()) and bool((logp == 0.5).all())


# ---- f5e_whisper_accept ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_sum", (True, False))
@pytest.mark.parametrize("case", AR.ACCEPT_CASES, ids=[c["name"] for c in AR.ACCEPT_CASES])
def test_accept_hand_made_cases_exactly(ops, case, with_sum):
    eos, p, pad = AR.ACCEPT_EOS, 3, 2
    cand, drafts, done0 = case["cand"], case["drafts"], case["done"]
    R, U, a = len(cand), len(drafts[0]), case["a"]
    ld = p + U + 2 + pad
    logp = AR.accept_logp(case)
    tokens = torch.full((R + 2, ld), -5, dtype=I32)
    tokens[1:-1, :p + 1] = torch.arange(20, 20 + p + 1, dtype=I32)
    hist = tokens.clone()
    hist[1:-1, p + 1:p + 1 + U] = torch.tensor(drafts, dtype=I32)
    td, hd = tokens.cuda(), hist.cuda()
    cd, ld_ = torch.tensor(cand, dtype=I32).cuda(), torch.tensor(logp, dtype=F32).cuda()
    c0, l0 = cd.clone(), ld_.clone()
    vec, misc = torch.full((2, R + 2), -5, dtype=I32).cuda(), torch.full((4,), -5, dtype=I32).cuda()
    last, done = vec[0, 1:-1], vec[1, 1:-1]                              # misc: guard, alive, adv, guard
    done.copy_(torch.tensor(done0, dtype=I32))
    slp = torch.full((R + 2,), 0.5).cuda()
    slp[1:-1] = 1.0
    ops.whisper_accept(cd, ld_, hd[1:-1], td[1:-1], last, done, misc[1:2], slp[1:-1] if with_sum else None, misc[2:3], p, eos)
    torch.cuda.synchronize()
    want_t, want_h = tokens.clone(), hist.clone()
    want_t[1:-1, p + 1:p + 1 + a] = torch.tensor(case["new"], dtype=I32)
    want_h[1:-1, p + 1:p + 1 + a] = torch.tensor(case["new"], dtype=I32)
    want_h[1:-1, p + 1 + a:p + 1 + U] = eos
    assert torch.equal(td.cpu(), want_t), "tokens: columns p + 1 .. p + a, nothing beyond and no other byte"
    assert torch.equal(hd.cpu(), want_h), "hist: tokens up to p + a, eos on the rejected drafts"
    assert last.tolist() == [row[-1] for row in case["new"]] and done.tolist() == case["after"]
    assert int(misc[1]) == sum(1 for d in case["after"] if not d) and int(misc[2]) == a
    assert vec[0, [0, -1]].tolist() == [-5, -5] and vec[1, [0, -1]].tolist() == [-5, -5] and int(misc[0]) == -5 and int(misc[3]) == -5
    want_s = [1.0 + sum(logp[r][:k]) for r, k in enumerate(case["kept"])] if with_sum else [1.0] * R
    assert slp.tolist() == [0.5] + want_s + [0.5]
    assert torch.equal(cd, c0) and torch.equal(ld_, l0)


def test_accept_refusals(ops):
    from f5e_tts_amd._C import F5EError
    zi = lambda *s: torch.full(s, -5, dtype=I32).cuda()   # noqa: E731
    cand, logp, hist, tokens = zi(2, 3), torch.zeros(2, 3).cuda(), zi(2, 8), zi(2, 8)
    last, done, alive, adv = zi(2), zi(2), zi(1), zi(1)
    for call in (lambda: ops.whisper_accept(cand, logp, hist, tokens, last, done, alive, None, adv, 5, 1),          # p + U + 2 > ld
                 lambda: ops.whisper_accept(cand[:, :1], logp[:, :1], hist, tokens, last, done, alive, None, adv, 3, 1),   # U = 0
                 lambda: ops.whisper_accept(cand, logp, hist[:1], tokens, last, done, alive, None, adv, 3, 1),      # rows
                 lambda: ops.whisper_accept(cand, logp, hist, tokens, last, done, alive, torch.zeros(3).cuda(), adv, 3, 1)):
        with pytest.raises(F5EError):
            call()
    torch.cuda.synchronize()
    assert all(bool((t == -5).all()) for t in (hist, tokens, last, done, alive, adv))


# ---- the model ------------------------------------------------------------------------------------------------------------------------

def draft_of(model, kind, key):
    """The drafts of a target on the device: itself, its decoder with seeded noise, a seeded random model of its shapes."""
    if kind == "self":
        return model
    if (key, kind) not in _dev:
        from f5e_tts_amd.eval.whisper import Whisper
        sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
        sd = AR.noisy_decoder_sd(sd) if kind == "noisy" else AR.random_sd(sd)
        d = Whisper(model.cfg)
        d.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
        _dev[(key, kind)] = d.cuda()
    return _dev[(key, kind)]


def short_model(eos_case):
    if ("short", eos_case) not in _dev:
        _dev[("short", eos_case)] = WC.tiny_model(eos_case).cuda()
    return _dev[("short", eos_case)]


def fixture_draft():
    if "fixture" not in _dev:
        from f5e_tts_amd.eval.whisper import Whisper, WhisperConfig
        fx = AR.load_fixture()
        d = Whisper(WhisperConfig.from_dicts(fx["config"], WC.gold()["generation_config"]))
        d.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in fx["sd"].items()})
        _dev["fixture"] = d.cuda()
    return _dev["fixture"]


def short_wave(n):
    return torch.from_numpy(WC.gold()["wave_f32"][:n].copy()).cuda()[None]


@pytest.mark.parametrize("kind", ("self", "noisy", "random", "fixture"))
@pytest.mark.parametrize("case", ("14400", "40000", "48000", "eos"))
def test_generate_with_an_assistant_equals_generate_without(case, kind):
    """These fail without the feature.  The fixture's draft has another width and its own encoder; 4 drafts per round with it, as
    the fixture was made, 5 otherwise."""
    eos_case, n = case == "eos", 14400 if case == "eos" else int(case)
    model, w = short_model(eos_case), short_wave(n)
    want = WC.gold()[f"tokens_{case}"].tolist()
    base_t, base_n = model.generate(w, None, "en")
    assert base_t[0, :int(base_n[0])].tolist() == want
    draft = fixture_draft() if kind == "fixture" else draft_of(model, kind, ("short", eos_case))
    N, stats = (4 if kind == "fixture" else 5), {}
    tokens, length = model.generate(w, None, "en", assistant=draft, num_assistant_tokens=N, stats=stats,
                                    assistant_shares_encoder=kind == "self")
    assert torch.equal(tokens, base_t) and torch.equal(length, base_n)
    a, picks = stats["assistant"], int(base_n[0]) - 4
    print(f"case {case}, draft {kind}: {a}")
    assert all(isinstance(v, int) for v in a.values()) and a["accepted"] <= a["drafted"]
    # a round advances by what it accepted plus the target's own token (a drafted and accepted eos takes the column behind it too)
    assert picks <= a["rounds"] + a["accepted"] <= picks + 1
    if kind == "self":                                                   # only the last round can fall short
        assert a["drafted"] - a["accepted"] <= N
    if kind == "random":
        assert a["accepted"] == 0 and a["rounds"] == picks
    if kind == "fixture":                                                # the bound the fixture was made with
        c = [c for c in AR.load_fixture()["cases"] if c["name"] == case][0]
        cut = model.generate(w, None, "en", assistant=draft, num_assistant_tokens=N, max_new_tokens=c["max_new_tokens"])
        assert cut[0][0, :int(cut[1][0])].tolist() == c["tokens"]


def test_assistant_none_is_bit_identical_to_not_naming_it():
    model, w = short_model(False), short_wave(40000)
    a, b = model.generate(w, None, "en"), model.generate(w, None, "en", assistant=None, num_assistant_tokens=3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    model, _ = long_model("a")
    kv = model.encode(torch.from_numpy(LC.case_wave(LC.case("a")).copy()).cuda()[None, :16000])
    prompt, s1, s2 = model.prompt_ids("en", "transcribe", timestamps=True), {}, {}
    a = model.generate_from_kv(kv, prompt, return_timestamps=True, stats=s1)
    b = model.generate_from_kv(kv, prompt, return_timestamps=True, stats=s2, assistant=None, num_assistant_tokens=3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and "assistant" not in s2
    assert torch.equal(s1["no_speech_logp"], s2["no_speech_logp"]) and torch.equal(s1["sum_logp"], s2["sum_logp"])
    assert run_long("f") == run_long("f", assistant=None)                # dataclass equality: every float bit for bit


def long_model(name):
    rs = ("long", tuple(tuple(r) for r in LC.case(name)["row_scale"]))
    if rs not in _dev:
        _dev[rs] = LC.tiny_model(name).cuda()
    return _dev[rs], rs


def run_long(name, rows=None, kind=None, **kw):
    """transcribe_long, greedy, on a case's recordings (one ragged batch, garbage beyond a row's length)."""
    c = LC.case(name)
    rows = list(range(len(c["frames"]))) if rows is None else rows
    waves = [LC.case_wave(c, b) for b in rows]
    batch = torch.full((len(rows), max(len(w) for w in waves) + 37), 0.7)
    for i, w in enumerate(waves):
        batch[i, :len(w)] = torch.from_numpy(w.copy())
    model, key = long_model(name)
    if kind is not None:
        kw["assistant"] = draft_of(model, kind, key)
    return model.transcribe_long(batch.cuda(), [len(w) for w in waves], language="en", no_speech_threshold=c.get("no_speech_threshold"),
                                 logprob_threshold=c.get("logprob_threshold"), **kw)


def same_segments(got, want):
    """Tokens, boundaries, seeks and temperatures equal; the figures within the gate."""
    assert [(s.tokens, s.start_s, s.end_s, s.seek, s.temperature, s.compression_ratio) for s in got] == \
        [(s.tokens, s.start_s, s.end_s, s.seek, s.temperature, s.compression_ratio) for s in want]
    worst = 0.0
    for s, q in zip(got, want):
        worst = max(worst, abs(s.avg_logprob - q.avg_logprob) / abs(q.avg_logprob), abs(s.no_speech_prob - q.no_speech_prob) / q.no_speech_prob)
    assert worst < GATE, worst
    return worst


@pytest.mark.parametrize("kind", ("self", "noisy", "random"))
@pytest.mark.parametrize("name", tuple("abcdefgh"))
def test_transcribe_long_with_an_assistant_equals_the_run_without(name, kind):
    """Cases (a) .. (h) of whisper_long.npz, decoded greedily on both sides ((h) is the fixture's beam case: its model and wave).
    The fixture's own draft has 128 mel bins and these models 80, so it cannot read these windows: it is run on the short cases."""
    c = LC.case(name)
    base = run_long(name)
    if c.get("num_beams", 1) == 1:
        for b in range(len(c["frames"])):
            assert [s.tokens for s in base[b]] == [s["tokens"] for s in c["segments"][b]]
    got = run_long(name, kind=kind, assistant_shares_encoder=kind == "self")
    worst = max([same_segments(g, w) for g, w in zip(got, base)] + [0.0])
    print(f"case {name}, draft {kind}: avg_logprob / no_speech_prob within {worst:.2e} (gate {GATE:g})")


def test_a_batch_of_two_recordings_equals_its_rows_own_runs():
    both = run_long("f", kind="noisy")
    for b in range(2):
        same_segments(run_long("f", rows=[b], kind="noisy")[0], both[b])
        same_segments(run_long("f", rows=[b])[0], both[b])


@pytest.mark.parametrize("ts", (False, True))
def test_stats_and_token_timestamps_compose(ts):
    """sum_logp and no_speech_logp within the gate of the run without an assistant; the token times are those of the tokens."""
    model, key = long_model("a")
    w = torch.from_numpy(LC.case_wave(LC.case("a")).copy()).cuda()[None, :16000]
    kv = model.encode(w)
    prompt = model.prompt_ids("en", "transcribe", timestamps=ts)
    draft = draft_of(model, "noisy", key)
    s0, s1 = {}, {}
    base = model.generate_from_kv(kv, prompt, return_timestamps=ts, stats=s0)
    got = model.generate_from_kv(kv, prompt, return_timestamps=ts, stats=s1, assistant=(draft, draft.encode(w)), num_assistant_tokens=3)
    assert torch.equal(base[0], got[0]) and torch.equal(base[1], got[1])
    assert abs(float(s1["no_speech_logp"][0]) - float(s0["no_speech_logp"][0])) <= GATE * abs(float(s0["no_speech_logp"][0]))
    if ts:
        assert abs(float(s1["sum_logp"][0]) - float(s0["sum_logp"][0])) <= GATE * abs(float(s0["sum_logp"][0]))
    else:
        assert s1["sum_logp"] is None and s0["sum_logp"] is None
    if model.cfg.alignment_heads:
        t0 = model.generate_from_kv(kv, prompt, return_timestamps=ts, return_token_timestamps=True)[-1]
        t1 = model.generate_from_kv(kv, prompt, return_timestamps=ts, return_token_timestamps=True, assistant=(draft, draft.encode(w)))[-1]
        assert torch.equal(t0, t1)


@pytest.mark.parametrize("name,rows", (("a", [0]), ("e", [0, 1])))
def test_prompt_conditioning_and_ragged_prompts_with_an_assistant(name, rows):
    """whisper_prompt.npz: (a) conditioning on the previous text, (e) two rows left-padded to a common prompt length (``begin``);
    both models prefill the same padded prompt."""
    import test_whisper_prompt_cpu as PC
    c, fx = PC.case(name), PC.gold()
    key = ("prompt", tuple(tuple(r) for r in c["row_scale"]))
    if key not in _dev:
        _dev[key] = PC.tiny_model(c).cuda()
    model = _dev[key]
    waves = [fx["wave_f32"][c["waves"][b][0]:c["waves"][b][1]] for b in rows]
    batch = torch.full((len(rows), max(len(w) for w in waves)), 1e4, dtype=F32)
    for i, w in enumerate(waves):
        batch[i, :len(w)] = torch.from_numpy(w.copy())
    kw = dict(beam_size=1, context=PC.context_of(c))
    if c.get("no_speech_threshold") is not None:
        kw.update(no_speech_threshold=c["no_speech_threshold"], logprob_threshold=c["logprob_threshold"])
    base = model.transcribe_long(batch.cuda(), [len(w) for w in waves], "en", **kw)
    if c["num_beams"] == 1:
        for i, b in enumerate(rows):
            assert [s.tokens for s in base[i]] == [s["tokens"] for s in c["segments"][b]]
    for kind in ("self", "noisy"):
        got = model.transcribe_long(batch.cuda(), [len(w) for w in waves], "en", assistant=draft_of(model, kind, key), **kw)
        for g, w_ in zip(got, base):
            same_segments(g, w_)


def test_fallback_keeps_its_temperatures_with_an_assistant():
    """A case of whisper_fallback.npz whose windows fall back: the temperature-0 attempts are assisted, the sampled ones take the
    existing path, and attempts, kept temperatures and tokens are unchanged."""
    from f5e_tts_amd.eval.whisper import Fallback
    from test_whisper_fallback_cpu import fb_case, fb_gold, fb_model
    fx = fb_gold()
    c = fb_case("f")                                                     # three windows, the last one falls back to 0.2
    key = ("fb", c["name"])
    if key not in _dev:
        _dev[key] = fb_model(c).cuda()
    model = _dev[key]
    w = fx["wave_f32"][c["waves"][0][0]:c["waves"][0][1]]
    batch = torch.from_numpy(w.copy()).cuda()[None]
    fb = Fallback(tuple(c["temperatures"]), c["compression_ratio_threshold"], c["logprob_threshold"], c["seed"])

    def run(**kw):
        trace = []
        out = model.transcribe_long(batch, [len(w)], language="en", no_speech_threshold=c["no_speech_threshold"], fallback=fb,
                                    row_keys=[c["row_key"]], trace=trace, **kw)
        return out[0], [(t["seek"], t["temperature"], t["needs_fallback"], t["should_skip"]) for t in trace]
    base, attempts = run()
    assert any(t[1] > 0 for t in attempts) and [s.tokens for s in base] == [s["tokens"] for s in c["segments"]]
    got, attempts2 = run(assistant=draft_of(model, "noisy", key))
    assert attempts2 == attempts and [s.temperature for s in got] == [s.temperature for s in base]
    same_segments(got, base)
