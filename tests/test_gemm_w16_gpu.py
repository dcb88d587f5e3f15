"""The fp32 GEMM family with a 16-bit weight (csrc/gemm_f32_w16.hip, csrc/w_load.h): f5e_gemm_f32_w16_skinny, f5e_gemm_f32_w16,
f5e_whisper_embed_w16 and f5e_whisper_embed_w16_dev against their fp32 siblings on the widened copy of the weight.

Widening fp16 / bf16 to fp32 is exact and the kernels are the fp32 kernels' bodies behind another loader, so there is no
tolerance anywhere in this file: every comparison is ``torch.equal``, and on the bit patterns too (which tells -0 from +0).

Weights are random BITS of the 16-bit type (finite ones), with zeros, both signs of the largest finite value and subnormals
(fp16 2^-24; bf16 with a zero exponent field, which widen to fp32 subnormals) planted in every matrix.  The activations lie in
[-1, 1), a row of W holds the largest value once (+ in even rows, - in odd ones) and nothing else beyond 2^14, so no sum
overflows into inf - inf: a NaN would make ``torch.equal`` useless."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, I32, BF, F16 = torch.float32, torch.int32, torch.bfloat16, torch.float16
WTYPES = (F16, BF)
GUARD = -7.25


@pytest.fixture(scope="module")
def ops():
    from f5e_tts_amd import ops as o
    o.require_device()
    return o


def err():
    from f5e_tts_amd import _C
    return _C.F5EError


def weight(dt, N, K, seed, ld=None):
    """[N, K] of random finite bits in ``dt`` (a view of an [N, ld] buffer) with the special values planted."""
    g = torch.Generator().manual_seed(seed)
    ld = K if ld is None else ld
    bits = torch.randint(0, 1 << 16, (N, ld), generator=g, dtype=torch.int32)
    if dt == F16:
        exp = (bits >> 10) & 0x1F
        bits = torch.where(exp == 0x1F, bits & ~(1 << 14), bits)                   # no inf / nan
        big, tiny = 0x7BFF, (0x0001, 0x8001, 0x03FF)                               # 65504; 2^-24, -2^-24, the largest subnormal
    else:
        # exponent field at most 140 (|w| < 2^14): the planted extremes are the only huge values of a row
        exp = (bits >> 7) & 0xFF
        bits = torch.where(exp > 140, bits & ~(1 << 14), bits)
        big, tiny = 0x7F7F, (0x0001, 0x8040, 0x007F)                               # zero exponent field: fp32 subnormals
    flat = bits.view(-1)
    special = (0x0000, 0x8000) + tiny
    for n in range(N):                                                             # one of each per row while K has room
        cols = torch.randperm(K, generator=g)[:len(special) + 1].tolist()
        for c, v in zip(cols, special + (big | (0x8000 if n & 1 else 0),)):       # the largest value: + in even rows, - in odd
            flat[n * ld + c] = v
    w16 = torch.from_numpy((bits & 0xFFFF).numpy().astype("uint16").view("int16")).view(dt)
    assert torch.isfinite(w16.float()).all()
    return w16.cuda()[:, :K]


def acts(M, K, seed, ld=None):
    g = torch.Generator().manual_seed(seed)
    ld = K if ld is None else ld
    return (torch.rand(M, ld, generator=g) * 2 - 1).cuda()[:, :K]


def same_bits(a, b):
    return torch.equal(a, b) and torch.equal(a.contiguous().view(I32), b.contiguous().view(I32))


def test_planted_values_survive_widening():
    """The weights of this file hold what the issue asks for, and ``float()`` (the reference's widening) keeps subnormals."""
    w = weight(F16, 3, 20, 0)
    assert (w.float() == 2.0 ** -24).any() and (w.float() == 65504.0).any() and (w.float() == -65504.0).any() and (w == 0).any()
    b = weight(BF, 3, 20, 0).float()
    sub = (b != 0) & (b.abs() < 2.0 ** -126)
    assert sub.any() and (b == torch.finfo(BF).max).any() and (b == -torch.finfo(BF).max).any()


# ---- skinny -----------------------------------------------------------------------------------------------------------------

def skinny_pair(ops, a, w, bias, act, addend, alias=False):
    """(w16 result, fp32-on-widened result), each inside its own guard-filled buffer with ldo > N; the guards are checked."""
    M, N = a.shape[0], w.shape[0]
    outs = []
    for fn, wt in ((ops.gemm_f32_w16_skinny, w), (ops.gemm_f32_skinny, w.float().contiguous())):
        buf = torch.full((M + 2, N + 5), GUARD).cuda()
        out = buf[1:M + 1, 2:N + 2]
        add = addend
        if alias:
            out.copy_(addend)
            add = out
        fn(a, wt, bias, out=out, act=act, addend=add)
        chk = buf.clone()
        chk[1:M + 1, 2:N + 2] = GUARD
        assert (chk == GUARD).all(), "a byte outside out changed"
        outs.append(out.clone())
    return outs


@pytest.mark.parametrize("M", (1, 3, 16))
@pytest.mark.parametrize("dt", WTYPES, ids=("fp16", "bf16"))
def test_skinny_equals_the_fp32_launch_on_the_widened_weight(ops, dt, M):
    for N in (1, 17, 40):
        for K in (4, 20, 260):
            a, w = acts(M, K, 10 * N + K, ld=K + 4), weight(dt, N, K, 7 * N + K, ld=K + 8)
            bias, addend = torch.randn(N).cuda(), torch.randn(M, N).cuda()
            for b, act, ad, alias in ((None, ops.ACT_NONE, None, False), (bias, ops.ACT_GELU_ERF, None, False),
                                      (bias, ops.ACT_NONE, addend, False), (bias, ops.ACT_GELU_ERF, addend, True),
                                      (None, ops.ACT_GELU_ERF, addend, True)):
                got, want = skinny_pair(ops, a, w, b, act, ad, alias)
                assert same_bits(got, want), (dt, M, N, K, b is not None, act, ad is not None, alias)


@pytest.mark.parametrize("dt", WTYPES, ids=("fp16", "bf16"))
def test_skinny_k_split_rows_independent_of_m_and_reproducible(ops, dt):
    N, K, M = 24, 1040, 16
    need = ops.gemm_f32_w16_skinny_workspace(N, K)
    assert need > 0 and need == ops.gemm_f32_skinny_workspace(N, K)
    a, w, bias = acts(M, K, 3), weight(dt, N, K, 4), torch.randn(N).cuda()
    addend = torch.randn(M, N).cuda()
    # the caller's workspace inside a guard-filled buffer: nothing beyond its bytes is written
    wsbuf = torch.full((need // 4 + 64,), GUARD).cuda()
    ws = wsbuf[32:32 + need // 4]
    out = torch.empty(M, N).cuda()
    ops.gemm_f32_w16_skinny(a, w, bias, out=out, act=ops.ACT_GELU_ERF, addend=addend, workspace=ws)
    assert (wsbuf[:32] == GUARD).all() and (wsbuf[32 + need // 4:] == GUARD).all()
    want = torch.empty(M, N).cuda()
    ops.gemm_f32_skinny(a, w.float(), bias, out=want, act=ops.ACT_GELU_ERF, addend=addend)
    assert same_bits(out, want)
    again = torch.empty(M, N).cuda()
    ops.gemm_f32_w16_skinny(a, w, bias, out=again, act=ops.ACT_GELU_ERF, addend=addend)          # the kept workspace
    assert same_bits(again, out)
    for m in (0, 5, 15):
        one = torch.empty(1, N).cuda()
        ops.gemm_f32_w16_skinny(a[m:m + 1], w, bias, out=one, act=ops.ACT_GELU_ERF, addend=addend[m:m + 1])
        assert same_bits(one[0], out[m]), m
    # and without the split
    a2, w2 = acts(M, 260, 5), weight(dt, 40, 260, 6)
    full, one = torch.empty(M, 40).cuda(), torch.empty(1, 40).cuda()
    ops.gemm_f32_w16_skinny(a2, w2, None, out=full)
    ops.gemm_f32_w16_skinny(a2[7:8], w2, None, out=one)
    assert same_bits(one[0], full[7])


# ---- general ----------------------------------------------------------------------------------------------------------------

def general_pair(ops, a, w, M, kw, want_f32=True, want_bf16=False):
    """Both ops on the same operands; ``out`` / ``out_bf16`` sit in guard-filled buffers with ldo > N, and the guards are checked."""
    N = w.shape[0]
    res = []
    for fn, wt in ((ops.gemm_f32_w16, w), (ops.gemm_f32, w.float().contiguous())):
        bufs, outs = [], {}
        for name, dt, want in (("out", F32, want_f32), ("out_bf16", BF, want_bf16)):
            if want:
                buf = torch.full((M + 2, N + 8), GUARD, dtype=dt).cuda()
                outs[name] = buf[1:M + 1, 4:N + 4]
                bufs.append(buf)
        fn(a, wt, kw.get("bias"), M=M, **{k: v for k, v in kw.items() if k != "bias"}, **outs)
        for buf in bufs:
            chk = buf.clone()
            chk[1:M + 1, 4:N + 4] = GUARD
            assert (chk == GUARD).all(), "a byte outside the output changed"
        res.append({k: v.clone() for k, v in outs.items()})
    return res


def general_same(got, want):
    return all((same_bits(got[k], want[k]) if want[k].dtype == F32 else torch.equal(got[k].view(torch.int16), want[k].view(torch.int16)))
               for k in want)


@pytest.mark.parametrize("M", (17, 65, 130))
@pytest.mark.parametrize("dt", WTYPES, ids=("fp16", "bf16"))
def test_general_equals_gemm_f32_on_the_widened_weight(ops, dt, M):
    """Both k orders of the fp32 entry point: a 16-byte aligned A without ``a_act`` goes to its LDS-DMA kernel, an A-side
    activation or an A offset by one element to the plain kernel; the w16 launch must follow each."""
    for N in (1, 63, 130):
        for K in (4, 36, 132):
            w = weight(dt, N, K, 3 * N + K, ld=K + 4)
            a = acts(M, K, N + 5 * K, ld=K + 4)
            bias, chs, rs = torch.randn(N).cuda(), torch.randn(N).cuda(), torch.randn(M).cuda()
            add1, addM = torch.randn(1, N).cuda(), torch.randn(M, N).cuda()
            a_small = acts(5, K, 11, ld=K + 4)                                   # a_rows < M: row m reads a[m % 5]
            a_off = torch.empty(M * (K + 4) + 1).cuda()[1:].view(M, K + 4)        # 4-byte aligned only: the plain kernel
            a_off.copy_(torch.as_strided(a, (M, K + 4), (K + 4, 1)))
            cases = [
                (a, dict(), True, False),
                (a, dict(bias=bias, act=ops.ACT_GELU_ERF), True, False),
                (a, dict(bias=bias, act=ops.ACT_SILU, ch_scale=chs, addend=add1, row_scale=rs), True, True),
                (a, dict(addend=addM, row_scale=rs), True, False),
                (a, dict(bias=bias, ch_scale=chs), False, True),
                (a_small, dict(bias=bias, addend=addM), True, False),
                (a, dict(a_act=ops.ACT_SILU, bias=bias), True, False),
                (a_small, dict(a_act=ops.ACT_SILU, act=ops.ACT_RELU, addend=add1), True, True),
                (a_off[:, :K], dict(bias=bias, act=ops.ACT_GELU_ERF, addend=addM), True, False),
            ]
            for i, (aa, kw, f, b) in enumerate(cases):
                got, want = general_pair(ops, aa, w, M, kw, f, b)
                assert general_same(got, want), (dt, M, N, K, i)


def test_general_takes_the_16_byte_friendly_epilogue(ops):
    """N % 4 == 0 with aligned outputs: the vector epilogue of the fp32 DMA kernel against the tile's scalar one."""
    for dt in WTYPES:
        M, N, K = 70, 64, 68
        a, w, bias, add = acts(M, K, 1), weight(dt, N, K, 2), torch.randn(N).cuda(), torch.randn(M, N).cuda()
        got, want = torch.empty(M, N).cuda(), torch.empty(M, N).cuda()
        ops.gemm_f32_w16(a, w, bias, out=got, act=ops.ACT_GELU_ERF, addend=add)
        ops.gemm_f32(a, w.float(), bias, out=want, act=ops.ACT_GELU_ERF, addend=add)
        assert same_bits(got, want)


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_leave_out_untouched(ops):
    E = err()
    M, N, K = 4, 24, 1040
    a, w = acts(M, K, 0), weight(F16, N, K, 1)
    out = torch.full((M, N), GUARD).cuda()
    bad = [
        lambda: ops.gemm_f32_w16_skinny(a, w.float(), None, out=out),                               # a float32 W
        lambda: ops.gemm_f32_w16(a, w.float(), None, out=out),
        lambda: ops.gemm_f32_skinny(a, w, None, out=out),                                           # a 16-bit W to the fp32 ops
        lambda: ops.gemm_f32(a, w, None, out=out),
        lambda: ops.gemm_f32_w16_skinny(acts(17, K, 0), w, None, out=torch.full((17, N), GUARD).cuda()),   # M = 17
        lambda: ops.gemm_f32_w16_skinny(a, weight(F16, N, K, 1, ld=K + 2), None, out=out),          # ldw % 4 != 0
        lambda: ops.gemm_f32_w16(a, weight(F16, N, K, 1, ld=K + 2), None, out=out),
        lambda: ops.gemm_f32_w16_skinny(a, torch.zeros(N * K + 1, dtype=F16).cuda()[1:].view(N, K), None, out=out),   # 2-byte aligned
        lambda: ops.gemm_f32_w16(a, torch.zeros(N * K + 1, dtype=F16).cuda()[1:].view(N, K), None, out=out),
        lambda: ops.gemm_f32_w16_skinny(a, w, None, out=out, act=ops.ACT_SILU),                     # an act that is not built
        lambda: ops.gemm_f32_w16_skinny(a, w, None, out=out, workspace=torch.empty(4).cuda()),      # a short workspace
    ]
    for i, f in enumerate(bad):
        with pytest.raises(E):
            f()
        assert (out == GUARD).all(), i
    # the library's own refusals, past the wrapper
    import ctypes as C
    from f5e_tts_amd import _C
    lib = _C.lib()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    assert lib.f5e_gemm_f32_w16_skinny(None, p(a), K, p(w), K, 7, None, 0, None, 0, p(out), N, None, 0, M, N, K) != 0        # wtype
    assert lib.f5e_gemm_f32_w16_skinny(None, p(a), K, p(w), K, _C.W_FP16, None, 0, None, 0, p(out), N, None, 0, 17, N, K) != 0
    assert lib.f5e_gemm_f32_w16_skinny(None, p(a), K, p(w), K, _C.W_FP16, None, 0, None, 0, p(out), N, None, 0, M, N, K) != 0  # no workspace
    assert lib.f5e_gemm_f32_w16_skinny(None, p(a), K, C.c_void_p(w.data_ptr() + 2), K, _C.W_FP16, None, 0, None, 0, p(out), N, None,
                                       0, M, 8, 16) != 0
    assert lib.f5e_gemm_f32_w16(None, p(a), K, M, 0, C.c_void_p(w.data_ptr() + 2), K, _C.W_BF16, None, 0, None, None, 0, 0, None,
                                p(out), N, None, 0, M, N, 16) != 0
    assert lib.f5e_gemm_f32_w16(None, p(a), K, M, 0, p(w), K + 2, _C.W_BF16, None, 0, None, None, 0, 0, None, p(out), N, None, 0, M,
                                N, 16) != 0
    torch.cuda.synchronize()
    assert (out == GUARD).all()


# ---- embed ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", WTYPES, ids=("fp16", "bf16"))
def test_embed_equals_the_fp32_gather_on_the_widened_table(ops, dt):
    R, U, D, V, P = 2, 3, 8, 5, 7
    emb = weight(dt, V, D, 9).contiguous()
    pos = torch.randn(P, D).cuda()
    ids = torch.tensor([[0, -1, 4], [5, 2, 3]], dtype=I32).cuda()                 # -1 and 5 are clamped
    for p0 in (0, P - U):                                                          # p0 + U at the edge of the table
        for begin in (None, torch.tensor([0, 2], dtype=I32).cuda()):
            buf = torch.full((R * U * D + 8,), GUARD).cuda()
            got = buf[4:4 + R * U * D].view(R, U, D)
            ops.whisper_embed_w16(ids, emb, pos, got, p0, begin)
            want = ops.whisper_embed(ids, emb.float(), pos, torch.empty(R, U, D).cuda(), p0, begin)
            assert same_bits(got, want) and (buf[:4] == GUARD).all() and (buf[-4:] == GUARD).all()
    # the device-position form: at a record position, and at one beyond the table (clamped)
    last = torch.tensor([4, -3], dtype=I32).cuda()
    for p, begin in ((3, None), (3, torch.tensor([1, 0], dtype=I32).cuda()), (P + 5, None)):
        rec = torch.zeros(ops.STEP_REC_WORDS, dtype=I32)
        rec[0] = p
        rec = rec.cuda()
        got = ops.whisper_embed_w16_dev(last, emb, pos, torch.empty(R, D).cuda(), rec, begin)
        want = ops.whisper_embed_dev(last, emb.float(), pos, torch.empty(R, D).cuda(), rec, begin)
        assert same_bits(got, want)
        if p < P:
            twin = ops.whisper_embed_w16(last.view(R, 1), emb, pos, torch.empty(R, 1, D).cuda(), p, begin)
            assert same_bits(got, twin.view(R, D))
    E = err()
    with pytest.raises(E):
        ops.whisper_embed_w16(ids, emb.float(), pos, torch.empty(R, U, D).cuda())
    with pytest.raises(E):
        ops.whisper_embed(ids, emb, pos, torch.empty(R, U, D).cuda())
    with pytest.raises(E):
        ops.whisper_embed_w16(ids, emb, pos, torch.empty(R, U, D).cuda(), P - U + 1)
