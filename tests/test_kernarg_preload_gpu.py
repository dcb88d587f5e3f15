"""Marshalling of the kernels that take their hot arguments twice: as leading scalar parameters (preloaded into SGPRs at wave
launch: csrc/Makefile PRELOAD_UNITS, tools/check_kernarg_preload.py) and inside the argument struct behind them.

The new hazard is a scalar in the wrong slot, which only shows when the swapped fields differ: every case keeps the preloaded
fields pairwise distinct where the shapes allow it (lda = K + 8, ldw = K + 16, M != N != K in the K = 256 cases, tiles_m !=
tiles_n, n_main different from all of them, rows_per_seq != n_pad != H, kv_len per sequence).  Every case is launched once
eagerly and once from a captured graph that is replayed twice -- a graph owns a copy of the kernel arguments -- and the three
outputs must be equal byte for byte, whole buffers (sentinels around the views included).

bf16 GEMM (tests/gemm_bf16_ref.py, the helpers of tests/test_gemm_bf16_gpu.py): one case per instantiation of the 64-row
tile families and the two 128-wide classic tiles at M = 130 (three row tiles of 64, the last ragged), N = 128 (384 on the
64 x 192 consumer), K = 128, plus K = 256 / N = 384 variants for distinct N and K, the other tile walk (m_major <= 0 for M <=
N, 1 for M > N) and tiles_m != tiles_n on every tile.  Bit for bit against the reference for the exact epilogues.  What the
issue's shapes cannot reach, and what stands in for it:
  * the fused-AdaLN consumers (64 x 192, 64 x 128, classic 64 x 64) refuse K = 128 (statistics parts % 4 == 0: K % 256 == 0)
    and are not exact by construction (rsqrt, Chan's merge): K = 256, the ``gated`` yardstick of test_gemm_bf16_gpu.test_consumer;
  * the 4-stage classic tiles need K >= 2048;
  * prefetch workgroups behind n_main exist only inside f5e_dit_forward (the hints are not part of the C ABI, which does not
    change): tests/test_dit_chain_gpu.py runs every hosting launch with and without them against the op-by-op assembly, bit for
    bit, and the sampler with prefetch off and on, eagerly and from graphs.  The cases here launch without them.
Attention: S = 2, H = 3, N = 70, n_pad 128 and 192, ldo = 64 H and 64 H + 40, kv_len None and {70, 33}; 4 splits (the batch-1
kernel) and 1 / 2 splits (the general kernel) against the fp32 softmax of tests/test_attention_batch1_gpu.py; the batch-1
kernel and attn_fwd_kernel<4> share no shape in the shipped dispatch (N <= 512 / N > 512), so the bit-for-bit comparison is
between paddings and output strides of one kernel, where n_pad or ldo in a wrong slot shows.
convpos and the K = 100 input projection at S = 2, N = 70 against tests/frontend_ops_ref.py / an fp64 product."""
import ctypes as C

import pytest
import torch

import frontend_ops_ref as FR
import gemm_bf16_ref as R
import test_attention_batch1_gpu as AT
import test_gemm_bf16_gpu as G
from test_fp32_ops_gpu import Placed, gated, vector1d
from test_ops_gpu import close, pack_qkv

pytestmark = pytest.mark.gpu

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
SENT = R.SENTINEL


@pytest.fixture(scope="module")
def ops():
    import f5e_tts_amd.ops as ops_mod
    ops_mod.require_device()
    return ops_mod


def three_ways(ops, launch, outs, before=()):
    """``launch`` once eagerly, then captured in a graph that is replayed twice; before each run every buffer of ``outs`` is set
    back to its initial bytes (and the (buffer, initial) pairs of ``before`` restored: in-place operands).  Returns the three
    lists of host copies after asserting that they are equal byte for byte."""
    init = [o.clone() for o in outs]

    def reset():
        for o, i in zip(outs, init):
            o.copy_(i)
        for b, i in before:
            b.copy_(i)

    def snap():
        torch.cuda.current_stream().synchronize()
        return [o.cpu() for o in outs]

    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        reset()
        launch()
        runs = [snap()]
        reset()
        gr = ops.Graph()
        gr.begin()
        try:
            launch()
        finally:
            gr.end()
        for _ in range(2):
            reset()
            gr.launch()
            runs.append(snap())
        gr.destroy()
    torch.cuda.synchronize()
    for i, r in enumerate(runs[1:]):
        for a, b in zip(runs[0], r):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"graph replay {i + 1} differs from the eager launch"
    return runs


# ------------------------------------------------------------------ bf16 GEMM

def _b(epi, N, K, hint, M=130):
    return R.Case(epi, M, N, K, hint=hint, out="f32" if epi == "f32" else "bf16")


GEMM_EXACT = (
    # classic 64 x 64, 3 stages: the final projection's tile (f32 out), both walks
    (_b("f32", 128, 128, 3), R.T64_3), (_b("bf16", 128, 256, 3), R.T64_3), (_b("f32", 384, 128, 3), R.T64_3),
    (_b("bf16", 128, 2048, 3), R.T64_4),
    (_b("bf16", 128, 128, 1), R.T128), (_b("bf16", 384, 256, 1), R.T128),
    (_b("bf16", 128, 128, 2), R.T128X64), (_b("f32", 384, 256, 2), R.T128X64),
    # gate + residual: role split, and the fused-AdaLN producers
    (R._gate(130, 128, 128, 65), R.GATE_RS), (R._gate(130, 384, 256, 65, masked=True, evalp=True), R.GATE_RS),
    (R._prod(130, 128, 128, 65), R.PROD_RS6), (R._prod(130, 384, 256, 65, masked=True, evalp=True), R.PROD_RS6),
    (R._prod(130, 128, 192, 65), R.PROD_RS4),
    (R._prod(130, 128, 128, 65, gate_rows=2), R.PROD_C3), (R._prod(130, 128, 2048, 65, gate_rows=2), R.PROD_C4),
    # QKV without RoPE on the classic tile
    (R._qkv(130, 2, 128, 65, hint=3), R.T64_3), (R._qkv(450, 2, 256, 225, hint=3), R.T64_3),
)
GEMM_CONSUMERS = (
    (R._cons("qkv", 130, 384, 256, 65), R.CONS_QKV), (R._cons("qkv", 450, 384, 256, 225), R.CONS_QKV),
    (R._cons("f32", 130, 128, 256), R.CONS_WIDE), (R._cons("bf16", 130, 512, 256), R.CONS_WIDE),
    (R._cons("f32", 130, 320, 256), R.CONS_C3),
)


def test_the_cases_reach_their_instantiations_with_distinct_fields():
    walks = set()
    for c, inst in GEMM_EXACT + GEMM_CONSUMERS:
        p = R.case_path(c)
        assert p.inst == inst, f"{R.cid(c)}: {R.NAME_OF[p.inst]}, not {R.NAME_OF[inst]}"
        lda, ldw = c.K + 8, c.K + 16
        assert len({lda, ldw, c.K}) == 3 and p.n_tiles not in (c.M, c.N, c.K, lda, ldw)
        assert p.tiles_m != p.tiles_n or (c.N, c.K) == (128, 128), R.cid(c)     # the issue's N = 128 on the 128 x 64 tile: 2 x 2
        walks.add((inst, p.walk))
    for inst in (R.T64_3, R.T128, R.T128X64, R.GATE_RS, R.PROD_RS6, R.CONS_QKV, R.CONS_WIDE):
        assert {(inst, "m_major"), (inst, "grouped")} <= walks, f"{R.NAME_OF[inst]}: both signs of m_major"


@pytest.mark.parametrize("c", [c for c, _ in GEMM_EXACT], ids=R.cid)
def test_gemm_exact_eager_and_graph(ops, c):
    o = G.Operands(c)
    if c.epi == "qkv":
        cs = R.rope_table(c.rps).cuda()
        b = G.QkvBuffers(c)
        want = R.pre_activation(c).float()
        want[:, :c.N // 3] = want[:, :c.N // 3] * torch.tensor(R.QSCALE, dtype=F32)
        three_ways(ops, lambda: ops.gemm_bf16_qkv_rope(o.A.v, o.W.v, o.bias, b.q, b.k, b.vt, b.heads, c.rope_heads, cs, c.rps,
                                                       tile_hint=c.hint), [b.dflat])
        assert b.same_but(want), G.describe(c)
    elif c.epi == "gate":
        x0 = R.gate_operands(c)[0]
        ns = R.producer_operands(c)[1] if c.fuse else None
        full, d, gate, nsv, ev, sl = G.gate_tables(c, ns)
        resid = Placed(x0, 4, c.N + 8)
        outs, ln = [resid.dflat], None
        if c.fuse:
            rm = R.producer_operands(c)[0]
            xs_out = Placed(torch.full((c.M, c.N), SENT, dtype=BF), 8, c.N + 12)
            st = torch.full((c.M + 2, c.N // 64, 2), SENT, device="cuda")
            rm_flat, rm_dev, rm_v = vector1d(rm, 0)
            ln = ops.ln_producer(xs_out.v, nsv, st, rm_v)
            outs += [xs_out.dflat, st, rm_dev]
        three_ways(ops, lambda: ops.gemm_bf16_gate_residual(o.A.v, o.W.v, o.bias, resid.v, gate, c.rps, seq_len=sl, eval_ptr=ev,
                                                            eval_stride=d.stride(0) if c.evalp else 0, tile_hint=c.hint, ln=ln), outs)
        if c.fuse:
            x_new, xs, mean, _ = R.producer_expect(c)
            assert resid.same_but(x_new.float()) and xs_out.same_but(xs.float().to(BF)), G.describe(c)
            assert torch.equal(st.cpu()[:c.M, :, 0], mean.float()) and torch.equal(rm_dev.cpu(), rm_flat)
        else:
            assert resid.same_but(R.gate_expect(c).float()), G.describe(c)
        assert torch.equal(d.cpu(), full)
    else:
        dtype = F32 if c.epi == "f32" else BF
        out = G.out_placed(c, dtype)
        three_ways(ops, lambda: ops.gemm_bf16_bias(o.A.v, o.W.v, o.bias, out.v, tile_hint=c.hint), [out.dflat])
        assert out.same_but(R.pre_activation(c).float().to(dtype)), G.describe(c)
    assert o.unchanged(), "an input operand changed"


@pytest.mark.parametrize("c", [c for c, _ in GEMM_CONSUMERS], ids=R.cid)
def test_gemm_consumer_eager_and_graph(ops, c):
    """The gate of test_gemm_bf16_gpu.test_consumer (4 x the fp32 restatement's error against fp64, + one fp32 ulp, + 2^-8
    relative behind a bf16 store); row_mean is updated in place, so it is restored before every run."""
    o = G.Operands(c)
    stats, rm, cc, dd = R.consumer_operands(c)
    (pre, mean), (pre32, mean32) = R.consumer_expect(c), R.consumer_expect(c, F32)
    st = torch.full((c.M + 2, c.K // 64, 2), SENT)
    st[:c.M] = stats
    cd = torch.full((2, 1, c.N + 8), SENT)
    cd[0, 0, 4:4 + c.N], cd[1, 0, 4:4 + c.N] = cc, dd
    std, cdd = st.cuda(), cd.cuda()
    rm_flat, rm_dev, rm_v = vector1d(rm, 0)
    ln = ops.ln_consumer(std, cdd[0, :, 4:4 + c.N], cdd[1, :, 4:4 + c.N], c.rps, rm_v)
    if c.epi == "qkv":
        cs = R.rope_table(c.rps).cuda()
        b = G.QkvBuffers(c)
        three_ways(ops, lambda: ops.gemm_bf16_qkv_rope(o.A.v, o.W.v, None, b.q, b.k, b.vt, b.heads, c.rope_heads, cs, c.rps,
                                                       tile_hint=c.hint, ln=ln), [b.dflat, rm_dev])
        got = b.values()
        ref, ref32 = pre.clone(), pre32.clone()
        ref[:, :c.N // 3] *= R.QSCALE
        ref32[:, :c.N // 3] *= torch.tensor(R.QSCALE, dtype=F32)
        gated(G.describe(c), got, ref, ref32, rel_extra=G.BF_ULP)
        assert b.same_but(got)
    else:
        out = G.out_placed(c, F32 if c.epi == "f32" else BF)
        three_ways(ops, lambda: ops.gemm_bf16_bias(o.A.v, o.W.v, None, out.v, tile_hint=c.hint, ln=ln), [out.dflat, rm_dev])
        gated(G.describe(c), out.v.float(), pre, pre32, rel_extra=0.0 if c.epi == "f32" else G.BF_ULP)
        assert out.same_but(out.v.cpu())
    rm_got = rm_dev.cpu()
    gated(G.describe(c) + " row_mean", rm_got[:c.M], rm.double() + mean, rm + mean32)
    assert torch.equal(rm_got[c.M:], rm_flat[c.M:]) and o.unchanged() and torch.equal(std.cpu(), st) and torch.equal(cdd.cpu(), cd)


# ------------------------------------------------------------------ attention

A_S, A_H, A_N = 2, 3, 70


@pytest.fixture(scope="module")
def attn_case():
    q = (torch.randn(A_S, A_H, A_N, 64, generator=AT.g(50)) * AT.QSCALE).to(BF)
    k = torch.randn(A_S, A_H, A_N, 64, generator=AT.g(51)).to(BF)
    v = torch.randn(A_S, A_H, A_N, 64, generator=AT.g(52)).to(BF)
    lens = torch.tensor([70, 33], dtype=I32)
    kr, vr = k.clone(), v.clone()
    kr[1, :, 33:], vr[1, :, 33:] = AT.PAST, -AT.PAST

    def ref(kk, vv, ll):
        s = (q.float() @ kk.float().transpose(-1, -2)) * 0.6931471805599453
        if ll is not None:
            km = torch.arange(A_N)[None, :] < ll[:, None]
            s = s.masked_fill(~km[:, None, None, :], float("-inf"))
        return (torch.softmax(s, -1) @ vv.float()).transpose(1, 2).reshape(A_S * A_N, A_H * 64)

    return {False: (q, k, v, None, ref(k, v, None)), True: (q, kr, vr, lens, ref(kr, vr, lens))}


@pytest.mark.parametrize("waves", [4, 2, 1], ids=["batch1_4_splits", "general_2_splits", "general_1_split"])
@pytest.mark.parametrize("ragged", [False, True], ids=["kv_len_none", "kv_len_70_33"])
def test_attention_eager_and_graph(ops, attn_case, ragged, waves):
    q, k, v, lens, ref = attn_case[ragged]
    results = {}
    for n_pad, pad_o in ((128, 0), (128, 40), (192, 40)):
        qd, kd, vtd = pack_qkv(ops, q, k, v, n_pad)
        buf = torch.full((A_S * A_N + 2, A_H * 64 + pad_o), SENT, device="cuda", dtype=BF)
        out = buf[:A_S * A_N, :A_H * 64]
        ld = lens.cuda() if lens is not None else None
        assert out.stride(0) == A_H * 64 + pad_o and len({A_N, n_pad, A_H, out.stride(0)}) == 4
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None    # noqa: E731

        def launch():   # the C entry itself: ops.flash_attn takes a contiguous out only
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            ops.check(ops.lib().f5e_flash_attn(st, P(qd), P(kd), P(vtd), P(out), out.stride(0), P(ld), A_S, A_H, A_N, n_pad, waves),
                      "f5e_flash_attn")

        three_ways(ops, launch, [buf])
        got = buf.cpu()
        assert bool((got[A_S * A_N:] == SENT).all()) and bool((got[:, A_H * 64:] == SENT).all()), "written outside the view"
        close(got[:A_S * A_N, :A_H * 64].float(), ref, AT.RTOL, AT.ATOL)
        results[(n_pad, pad_o)] = got[:A_S * A_N, :A_H * 64].clone()
    first = results[(128, 0)]
    assert all(torch.equal(first, r) for r in results.values()), "the result depends on n_pad or ldo"


# ------------------------------------------------------------------ convpos and the per-step input projection

def test_convpos_eager_and_graph(ops):
    """S = 2, N = 70 on the split-tap kernel (16 groups x 2 tiles x 2 sequences on one round): mode 0 and mode 1, all of D, N, ldx,
    ldr, cpg, the two modes and the four strides distinct; against the exact pre-activation of tests/frontend_ops_ref.py."""
    D, Gr, N, S = 1024, 16, 70, 2
    x, w, bias, _ = FR.convpos_inputs(D, Gr, N)
    pre = FR.convpos_pre(x, w, bias, Gr)
    ref64, ref32 = FR.mish(pre), FR.mish(pre, F32)
    arg = pre.abs().clamp(max=20.0)
    res = torch.randn(S, N, D, generator=FR.g(77))
    wp, bd = ops.pack_convpos_weight(w, Gr).cuda(), bias.cuda()
    xin = Placed(x.reshape(S * N, D).to(BF), 8, D + 8)
    rin = Placed(res.reshape(S * N, D), 4, D + 12)
    o16 = Placed(torch.full((S * N, D), SENT, dtype=BF), 8, D + 16)
    o32 = Placed(torch.full((S * N, D), SENT), 4, D + 20)
    assert len({N, D, D // Gr, xin.v.stride(0), rin.v.stride(0), o16.v.stride(0), o32.v.stride(0)}) == 7

    def both():
        ops.convpos(xin.v, wp, bd, S, N, out_bf16=o16.v)
        ops.convpos(xin.v, wp, bd, S, N, out_f32=o32.v, resid=rin.v)

    three_ways(ops, both, [o16.dflat, o32.dflat])
    r64, r32, a = (t.reshape(S * N, D) for t in (ref64, ref32, arg))
    yard = float((r32.double() - r64).abs().max())
    gate = 4 * yard + (2.0 ** -23 + a * 2.0 ** -23) * r64.abs()
    want = r64 + res.reshape(S * N, D).double()
    err = (o32.v.double().cpu() - want).abs()
    assert bool((err <= gate + 2.0 ** -23 * want.abs()).all()), f"mode 1: max err {float(err.max()):.3e}"
    lo, hi = FR.rn_bf16(r64 - gate).float(), FR.rn_bf16(r64 + gate).float()
    got0 = o16.v.float().cpu()
    assert bool(((got0 >= lo) & (got0 <= hi)).all()), "mode 0 outside the rounding interval"
    assert o16.same_but(o16.v.cpu()) and o32.same_but(o32.v.cpu()) and xin.same_but() and rin.same_but()


def test_input_projection_eager_and_graph(ops):
    """The per-step input projection's launch: K = 100 (two K-tiles, the second ragged) on the 32-row LDS-DMA kernel, M = S N =
    140, N = 1024, integer operands (every summation order gives the same fp32 number): bit for bit."""
    M, N, K = 140, 1024, 100
    a = torch.randint(-4, 5, (M, K), generator=FR.g(5)).float()
    w = torch.randint(-4, 5, (N, K), generator=FR.g(6)).float()
    bias = torch.randint(-8, 9, (N,), generator=FR.g(7)).float()
    A, W = Placed(a, 4, K + 4), Placed(w, 8, K + 12)
    out = Placed(torch.full((M, N), SENT), 4, N + 8)
    assert len({M, N, K, A.v.stride(0), W.v.stride(0), out.v.stride(0), (M + 31) // 32}) == 7
    bd = bias.cuda()
    three_ways(ops, lambda: ops.gemm_f32(A.v, W.v, bd, out=out.v), [out.dflat])
    want = (a.double() @ w.double().T + bias.double()).float()
    assert out.same_but(want) and A.same_but() and W.same_but()
