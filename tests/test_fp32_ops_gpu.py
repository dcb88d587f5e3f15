"""Direct parity of the fp32 GEMM, GRN, dwconv7 and im2col kernels: every HIP op, called through f5e_tts_amd.ops, against the
fp64 restatement of tests/fp32_ops_ref.py (pinned on the CPU by tests/test_fp32_ops_cpu.py) on the same seeded inputs.

Case -> path (kernel | epilogue | ring state; what nothing else in the suite executes).  dma32 = gemm_f32_dma_kernel<32, 64,
2, 2, 4> (NSTAGE 4), dma64 = gemm_f32_dma_kernel<64, 64, 2, 2, 3> (NSTAGE 3), plain = gemm_f32_kernel (K step 16, 2 buffers):
  test_gemm_misaligned_base          plain | scalar | KT 1, 1, 1, 2, 2, 3, 7 of 16 (K 4 .. 100), reached through an A or a W whose
                                     base is 4 bytes past a 16-byte boundary: the host's ``((A | W) & 15)`` test and the kernel's
                                     16-byte global loads from a 4-byte aligned address.  Run alone before the rest
  test_gemm_ring_32row               dma32 | vector (N 68) and scalar (N 67) | KT 1, 2 (< NSTAGE - 1: slots >= KT not allocated),
                                     3 (= NSTAGE - 1), 4 (= NSTAGE), 5, 6, 9 (> NSTAGE: slots reused); K % 64 = 4 (one live chunk
                                     in the tail), 60 (one dead chunk), 0 (no tail); every ring state with and without a tail
  test_gemm_ring_64row               dma64 | vector (449 x 1024: one row in the last M tile; 512 x 964: a partial last tile of
                                     quads) and scalar (450 x 961) | KT 1 (< NSTAGE - 1), 2, 3 (= NSTAGE), 4, 5, 7; 448 x 1152 x
                                     132: 126 tiles, the last shape that still takes dma32
  test_gemm_edges                    dma32 | M 1 .. 65 around the 32-row tile, N 1 .. 68 around the quad and the 64-column tile
                                     (vector for N 4, 60, 64, 68; scalar otherwise) | KT 2 with a tail
  test_gemm_epilogue_forms           dma32 | vector for ``out = buf[:, 4:4 + N]`` inside a wider buffer (engine.py's ``cd[:, off:off
                                     + n]``); scalar through exactly one broken condition: N 67, ldo, out base, out_bf16 base,
                                     ldo_bf16, bias base, ch_scale base, addend base, ld_add | out / out_bf16 / both, with and
                                     without bias, ch_scale, addend, row_scale (48 launches per form and activation)
  test_gemm_wraps                    dma32 | both epilogues | a_rows 13 under M 33, add_rows 1 / 3 / 33, row_scale with zeros
  test_gemm_in_place                 dma32 | both epilogues | addend is the out view itself (ppg_model.py's ``out=sc[:, :T],
                                     addend=sc[:, :T]``), M 33 and 65
  test_gemm_activations              dma32, dma64, plain | vector, vector, scalar | SILU, GELU_ERF, GELU_TANH, MISH on an exact
                                     argument within +-20: only the activation's own error is left
  test_gemm_a_side_silu              plain | scalar | a_act = SILU on aligned randn operands, K 64 (4 whole steps), 100, 260
  test_grn                           grn_norm4_kernel + vector apply: partial last 64-channel block (C 4, 68), 0 / 1 / 2 rows per
                                     row group and one / two trips of the loop unrolled by 8 (T 1 .. 241); grn_norm_kernel +
                                     scalar apply at C % 4 == 0 through a misaligned x or gamma; second grid-stride trip of
                                     grn_apply_kernel on both paths; an all-zero batch row; ws pre-filled with NaN
  test_dwconv7                       T 1 .. 7 (every tap pattern at the edges), B 3 (no tap crosses a batch boundary), second
                                     grid-stride trip (2 x 2100 x 1024 past 4096 x 256 quads)
  test_im2col[_past_the_grid_cap]    ksize 1 .. 31, pad 0 .. T + 2 (whole taps in the padding), T 1, Cin 1; second trip
  test_*_refusals, test_gemm_accepts_the_forms_of_the_tree    every host-side refusal (nothing is launched), and what must pass

Gates.  The integer GEMM cases, dwconv7 and im2col are exact in fp32 (checked on the CPU): ``torch.equal``, on the whole
sentinel-filled buffer behind each output view, so every element outside [0, M) x [0, N) is compared bit for bit too.  GRN and
the inexact activations follow tests/test_small_ops_gpu.py: the kernel's error against fp64 may be 4x the error of the same
restatement evaluated in fp32 on the CPU, plus one fp32 ulp of the result, plus |e| 2^-23 relative where e is the argument of
the activation's exponential (the rounding of e log2(e)); a bf16 copy adds its own rounding, 2^-8 relative.  The A-side SILU
cases use the standard summation bound, any order: (K + 8) 2^-24 (|actA(A)| |W|^T + |bias|), plus test_gemm_f32's 1e-5 relative
/ 3e-5 absolute for an epilogue activation.  Each gated test prints the yardstick and the kernel's error side by side."""
import ctypes as C

import pytest
import torch

import fp32_ops_ref as R

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ULP = 2.0 ** -23
SENT = R.SENTINEL


@pytest.fixture(scope="module")
def ops():
    import f5e_tts_amd.ops as ops_mod
    ops_mod.require_device()
    return ops_mod


@pytest.fixture(scope="module")
def F5EError():
    from f5e_tts_amd import _C
    return _C.F5EError


def dev(t):
    return t.cuda().contiguous()


def gated(what, got, ref64, ref32, rel_extra=0.0):
    """|kernel - fp64| <= 4 max|fp32 restatement - fp64| + (2^-23 + rel_extra) |fp64|, element by element (``gated`` of
    tests/test_small_ops_gpu.py; rel_extra may be a tensor)."""
    got, ref32 = got.double().cpu().reshape(ref64.shape), ref32.double().reshape(ref64.shape)
    yard = float((ref32 - ref64).abs().max())
    err = (got - ref64).abs()
    print(f"{what}: fp32 restatement vs fp64 {yard:.3e}, kernel vs fp64 {float(err.max()):.3e}")
    bad = ~(err <= 4 * yard + (ULP + rel_extra) * ref64.abs())
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} past the gate, max err {float(err.max()):.3e}, yardstick {yard:.3e}"


class Placed:
    """A [rows, cols] operand as a view at ``off`` with row stride ``ld`` inside a flat sentinel-filled device buffer (the
    ``in_buffer`` of tests/test_small_ops_gpu.py with a column offset); ``same_but`` is its ``untouched``: the whole buffer
    must equal the original with the view's [0, M) x [0, N) replaced by ``want``."""

    def __init__(self, t, off, ld):
        self.flat, self.spec = R.placed(t, off, ld)
        self.dflat = self.flat.cuda()
        self.v = R.view(self.dflat, self.spec)

    def same_but(self, want=None):
        exp = self.flat.clone()
        if want is not None:
            R.view(exp, self.spec).copy_(want)
        got = self.dflat.cpu()
        if torch.equal(got, exp):
            return True
        diff = torch.nonzero(got != exp).flatten()
        print(f"{diff.numel()} of {exp.numel()} elements differ, first at flat {diff[:8].tolist()} (view {self.spec}): got "
              f"{got[diff[:8]].tolist()}, want {exp[diff[:8]].tolist()}")
        return False


def vector1d(t, off):
    """t [n] as flat[off:off + n] of a sentinel-filled device buffer."""
    flat = torch.full((t.numel() + 8,), SENT)
    flat[off:off + t.numel()] = t
    d = flat.cuda()
    return flat, d, d[off:off + t.numel()]


_AW = {}


def device_aw(c, t):
    key = (c.M, c.N, c.K, c.a_rows, c.a_off, c.w_off, c.randn, c.act in R.INEXACT_ACTS)
    if key not in _AW:
        _AW.clear()
        _AW[key] = (Placed(t["A"], c.a_off, c.K + R.A_PAD), Placed(t["W"], c.w_off, c.K + R.W_PAD))
    return _AW[key]


def run_gemm(ops, c):
    """One launch of the case -> (reference fp64, operands, out Placed or None, out_bf16 Placed or None, path).  Asserts that
    the device pointers and leading dimensions are what the case claims and that the restated dispatch sends them down the
    claimed path, and afterwards that no input changed."""
    t = R.gemm_operands(c)
    A, W = device_aw(c, t)
    kw, off, lds = {}, dict(A=A.v.data_ptr() % 16, W=W.v.data_ptr() % 16, bias=0, ch_scale=0, addend=0, out=0, out_bf16=0), \
        dict(ldo=0, ldo_bf16=0, ld_add=0)
    keep = [A, W]
    out = outb = None
    if c.outs in ("f32", "both"):
        init = t["add"] if c.inplace else torch.full((c.M, c.N), SENT)
        out = Placed(init, c.out_off, c.N + c.out_pad)
        kw["out"], off["out"], lds["ldo"] = out.v, out.v.data_ptr() % 16, out.v.stride(0)
    if c.outs in ("bf16", "both"):
        outb = Placed(torch.full((c.M, c.N), SENT, dtype=BF), c.bf_off, c.N + c.bf_pad)
        kw["out_bf16"], off["out_bf16"], lds["ldo_bf16"] = outb.v, outb.v.data_ptr() % 8, outb.v.stride(0)
    if c.inplace:
        kw["addend"], off["addend"], lds["ld_add"] = out.v, off["out"], lds["ldo"]
    elif t["add"] is not None:
        add = Placed(t["add"], c.add_off, c.N + c.add_pad)
        keep.append(add)
        kw["addend"], off["addend"], lds["ld_add"] = add.v, add.v.data_ptr() % 16, add.v.stride(0)
    flats = []
    for name, key, o in (("bias", "bias", c.bias_off), ("ch_scale", "cs", c.cs_off)):
        if t[key] is not None:
            flat, d, v = vector1d(t[key], o)
            flats.append((flat, d))
            kw[name], off[name] = v, v.data_ptr() % 16
    if t["rs"] is not None:
        kw["row_scale"] = dev(t["rs"])
    bias = kw.pop("bias", None)
    claimed = R.case_layout(c)
    assert (off, lds) == claimed, f"layout moved: device {(off, lds)}, case {claimed}"
    path = R.gemm_f32_path(c.M, c.N, c.K, c.a_act, off, lds)
    assert path == R.case_path(c)
    ops.gemm_f32(A.v, W.v, bias, M=c.M, K=c.K, a_act=c.a_act, act=c.act, **kw)
    torch.cuda.synchronize()
    assert all(p.same_but() for p in keep) and all(torch.equal(d.cpu(), f) for f, d in flats), "an input operand changed"
    return R.gemm_ref(c, t), t, out, outb, path


def check_exact(ops, c):
    for act in R.EXACT_ACTS:
        ca = c._replace(act=act)
        ref, _, out, outb, path = run_gemm(ops, ca)
        exact = ref.float()
        assert out is None or out.same_but(exact), f"{R.cid(ca)} via {path}: out"
        assert outb is None or outb.same_but(exact.to(BF)), f"{R.cid(ca)} via {path}: out_bf16"
    return path


# ------------------------------------------------------------------ gemm_f32, exact

@pytest.mark.parametrize("c", R.MISALIGNED, ids=R.cid)
def test_gemm_misaligned_base(ops, c):
    assert check_exact(ops, c)[0] == "plain" and (c.a_off, c.w_off) in ((1, 0), (0, 1))


@pytest.mark.parametrize("c", R.RING32 + R.RING32_SCALAR, ids=R.cid)
def test_gemm_ring_32row(ops, c):
    assert check_exact(ops, c)[0] == "dma32"


@pytest.mark.parametrize("c", R.RING64, ids=R.cid)
def test_gemm_ring_64row(ops, c):
    assert check_exact(ops, c)[0] == ("dma64" if c.M != 448 else "dma32")


@pytest.mark.parametrize("c", R.EDGES, ids=R.cid)
def test_gemm_edges(ops, c):
    assert check_exact(ops, c)[:2] == ("dma32", c.N % 4 == 0)


@pytest.mark.parametrize("name", list(R.FORMS))
def test_gemm_epilogue_forms(ops, name):
    c, cond = R.FORMS[name]
    assert check_exact(ops, c)[1] == (cond is None)
    paths = {check_exact(ops, v)[1] for v in R.form_variants(c)}
    # without the offending operand the vector path is back; N % 4 != 0 offends in every variant
    assert paths == ({True} if cond is None else {False} if cond == "N" else {True, False})


@pytest.mark.parametrize("c", R.WRAPS, ids=R.cid)
def test_gemm_wraps(ops, c):
    check_exact(ops, c)


@pytest.mark.parametrize("c", R.INPLACE, ids=R.cid)
def test_gemm_in_place(ops, c):
    assert check_exact(ops, c)[1] == (c.N % 4 == 0)


# ------------------------------------------------------------------ gemm_f32, inexact paths

@pytest.mark.parametrize("c", R.ACT_CASES, ids=R.cid)
def test_gemm_activations(ops, c):
    """The small-ops gate with the exponential's own argument as the allowance (results up to 160 = 20 x 4 x 2).  Observed on
    one MI355X (fp32 restatement vs fp64 | kernel vs fp64), 33 x 68 x 196 on dma32: SILU 8.2e-6 | 8.2e-6, GELU_ERF 2.3e-6 |
    2.3e-6, GELU_TANH 3.2e-6 | 3.2e-6, MISH 5.4e-6 | 7.6e-6; 450 x 1024 x 132 on dma64: 8.1e-6 | 8.1e-6, 3.1e-6 | 3.1e-6,
    3.8e-6 | 3.8e-6, 5.4e-6 | 1.5e-5; 65 x 65 x 100 on the plain kernel: 6.0e-6 | 6.0e-6, 2.8e-6 | 2.8e-6, 3.8e-6 | 3.8e-6,
    5.2e-6 | 5.2e-6.  The bf16 copies: 0.24 .. 0.25, half a bf16 ulp of the largest results."""
    ref, t, out, outb, path = run_gemm(ops, c)
    ref32 = R.gemm_ref(c, t, dtype=F32)
    e = R.act_exp_arg(R.gemm_pre(c, t), c.act).abs()
    assert bool(torch.isfinite(out.v).all())
    gated(f"{R.cid(c)} via {path[0]} f32", out.v, ref, ref32, rel_extra=e * ULP)
    gated(f"{R.cid(c)} via {path[0]} bf16", outb.v.float(), ref, ref32, rel_extra=e * ULP + 2.0 ** -8)
    assert out.same_but(out.v.cpu()) and outb.same_but(outb.v.cpu())             # nothing outside the views


@pytest.mark.parametrize("c", R.A_ACT_CASES, ids=R.cid)
def test_gemm_a_side_silu(ops, c):
    """|err| <= (K + 8) 2^-24 (|silu(A)| |W|^T + |bias|), plus 1e-5 |ref| + 3e-5 when the epilogue has an activation.
    Observed on one MI355X (smallest gate | kernel vs fp64 | largest err / gate), bias only: 33 x 68 x 100 1.4e-5 | 8.3e-7 |
    0.029, 65 x 65 x 64 5.5e-6 | 6.1e-7 | 0.039, 130 x 100 x 260 5.9e-5 | 1.2e-6 | 0.016; with GELU_ERF: 4.5e-5 | 8.2e-7 |
    0.011, 3.7e-5 | 6.2e-7 | 0.009, 8.9e-5 | 1.3e-6 | 0.011."""
    ref, t, out, _, path = run_gemm(ops, c)
    assert path[0] == "plain"
    gate = (c.K + 8) * 2.0 ** -24 * R.gemm_abs_bound(c, t)
    if c.act != R.ACT_NONE:
        gate = gate + 1e-5 * ref.abs() + 3e-5
    err = (out.v.double().cpu() - ref).abs()
    print(f"{R.cid(c)}: smallest gate {float(gate.min()):.3e}, largest {float(gate.max()):.3e}, kernel vs fp64 "
          f"{float(err.max()):.3e}, largest err / gate {float((err / gate).max()):.3f}")
    assert bool((err <= gate).all()) and out.same_but(out.v.cpu())


# ------------------------------------------------------------------ GRN

@pytest.mark.parametrize("B,T,C,kind", R.GRN_CASES)
def test_grn(ops, B, T, C, kind):
    """No earlier gate at these shapes: 4x the fp32 restatement + one ulp, for the output and for gx in ws.  Observed on one
    MI355X (fp32 restatement vs fp64 | kernel vs fp64), output: C 68, T 1 3.3e-6 | 2.2e-6, 15 2.0e-6 | 2.0e-6, 16 2.3e-6 |
    1.9e-6, 17 2.3e-6 | 2.3e-6, 112 2.0e-6 | 2.8e-6, 113 3.2e-6 | 3.2e-6, 128 2.8e-6 | 2.1e-6, 129 2.1e-6 | 2.2e-6, 241
    2.7e-6 | 5.0e-6; C 4 6.1e-7 | 9.9e-7; misaligned x or gamma 1.2e-6 | 2.0e-6; (1, 1100, 1024) 5.6e-6 | 3.5e-6; (1, 4100,
    66) 4.0e-6 | 5.5e-6; zero row 1.9e-6 | 1.9e-6 (C 68), 2.0e-6 | 3.2e-6 (C 66).  gx: T 1 exact on both sides, otherwise
    7.5e-7 | 1.2e-6 (T 15) .. 1.5e-5 | 2.8e-5 ((1, 4100, 66): 1025 sequential adds per wave against the CPU's pairwise sum)."""
    x, gam, bet = R.grn_inputs(B, T, C, kind)
    n = x.numel()
    xflat = torch.full((n + 4,), SENT, device="cuda")
    xo = 1 if kind == "x1" else 0
    xd = xflat[xo:xo + n].view(B, T, C)
    xd.copy_(x)
    gflat = torch.full((C + 4,), SENT, device="cuda")
    go = 1 if kind == "g1" else 0
    gd = gflat[go:go + C]
    gd.copy_(gam)
    assert xd.data_ptr() % 16 == 4 * xo and gd.data_ptr() % 16 == 4 * go and xd.is_contiguous()
    vec, trips = R.grn_path(B, T, C, kind)
    assert vec == (C % 4 == 0 and xo == 0 and go == 0)
    ws = torch.full((B, C), float("nan"), device="cuda")
    out = torch.full((B, T, C), SENT, device="cuda")
    ops.grn(xd, out, gd, dev(bet), ws)
    ref, gx = R.grn(x, gam, bet, want_gx=True)
    ref32, gx32 = R.grn(x, gam, bet, dtype=F32, want_gx=True)
    assert bool(torch.isfinite(ws).all()) and bool(torch.isfinite(out).all())       # pass 1 wrote all of [B, C]
    gated(f"grn {(B, T, C, kind)} vec={vec} trips={trips} gx", ws, gx, gx32)
    gated(f"grn {(B, T, C, kind)} vec={vec} trips={trips}", out, ref, ref32)
    assert torch.equal(xd.cpu(), x) and float(xflat[n + xo]) == SENT and float(gflat[C + go]) == SENT
    if kind == "zero":                                          # gx = 0 -> beta + x through the + 1e-6
        assert float(ws[1].abs().max()) == 0 and torch.equal(out[1].cpu(), bet.expand(T, C))


# ------------------------------------------------------------------ dwconv7, im2col

@pytest.mark.parametrize("B,T,C", R.DWCONV7_CASES)
def test_dwconv7(ops, B, T, C):
    x, w_t, bias = R.dwconv7_inputs(B, T, C)
    xd, wd, bd = dev(x), dev(w_t), dev(bias)
    out = torch.full((B + 1, T, C), SENT, device="cuda")
    ops.dwconv7(xd, wd, bd, out[:B])
    assert torch.equal(out[:B].cpu(), R.dwconv7(x, w_t, bias).float()) and bool((out[B] == SENT).all())
    assert torch.equal(xd.cpu(), x) and torch.equal(wd.cpu(), w_t)


@pytest.mark.parametrize("ksize", R.IM2COL_K)
def test_im2col(ops, ksize):
    B = R.IM2COL_B
    for T in R.IM2COL_T:
        for Cin in R.IM2COL_CIN:
            x = R.im2col_inputs(B, T, Cin)
            xd = dev(x)
            for pad in R.im2col_pads(ksize, T):
                col = torch.full((B + 1, T, ksize * Cin), SENT, device="cuda")
                ops.im2col(xd, col[:B], ksize, pad)
                assert torch.equal(col[:B].cpu(), R.im2col(x, ksize, pad)), (ksize, T, Cin, pad)
                assert bool((col[B] == SENT).all())


def test_im2col_past_the_grid_cap(ops):
    B, T, Cin, ksize, pad = R.IM2COL_BIG
    x = R.im2col_inputs(B, T, Cin)
    col = torch.full((B + 1, T, ksize * Cin), SENT, device="cuda")
    ops.im2col(dev(x), col[:B], ksize, pad)
    assert torch.equal(col[:B].cpu(), R.im2col(x, ksize, pad)) and bool((col[B] == SENT).all())


# ------------------------------------------------------------------ refusals: nothing is launched

M0, N0, K0 = 5, 8, 8


def gemm_problem():
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)   # noqa: E731
    return dict(a=torch.ones(M0, K0, device="cuda"), w=torch.ones(N0, K0, device="cuda"), bias=z(N0),
                out=torch.full((M0, N0), SENT, device="cuda"), outb=torch.full((M0, N0), SENT, device="cuda", dtype=BF))


def test_gemm_wrapper_refusals(ops, F5EError):
    """One refusal per rule of ops.gemm_f32, each with its message; the sentinel-filled outputs keep their bits."""
    p = gemm_problem()
    a, w, b, out, outb = p["a"], p["w"], p["bias"], p["out"], p["outb"]
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)   # noqa: E731
    wide = torch.full((M0, 2 * N0), SENT, device="cuda")
    bad = [
        (dict(out=outb), "out must be a 2-D torch.float32"),                        # a bf16 tensor as the fp32 output
        (dict(out=torch.zeros(M0, N0)), "out must be a 2-D torch.float32"),         # on the CPU
        (dict(out=wide[:, ::2]), "out must be a 2-D torch.float32"),                # column stride 2
        (dict(out=out.view(-1)), "out must be a 2-D torch.float32"),                # 1-D
        (dict(out_bf16=out), "out_bf16 must be a 2-D torch.bfloat16"),
        (dict(out_bf16=wide.to(BF)[:, ::2]), "out_bf16 must be a 2-D torch.bfloat16"),
        (dict(out=out, addend=outb), "addend must be a 2-D torch.float32"),
        (dict(out=out, addend=wide[:, ::2]), "addend must be a 2-D torch.float32"),
        (dict(out=out[:, :N0 - 1]), "out has 7 columns, fewer than the 8"),
        (dict(out_bf16=outb[:, :N0 - 1]), "out_bf16 has 7 columns, fewer than the 8"),
        (dict(out=out[1:]), "out: 5 rows of stride 8 need 40 elements, the storage holds 32"),
        (dict(out_bf16=outb[1:]), "out_bf16: 5 rows of stride 8 need 40 elements, the storage holds 32"),
        (dict(out=out[:1].expand(M0, N0)), "out: row stride 0 is smaller than the 8 columns"),
        (dict(out=out, addend=out[:, :N0 - 1]), "addend has 7 columns, fewer than the 8"),
        (dict(out=out, addend=z(M0, N0)[:0]), "addend must have at least one row"),
        (dict(out=out, bias=z(N0 - 1)), "bias must hold at least 8 elements"),
        (dict(out=out, ch_scale=z(N0 - 1)), "ch_scale must hold at least 8 elements"),
        (dict(out=out, row_scale=z(M0 - 1)), "row_scale must hold at least 5 elements"),
        (dict(), "needs out or out_bf16"),
        (dict(out=out, K=K0 + 4), "K = 12 is larger than a's width 8"),
        (dict(out=out, a=z(M0, K0 + 4)), "K = 12 is larger than a's width 12 or w's width 8"),
        (dict(out=out, a=a[:M0 - 2], M=M0 + 1, addend=z(M0, N0)), "out: 6 rows of stride 8 need 48 elements"),
        (dict(out=out, w=w.to(BF)), "w must be a 2-D f32 GPU tensor"),
        (dict(out=out, a=a.cpu()), "a must be a 2-D f32 GPU tensor"),
    ]
    for kw, msg in bad:
        kw = dict(kw)
        args = (kw.pop("a", a), kw.pop("w", w), kw.pop("bias", b))
        with pytest.raises(F5EError) as e:
            ops.gemm_f32(*args, **kw)
        assert msg in str(e.value), (msg, str(e.value))
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((outb == SENT).all()) and bool((wide == SENT).all())


def test_gemm_library_refusals(ops, F5EError):
    """The C entry's own refusals, reached through the wrapper where it lets them through (K % 4, lda % 4, ldw % 4, the empty
    problem) and by a direct call for what the wrapper already refuses (leading dimensions below N, add_rows = 0)."""
    p = gemm_problem()
    a, w, b, out = p["a"], p["w"], p["bias"], p["out"]
    odd = torch.ones(M0, K0 + 2, device="cuda")
    for kw, msg in ((dict(K=6), "K, lda, ldw must be multiples of 4"),
                    (dict(a=odd[:, :K0]), "K, lda, ldw must be multiples of 4"),
                    (dict(w=torch.ones(N0, K0 + 2, device="cuda")[:, :K0]), "K, lda, ldw must be multiples of 4"),
                    (dict(M=0), "empty problem")):
        kw = dict(kw)
        args = (kw.pop("a", a), kw.pop("w", w), b)
        with pytest.raises(F5EError) as e:
            ops.gemm_f32(*args, out=out, **kw)
        assert msg in str(e.value), (msg, str(e.value))
    st, P = torch.cuda.current_stream().cuda_stream, lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    outb = p["outb"]
    for ldo, ldb, ld_add, add_rows, msg in ((N0 - 1, N0, N0, M0, "ldo=7 must be at least N=8"),
                                            (N0, N0 - 1, N0, M0, "ldo_bf16=7 must be at least N=8"),
                                            (N0, N0, N0 - 1, M0, "ld_add=7 must be at least N=8"),
                                            (N0, N0, N0, 0, "add_rows must be positive")):
        with pytest.raises(F5EError) as e:
            ops.check(ops.lib().f5e_gemm_f32(st, P(a), K0, M0, 0, P(w), K0, P(b), 0, None, P(out), ld_add, add_rows, None,
                                             P(out), ldo, P(outb), ldb, M0, N0, K0), "f5e_gemm_f32")
        assert msg in str(e.value), (msg, str(e.value))
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((outb == SENT).all())


def test_gemm_accepts_the_forms_of_the_tree(ops):
    """What the models pass and the new checks must not refuse: an A whose rows overlap (lda < width, WavLM's as_strided
    patches), M > a_rows, one-row tensors with an arbitrary row stride, misaligned 1-D slices."""
    Cc, k, s, rows = 4, 3, 2, 6
    flat = torch.arange(((rows - 1) * s + k) * Cc, dtype=F32)
    w = torch.randint(-4, 5, (8, k * Cc), generator=R.g(400)).float()
    av = torch.as_strided(flat, (rows, k * Cc), (s * Cc, 1))
    out = torch.full((rows, 8), SENT, device="cuda")
    ops.gemm_f32(torch.as_strided(flat.cuda(), (rows, k * Cc), (s * Cc, 1)), dev(w), None, out=out)
    assert torch.equal(out.cpu(), (av.double() @ w.double().T).float())
    # M > a_rows, a one-row addend whose row stride is 0 (a broadcast view), bias and ch_scale as misaligned 1-D slices
    t = R.gemm_operands(R.Case(33, 68, 68, a_rows=13, **{**R.FULL, "add_rows": 1, "outs": "f32"}))
    vec = torch.cat([t["bias"], t["cs"]])
    vd = torch.cat([torch.zeros(1), vec]).cuda()
    add_row = dev(t["add"][0])
    out = torch.full((33, 68), SENT, device="cuda")
    ops.gemm_f32(dev(t["A"]), dev(t["W"]), vd[1:69], out=out, ch_scale=vd[69:137], M=33, row_scale=dev(t["rs"]),
                 addend=add_row.unsqueeze(0).expand(1, 68).as_strided((1, 68), (0, 1)))
    ref = R.gemm_ref(R.Case(33, 68, 68, a_rows=13, **{**R.FULL, "add_rows": 1, "outs": "f32"}), t)
    assert vd[1:69].data_ptr() % 16 == 4 and torch.equal(out.cpu(), ref.float())
    # a one-row output inside a wider buffer, taken as a row with a foreign stride
    buf = torch.full((3, 100), SENT, device="cuda")
    row = buf.as_strided((1, 68), (7, 1), 104)
    ops.gemm_f32(dev(t["A"][:1]), dev(t["W"]), None, out=row)
    got = buf.cpu()
    assert torch.equal(got.view(-1)[104:172], (t["A"][:1].double() @ t["W"].double().T).float()[0])
    assert bool((got.view(-1)[:104] == SENT).all()) and bool((got.view(-1)[172:] == SENT).all())


def test_grn_dwconv7_im2col_refusals(ops, F5EError):
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)   # noqa: E731
    B, T, Cc = 2, 5, 8
    x, out = z(B, T, Cc), torch.full((B, T, Cc), SENT, device="cuda")
    ws = torch.full((B, Cc), SENT, device="cuda")
    bad = [
        (lambda: ops.grn(x.view(B * T, Cc), out, z(Cc), z(Cc), ws), "grn: x must be a non-empty [B, T, C]"),
        (lambda: ops.grn(x, out[:, :T - 1], z(Cc), z(Cc), ws), "grn: out must be [2, 5, 8]"),
        (lambda: ops.grn(x, out.view(B * T, Cc), z(Cc), z(Cc), ws), "grn: out must be [2, 5, 8]"),
        (lambda: ops.grn(x, out, z(Cc + 1), z(Cc), ws), "grn: gamma must be [8]"),
        (lambda: ops.grn(x, out, z(Cc), z(1, 1, Cc), ws), "grn: beta must be [8]"),
        (lambda: ops.grn(x, out, z(Cc), z(Cc), ws.view(-1)[:B * Cc - 1]), "grn: ws must hold B * C = 16"),
        (lambda: ops.dwconv7(x[0], z(7, Cc), z(Cc), out[0]), "dwconv7: x must be a non-empty [B, T, C]"),
        (lambda: ops.dwconv7(x, z(7, Cc), z(Cc), out[:1]), "dwconv7: out must be [2, 5, 8]"),
        (lambda: ops.dwconv7(x, z(Cc, 7), z(Cc), out), "dwconv7: w_t must be [7, 8]"),
        (lambda: ops.dwconv7(x, z(5, Cc), z(Cc), out), "dwconv7: w_t must be [7, 8]"),
        (lambda: ops.dwconv7(x, z(7, Cc), z(Cc - 4), out), "dwconv7: bias must be [8]"),
        (lambda: ops.dwconv7(z(B, T, 6), z(7, 6), z(6), z(B, T, 6)), "must be a positive multiple of 4"),     # the library's own
        (lambda: ops.im2col(x.view(B * T, Cc), out, 1, 0), "im2col: x must be a non-empty [B, T, C]"),
        (lambda: ops.im2col(x, out, 3, 1), "im2col: col must be [2, 5, 24]"),
        (lambda: ops.im2col(x, z(B, T, 3, Cc), 3, 1), "im2col: col must be [2, 5, 24]"),
        (lambda: ops.im2col(x, out, 0, 0), "im2col: needs ksize >= 1 and pad >= 0"),
        (lambda: ops.im2col(x, out, 1, -1), "im2col: needs ksize >= 1 and pad >= 0"),
    ]
    for call, msg in bad:
        with pytest.raises(F5EError) as e:
            call()
        assert msg in str(e.value), (msg, str(e.value))
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((ws == SENT).all())
