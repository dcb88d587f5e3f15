"""Direct parity of the norm, conformer-front and sampler kernels: every HIP op, called through f5e_tts_amd.ops, against the
fp64 restatement of tests/small_ops_ref.py (pinned on the CPU by tests/test_small_ops_cpu.py) on the same seeded fp32 inputs.

Case -> path (what nothing else in the suite executes):
  test_layernorm_fixed_widths        layernorm_kernel<5..8> (D 1280..2048), partial last workgroup (rows 7); bf16 + modulation
                                     with mod_rows wrap-around (row 6 -> modulation row 0) and eval_ptr; eps 1e-5; gamma/beta
                                     together with scale/shift; in place; ldx / ldy of row-strided views
  test_layernorm_any_width           layernorm_any_kernel where D/4 crosses a 64-lane boundary (252 / 260 / 516 / 2044) and the
                                     ``c < nv`` guards decide; 4 (one lane), 100, 1000; in place
  test_adaln_pre                     adaln_pre_kernel<1, 2, 5, 8>, parts 4..32, mod_rows wrap, with / without eval_ptr
  test_l2norm                        l2norm_kernel<1, 3, 4, 8>, bf16 and fp32 stores, the 1e-12 clamp on a zero row, ldx / ldy
  test_norm_refusals, test_row_view_refusals    every host-side refusal (nothing is launched)
  test_glu                           second trip of the grid-stride loop (grid_for cap 4096 x 256), saturated gates, ldx / ldy
  test_dwconv                        K 1..31, T 1, ``keep`` over non-zero padding, second trip of the grid-stride loop
  test_softmax_rows[_large_magnitude]    len 0 / interior / L / > L, pad columns, 64-lane boundaries (63 / 64 / 65), in place
  test_kaldi_fbank_frames_and_bins   one frame (nw == win), (nw - win) % shift == shift - 1, silence (log(eps) floor), 23 bins
  test_axpby, test_casts_round_trip, test_stitch_past_the_grid_cap, test_text_gather_clamps, test_ode_update_*
                                     second trip of the grid-stride loops (grid_for cap 2048 x 256); y = None; bf16 rounding
                                     rule; min(n, max_pos - 1) and the id clamp; pos / keep = None; the done_ctr ticket with a
                                     capped grid; traj_stride / traj_div row selection
  test_vq_eval                       the per-lane ``v += 64`` loop, the cross-lane tie rule, the ``d += 64`` copy loop
                                     (var_dim 100), ld > G V, combine_groups; statistics at the num_vars limit
  test_bigvgan_post                  f5e_bigvgan_post: clamp and tanh, bias = None, L around the 256-thread workgroup

Gates.  Where the project already gates the op, that gate (cited at the comparison).  Elsewhere the kernel's error against
the fp64 reference may be 4x the error of the SAME restatement evaluated in fp32 on the CPU (neither side is more accurate than
fp32; the margin covers summation order and FMA contraction), plus one fp32 ulp of the output's magnitude, plus for the
``__expf`` kernels |arg| 2^-23 relative per exponential (the rounding of arg log2(e); |arg| <= 20 in every gated case, about
3e-6).  Each such test prints the yardstick and the kernel's error side by side; the observed pairs are in the docstrings."""
import math

import pytest
import torch

import small_ops_ref as R
from oracle import f5e_ppg_oracle as P

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
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


def close(a, b, rtol, atol, what=""):
    a, b = a.double().cpu(), b.double().cpu()
    err = (a - b).abs()
    bad = ~(err <= atol + rtol * b.abs())
    print(f"{what}: max err {float(err.max()):.3e}, largest err / gate {float((err / (atol + rtol * b.abs())).max()):.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.3e} " \
                          f"(ref max {float(b.abs().max()):.3e})"


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def gated(what, got, ref64, ref32, rel_extra=0.0):
    """|kernel - fp64| <= 4 max|fp32 restatement - fp64| + (2^-23 + rel_extra) |fp64|, element by element."""
    got, ref32 = got.double().cpu().reshape(ref64.shape), ref32.double().reshape(ref64.shape)
    yard = float((ref32 - ref64).abs().max())
    err = (got - ref64).abs()
    print(f"{what}: fp32 restatement vs fp64 {yard:.3e}, kernel vs fp64 {float(err.max()):.3e}")
    bad = ~(err <= 4 * yard + (ULP + rel_extra) * ref64.abs())
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} past the gate, max err {float(err.max()):.3e}, yardstick {yard:.3e}"


def in_buffer(t, extra, dtype=None):
    """t [rows, cols] as the [:, :cols] view of a sentinel-filled device buffer [rows, cols + extra]."""
    buf = torch.full((t.shape[0], t.shape[1] + extra), SENT, device="cuda", dtype=dtype or t.dtype)
    buf[:, :t.shape[1]] = t.cuda()
    return buf, buf[:, :t.shape[1]]


def untouched(buf, cols):
    return bool((buf[:, cols:] == SENT).all())


# ------------------------------------------------------------------ norm.hip

@pytest.mark.parametrize("D", R.LN_SMALL_D + R.LN_FIXED_D)
def test_layernorm_fixed_widths(ops, D):
    """Gates of test_layernorm_variants (tests/test_ops_gpu.py: bf16 ``close(out, ref, 2 ** -7, 2e-3)``, fp32
    ``close(out32, ..., 1e-5, 1e-5)``).  Observed on one MI355X over these widths: fp32 variants max error 1.9e-7 .. 1.5e-6
    (at most 0.04 of the gate), bf16 variants 1.5e-2 on values up to 7 (at most 0.46 of the gate)."""
    rows = 7
    x, gam, bet, tab = R.ln_inputs(rows, D)
    td, stride = dev(tab), tab.stride(0)
    sc, sh = tab[0, :, D:2 * D], tab[0, :, 0:D]
    scd, shd = td[0, :, D:2 * D], td[0, :, 0:D]
    if D in R.LN_FIXED_D:
        ev = torch.tensor([1], dtype=torch.int32, device="cuda")
        out = torch.empty(rows, D, device="cuda", dtype=BF)
        ops.layernorm(dev(x), out, scale=scd, shift=shd, rows_per_seq=3, eval_ptr=ev, eval_stride=stride)
        close(out, R.layernorm(x, None, scale=sc, shift=sh, rows_per_seq=3, eval_ptr=1, eval_stride=stride), 2 ** -7, 2e-3,
              "bf16, modulation rows wrap, eval 1")
        out32 = torch.empty(rows, D, device="cuda")
        ops.layernorm(dev(x), out32, gamma=dev(gam), beta=dev(bet), eps=1e-5)
        close(out32, R.layernorm(x, None, gamma=gam, beta=bet, eps=1e-5), 1e-5, 1e-5, "affine, eps 1e-5")
        (xbuf, xv), (obuf, ov) = in_buffer(x, 8), in_buffer(torch.zeros(rows, D), 12)
        ops.layernorm(xv, ov, gamma=dev(gam), beta=dev(bet))
        close(ov, R.layernorm(x, None, gamma=gam, beta=bet), 1e-5, 1e-5, "row-strided views")
        assert untouched(xbuf, D) and untouched(obuf, D) and torch.equal(xv.cpu(), x)
        obuf, ov = in_buffer(torch.zeros(rows, D), 4, BF)
        ops.layernorm(xv, ov, scale=scd, shift=shd, rows_per_seq=3)
        close(ov, R.layernorm(x, None, scale=sc, shift=sh, rows_per_seq=3), 2 ** -7, 2e-3, "row-strided views, bf16 out")
        assert untouched(obuf, D)
    out32 = torch.empty(rows, D, device="cuda")
    ops.layernorm(dev(x), out32, gamma=dev(gam), beta=dev(bet), scale=scd, shift=shd, rows_per_seq=3)
    close(out32, R.layernorm(x, None, gamma=gam, beta=bet, scale=sc, shift=sh, rows_per_seq=3), 1e-5, 1e-5,
          "gamma/beta and scale/shift in one call")
    xd = dev(x)
    assert ops.layernorm(xd, xd, gamma=dev(gam), beta=dev(bet), eps=1e-5) is xd
    close(xd, R.layernorm(x, None, gamma=gam, beta=bet, eps=1e-5), 1e-5, 1e-5, "in place")


@pytest.mark.parametrize("D", R.LN_ANY_D)
def test_layernorm_any_width(ops, D):
    """fp32 gate of test_layernorm_variants (1e-5 / 1e-5).  The row after each one is live data (rows 5, contiguous), so a
    lane that reads past ``nv`` folds the next row into the statistics.  Observed on one MI355X: max error 1.3e-7 .. 7.8e-7,
    at most 0.03 of the gate."""
    rows = 5
    x, gam, bet, _ = R.ln_inputs(rows, D)
    out = torch.full((rows, D), SENT, device="cuda")
    ops.layernorm(dev(x), out, eps=1e-5)
    close(out, R.layernorm(x, None, eps=1e-5), 1e-5, 1e-5, "plain")
    out = torch.full((rows, D), SENT, device="cuda")
    ops.layernorm(dev(x), out, gamma=dev(gam), beta=dev(bet), eps=1e-5)
    ref = R.layernorm(x, None, gamma=gam, beta=bet, eps=1e-5)
    close(out, ref, 1e-5, 1e-5, "affine")
    xd = dev(x)
    ops.layernorm(xd, xd, gamma=dev(gam), beta=dev(bet), eps=1e-5)
    close(xd, ref, 1e-5, 1e-5, "in place")
    (xbuf, xv), (obuf, ov) = in_buffer(x, 4), in_buffer(torch.zeros(rows, D), 8)
    ops.layernorm(xv, ov, gamma=dev(gam), beta=dev(bet), eps=1e-5)
    close(ov, ref, 1e-5, 1e-5, "row-strided views")
    assert untouched(xbuf, D) and untouched(obuf, D)


@pytest.mark.parametrize("with_eval", [False, True])
@pytest.mark.parametrize("D", R.ADALN_D)
def test_adaln_pre(ops, D, with_eval):
    """Gates of test_fused_adaln_chain (tests/test_ops_gpu.py: "pre row mean" 1e-5 / 1e-6, "pre xs (centred)" 2^-7 / 1e-6,
    stats[..., 0] == 0 exactly, "pre M2" 1e-5 / 1e-4; a share is M2 / parts, so its absolute term is 1e-4 / parts; the shares
    of a row are NOT bitwise equal: wave_sum leaves the lanes of different quads an ulp apart).  Observed on one MI355X:
    row mean 4.7e-8 .. 8.5e-8 (0.008 of the gate), xs 0.50 of the gate (the bf16 rounding), M2 0.012 of the gate."""
    rows, parts = 7, D // 64
    x, _, _, tab = R.ln_inputs(rows, D)
    td = dev(tab)
    xs = torch.empty(rows, D, device="cuda", dtype=BF)
    stats = torch.full((rows, parts, 2), SENT, device="cuda")
    rm = torch.empty(rows, device="cuda")
    ev = torch.tensor([1], dtype=torch.int32, device="cuda") if with_eval else None
    ops.adaln_pre(dev(x), xs, td[0, :, D:2 * D], stats, rm, 3, eval_ptr=ev, eval_stride=tab.stride(0) if with_eval else 0)
    r_xs, r_st, r_rm = R.adaln_pre(x, None, tab[0, :, D:2 * D], parts, None, 3, 1 if with_eval else None, tab.stride(0))
    close(rm, r_rm, 1e-5, 1e-6, "row mean")
    close(xs, r_xs, 2 ** -7, 1e-6, "xs (centred)")
    assert float(stats[:, :, 0].abs().max()) == 0
    close(stats[:, :, 1].sum(1), r_st[:, :, 1].sum(1), 1e-5, 1e-4, "M2")
    close(stats[:, :, 1], r_st[:, :, 1], 1e-5, 1e-4 / parts, "M2 shares")          # the M2 gate, per share


@pytest.mark.parametrize("D", R.L2_D)
def test_l2norm(ops, D):
    """No earlier gate: 4x the fp32 restatement (+ one fp32 ulp); the bf16 output adds its own rounding, half a bf16 ulp
    <= 2^-8 |ref|.  Observed on one MI355X (fp32 restatement vs fp64 | kernel vs fp64): D 256 3.3e-7 | 4.2e-7, 768 5.3e-7 |
    5.2e-7, 1024 6.3e-7 | 6.3e-7, 2048 6.7e-7 | 6.7e-7; bf16 output 1.1e-2 .. 1.5e-2 on values up to 9."""
    rows = 7
    x, gw = R.l2_inputs(rows, D)
    ref, ref32 = R.l2norm(x, None, gw), R.l2norm(x, None, gw, dtype=F32)
    out = torch.full((rows, D), SENT, device="cuda")
    ops.l2norm(dev(x), out, dev(gw))
    gated(f"l2norm D={D} f32", out, ref, ref32)
    assert float(out[3].abs().max()) == 0 and bool(torch.isfinite(out).all())       # the zero row: finite zeros
    outb = torch.full((rows, D), SENT, device="cuda", dtype=BF)
    ops.l2norm(dev(x), outb, dev(gw))
    gated(f"l2norm D={D} bf16", outb, ref, ref32, rel_extra=2.0 ** -8)
    assert float(outb[3].float().abs().max()) == 0
    (xbuf, xv), (obuf, ov) = in_buffer(x, 8), in_buffer(torch.zeros(rows, D), 12)
    ops.l2norm(xv, ov, dev(gw))
    assert torch.equal(ov, out) and untouched(xbuf, D) and untouched(obuf, D)      # the stride changes nothing else
    obuf, ov = in_buffer(torch.zeros(rows, D), 4, BF)
    ops.l2norm(xv, ov, dev(gw))
    assert torch.equal(ov, outb) and untouched(obuf, D)


def test_norm_refusals(ops, F5EError):
    """Host-side checks only: each raises before anything is launched."""
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)   # noqa: E731
    with pytest.raises(F5EError):
        ops.layernorm(z(2, 258), z(2, 258))
    with pytest.raises(F5EError):
        ops.layernorm(z(2, 2052), z(2, 2052))
    with pytest.raises(F5EError):
        ops.layernorm(z(2, 100), z(2, 100, dtype=BF))
    with pytest.raises(F5EError):
        ops.layernorm(z(2, 100), z(2, 100), scale=z(2, 100), shift=z(2, 100))
    with pytest.raises(F5EError):
        ops.layernorm(z(2, 256), z(2, 256), gamma=z(256))
    with pytest.raises(F5EError):
        ops.l2norm(z(2, 100), z(2, 100), z(100))
    with pytest.raises(F5EError):
        ops.adaln_pre(z(2, 256), z(2, 256, dtype=BF), z(1, 256), z(2, 33, 2), z(2), 1)      # parts = 33


def test_row_view_refusals(ops, F5EError):
    """layernorm, l2norm, glu and softmax_rows take row-strided views; what their vector accesses cannot take is refused
    on the host (pytest.raises only: no misaligned launch is ever made)."""
    D = 256
    flat = torch.zeros(4 * (D + 8) + 8, device="cuda")
    ok = flat[:4 * (D + 8)].view(4, D + 8)[:, :D]
    off = flat[1:1 + 4 * (D + 8)].view(4, D + 8)[:, :D]                  # base 4 bytes past a 16-byte boundary
    odd = flat[:4 * (D + 6)].view(4, D + 6)[:, :D]                       # row stride not a multiple of 4
    cols = torch.zeros(4, 2 * D, device="cuda")[:, ::2]                  # column stride 2
    gw = torch.ones(D, device="cuda")
    for bad in (off, odd, cols):
        for call in (lambda t: ops.layernorm(t, ok), lambda t: ops.layernorm(ok, t), lambda t: ops.l2norm(t, ok, gw),
                     lambda t: ops.l2norm(ok, t, gw), lambda t: ops.glu(ok, t[:, :D // 2]),
                     lambda t: ops.glu(t, torch.zeros(4, D // 2, device="cuda"))):
            with pytest.raises(F5EError):
                call(bad)
    with pytest.raises(F5EError):
        ops.layernorm(ok, ok.to(BF)[:, 1:])                              # shape mismatch
    with pytest.raises(F5EError):
        ops.layernorm(ok, ok, scale=off[:2], shift=off[:2])              # misaligned modulation table
    with pytest.raises(F5EError):
        ops.glu(ok, torch.zeros(4, D, device="cuda"))                    # x must be [rows, 2C]
    # softmax_rows: scalar accesses, so any alignment and stride; but it zeroes whole rows of out's stride
    short = torch.zeros(4 * 12 - 2, device="cuda").as_strided((4, 9), (12, 1))
    full = torch.zeros(4, 12, device="cuda")[:, :9]
    with pytest.raises(F5EError):
        ops.softmax_rows(full, short, 9, 1.0)
    with pytest.raises(F5EError):
        ops.softmax_rows(cols, full, 9, 1.0)
    with pytest.raises(F5EError):
        ops.softmax_rows(full, full, 10, 1.0)                            # L past the view
    assert float(flat.abs().max()) == 0 and float(full.abs().max()) == 0


# ------------------------------------------------------------------ ppg.hip

@pytest.mark.parametrize("case", R.GLU_CASES)
def test_glu(ops, case):
    """No earlier gate: 4x the fp32 restatement + one ulp + |gate| 2^-23 for the one __expf.  Saturated gates are exact:
    +30 / +100 give a (1 + exp(-30) rounds to 1), -100 gives 0 (exp(100) overflows to inf), no NaN anywhere.  Observed on one
    MI355X (fp32 restatement | kernel): (5, 64) 2.1e-7 | 2.1e-7, (77, 256) 2.4e-7 | 2.4e-7, (4100, 1024) 4.6e-7 | 4.6e-7."""
    rows, C = case
    x, kind = R.glu_inputs(rows, C)
    ref, ref32 = R.glu(x), R.glu(x, dtype=F32)
    out = torch.full((rows, C), SENT, device="cuda")
    ops.glu(dev(x), out)
    o = out.cpu()
    assert bool(torch.isfinite(o).all())
    arg = x[:, C:].abs().double()
    err = (o.double() - ref).abs()
    yard = float((ref32.double() - ref).abs().max())
    print(f"glu {case}: fp32 restatement vs fp64 {yard:.3e}, kernel vs fp64 {float(err.max()):.3e}")
    assert bool((err <= 4 * yard + (ULP + arg * ULP) * ref.abs()).all()), float(err.max())
    assert torch.equal(o[(kind == 1) | (kind == 3)], x[:, :C][(kind == 1) | (kind == 3)])
    assert float(o[kind == 4].abs().max()) == 0
    if case == (77, 256):     # x and out as views of wider sentinel-filled buffers
        (xbuf, xv), (obuf, ov) = in_buffer(x, 8), in_buffer(torch.zeros(rows, C), 4)
        assert xv.stride(0) == 2 * C + 8 and ov.stride(0) == C + 4
        ops.glu(xv, ov)
        assert torch.equal(ov, out) and untouched(xbuf, 2 * C) and untouched(obuf, C)


@pytest.mark.parametrize("case", R.DWCONV_CASES)
def test_dwconv(ops, case):
    """Gate of test_dwconv_stream_kernel (tests/test_ppg_stream_gpu.py: ``assert e < 1e-6``, relative L2).  Observed on one
    MI355X: 2.0e-8 .. 1.2e-7 (K = 31, T = 53), the case past the grid cap 8.9e-8, with keep 7.0e-8."""
    B, T, C, K = case
    x, w_t, bias, keep = R.dwconv_inputs(B, T, C, K)
    xd, wd, bd = dev(x), dev(w_t), dev(bias)
    out = ops.dwconv(xd, wd, bd, torch.full((B, T, C), SENT, device="cuda"))
    e0 = rel_l2(out, R.dwconv(x, w_t, bias))
    outk = ops.dwconv(xd, wd, bd, torch.full((B, T, C), SENT, device="cuda"), keep=dev(keep))
    e1 = rel_l2(outk, R.dwconv(x, w_t, bias, None, keep))
    print(f"dwconv {case}: rel L2 {e0:.2e}, with keep {e1:.2e}")
    assert e0 < 1e-6 and e1 < 1e-6


def test_dwconv_refusals(ops, F5EError):
    z = lambda *s: torch.zeros(*s, device="cuda")   # noqa: E731
    for C, K in ((8, 4), (8, 33), (6, 3)):
        with pytest.raises(F5EError):
            ops.dwconv(z(1, 5, C), z(K, C), z(C), z(1, 5, C))


def softmax_case(ops, L, big=False):
    buf, kv, scale = R.softmax_inputs(L, big)
    ld = buf.shape[1]
    ref = R.softmax_rows(buf[:, :L], ld, L, scale, kv, R.SOFTMAX_RPS)
    xb = dev(buf)
    ob = torch.full((R.SOFTMAX_ROWS, ld), SENT, device="cuda")
    ops.softmax_rows(xb[:, :L], ob[:, :L], L, scale, kv_len=dev(kv), rows_per_seq=R.SOFTMAX_RPS)
    assert torch.equal(xb.cpu(), buf)
    o = ob.cpu()
    ln = torch.clamp(kv.long()[torch.arange(R.SOFTMAX_ROWS) // R.SOFTMAX_RPS], max=L)
    beyond = torch.arange(ld)[None, :] >= ln[:, None]
    assert bool(torch.isfinite(o).all()) and float(o[beyond].abs().max()) == 0      # pad columns and columns >= len: exact zeros
    assert float(o[:2].abs().max()) == 0                                             # kv_len = 0: all zero, no NaN
    plain = torch.full((R.SOFTMAX_ROWS, ld), SENT, device="cuda")
    ops.softmax_rows(xb[:, :L], plain[:, :L], L, scale)
    assert torch.equal(plain[6], ob[6])                                              # kv_len > L: the unmasked row
    inpl = xb.clone()
    ops.softmax_rows(inpl[:, :L], inpl[:, :L], L, scale, kv_len=dev(kv), rows_per_seq=R.SOFTMAX_RPS)
    assert torch.equal(inpl, ob)                                                     # in place: bitwise the same
    return buf, kv, scale, ref, o, ln


@pytest.mark.parametrize("L", R.SOFTMAX_L)
def test_softmax_rows(ops, L):
    """No earlier gate: 4x the fp32 restatement + one ulp + 2 x 20 x 2^-23 relative (numerator and denominator each carry
    __expf's argument rounding; |arg| <= 9.8 here, bounded by the 20 the gate is stated for).  Observed on one MI355X (fp32
    restatement | kernel): L 63 2.0e-8 | 2.0e-8, 64 3.6e-8 | 3.6e-8, 65 5.8e-8 | 5.8e-8, 200 8.5e-8 | 8.5e-8."""
    buf, kv, scale, ref, o, _ = softmax_case(ops, L)
    ref32 = R.softmax_rows(buf[:, :L], buf.shape[1], L, scale, kv, R.SOFTMAX_RPS, dtype=F32)
    gated(f"softmax_rows L={L}", o, ref, ref32, rel_extra=2 * 20 * ULP)


def test_softmax_rows_large_magnitude(ops):
    """scale x in +-1e4: far outside what __expf's accuracy is stated for, so only properties: finite, rows sum to one within
    1e-4, the largest input holds the largest output, masked columns exactly zero (softmax_case).  Observed on one MI355X:
    every live row sums to exactly 1 (one key takes all the mass)."""
    L = 200
    buf, kv, scale, ref, o, ln = softmax_case(ops, L, big=True)
    live = ln > 0
    sums = o[live].double().sum(1)
    print("softmax_rows +-1e4: row sums - 1:", [f"{float(s - 1):.1e}" for s in sums])
    assert bool(((sums - 1).abs() <= 1e-4).all())
    for r in torch.nonzero(live).flatten().tolist():
        k = int(torch.argmax(buf[r, :int(ln[r])]))
        assert float(o[r, k]) == float(o[r].max()) and float(o[r, k]) > 0


@pytest.mark.parametrize("nw,n_mels", R.FBANK_CASES)
def test_kaldi_fbank_frames_and_bins(nw, n_mels):
    """Gate of test_kaldi_fbank_kernel_vs_oracle (tests/test_ppg_gpu.py: rtol 2e-4, atol 2e-3) against the same oracle; the
    silent row equals log(eps) exactly.  Observed on one MI355X: max |kernel - oracle| 1.9e-6 .. 3.8e-6 at 23 bins, 8.3e-5 at
    80 bins, on values -15.9 .. 26.9."""
    from f5e_tts_amd.ppg import kaldiFbank
    wav = R.fbank_inputs(nw)
    feats, n = kaldiFbank(n_mels=n_mels)(wav.cuda())
    ref = torch.stack([P.kaldi_fbank(wav[i], n_mels) for i in range(3)])
    T = 1 + (nw - 400) // 160
    assert feats.shape == ref.shape == (3, T, n_mels) and int(n) == T
    f = feats.cpu()
    print(f"kaldi_fbank nw={nw} bins={n_mels}: max |kernel - oracle| {float((f - ref).abs().max()):.3e}, values "
          f"{float(ref.min()):.2f} .. {float(ref.max()):.2f}")
    assert torch.equal(f[1], ref[1]) and bool((f[1] == torch.tensor(torch.finfo(F32).eps).log()).all())
    torch.testing.assert_close(f, ref, rtol=2e-4, atol=2e-3)


# ------------------------------------------------------------------ elementwise.hip

@pytest.mark.parametrize("n", R.AXPBY_N)
def test_axpby(ops, n):
    """No earlier gate: 4x the fp32 restatement + one ulp.  Observed on one MI355X: the kernel's error equals the fp32
    restatement's at every n (2.3e-8 at n = 1 .. 7.2e-7 at n = 524 365): both are one correctly rounded fma chain."""
    x, y = torch.randn(n, generator=R.g(200)), torch.randn(n, generator=R.g(201))
    a, b, c = 0.7, -1.3, 0.25
    out = torch.full((n,), SENT, device="cuda")
    ops.axpby(dev(x), dev(y), out, a, b, c)
    gated(f"axpby n={n}", out, R.axpby(x, y, None, a, b, c), R.axpby(x, y, None, a, b, c, dtype=F32))
    ops.axpby(dev(x), None, out, a, 0.0, c)
    gated(f"axpby n={n} y=None", out, R.axpby(x, None, None, a, 0.0, c), R.axpby(x, None, None, a, 0.0, c, dtype=F32))
    xd = dev(x)
    ops.axpby(xd, dev(y), xd, a, b, c)
    gated(f"axpby n={n} in place", xd, R.axpby(x, y, None, a, b, c), R.axpby(x, y, None, a, b, c, dtype=F32))


def test_casts_round_trip(ops):
    """cast_f32(cast_bf16(x)) is bit-equal to x.to(bf16).float(): round to nearest even at exact ties, FLT_MAX -> inf, NaN stays
    NaN (isnan only: the payload is not part of the contract), the sign of zero, denormals; n past the grid cap."""
    n = R.BIG_N
    x = R.cast_inputs(n)
    xb = torch.empty(n, device="cuda", dtype=BF)
    ops.cast_bf16(dev(x), xb)
    back = torch.full((n,), SENT, device="cuda")
    ops.cast_f32(xb, back)
    got, want = back.cpu(), x.to(BF).float()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan) and torch.equal(torch.isnan(xb.cpu()), nan)
    diff = torch.nonzero((got.view(torch.int32) != want.view(torch.int32)) & ~nan).flatten()
    assert diff.numel() == 0, [(int(i), hex(int(x.view(torch.int32)[i]) & 0xFFFFFFFF), float(got[i]), float(want[i])) for i in diff[:8]]


def test_stitch_past_the_grid_cap(ops):
    rows, C = R.STITCH_CASE
    mask = (torch.rand(rows, generator=R.g(210)) > 0.5).to(torch.uint8)
    c, y = torch.randn(rows, C, generator=R.g(211)), torch.randn(rows, C, generator=R.g(212))
    out = torch.full((rows, C), SENT, device="cuda")
    ops.stitch(dev(c), dev(y), dev(mask), out)
    assert torch.equal(out.cpu(), R.stitch(c, y, mask))


def test_text_gather_clamps(ops):
    """N = 2100 > max_pos = 64: every n >= 64 reads the last position row; ids -1 / -7 and table_rows / table_rows + 5 clamp to
    the first and last table rows (text_gather_kernel's comment); pos = None; keep = None.  One add and one multiplication
    by 0 / 1 per element: exact."""
    B, N, TD, max_pos, rows = R.TEXT_GATHER_CASE
    ids, table, pos, keep = R.text_gather_inputs(B, N, TD, max_pos, rows)
    idd, tabd, posd, keepd = dev(ids), dev(table), dev(pos), dev(keep)
    for p, k, pd, kd in ((pos, keep, posd, keepd), (None, keep, None, keepd), (pos, None, posd, None)):
        out = torch.full((B, N, TD), SENT, device="cuda")
        ops.text_gather(idd, tabd, pd, kd, out)
        assert torch.equal(out.cpu(), R.text_gather(ids, table, p, k, dtype=F32)), (p is None, k is None)


def ode_operands(n):
    return (torch.randn(3, n, generator=R.g(220)), torch.randn(n, generator=R.g(221)), torch.tensor([0.1, 0.25, 0.5, -0.75]))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_ode_update_past_the_grid_cap(ops, mode):
    """No earlier gate at this size: 4x the fp32 restatement + one ulp.  Observed on one MI355X (fp32 restatement | kernel):
    mode 1 9.5e-7 | 9.5e-7, mode 2 1.2e-6 | 1.2e-6; ticket and trajectory cases 2.3e-7 .. 9.5e-7, equal on both sides."""
    n = R.BIG_N
    pred, y, coef = ode_operands(n)
    ev = torch.tensor([2], dtype=torch.int32, device="cuda")
    dst, traj = torch.full((n,), SENT, device="cuda"), torch.full((n,), SENT, device="cuda")
    ops.ode_update(dev(pred), n, mode, 2.0, 3.0, dev(y), dst, dev(coef), ev, traj)
    gated(f"ode_update mode {mode}", dst, R.ode_update(pred, n, mode, 2.0, 3.0, y, None, coef, 2),
          R.ode_update(pred, n, mode, 2.0, 3.0, y, None, coef, 2, dtype=F32))
    assert torch.equal(dst, traj) and int(ev.item()) == 2


def test_ode_update_ticket_with_a_capped_grid(ops):
    """done_ctr with 2048 blocks striding over n: the last block to finish advances eval_ptr by exactly one and re-arms the
    ticket; the next launch reads the advanced value (a different coef entry)."""
    n = R.BIG_N
    pred, y, coef = ode_operands(n)
    pd, yd, cd = dev(pred), dev(y), dev(coef)
    ev = torch.zeros(1, dtype=torch.int32, device="cuda")
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    for e in (0, 1):
        dst = torch.full((n,), SENT, device="cuda")
        ops.ode_update(pd, n, 0, 0.0, 0.0, yd, dst, cd, ev, None, done)
        assert int(ev.item()) == e + 1 and int(done.item()) == 0
        gated(f"ode_update ticket, eval {e}", dst, R.ode_update(pred, n, 0, 0.0, 0.0, y, None, coef, e),
              R.ode_update(pred, n, 0, 0.0, 0.0, y, None, coef, e, dtype=F32))


@pytest.mark.parametrize("e", [0, 1, 2])
def test_ode_update_trajectory_row(ops, e):
    """traj_stride > 0, traj_div = 2: only row (e + 1) // 2 of the trajectory is written, and it equals dst."""
    n = R.BIG_N
    pred, y, coef = ode_operands(n)
    ev = torch.tensor([e], dtype=torch.int32, device="cuda")
    traj = torch.full((3, n), SENT, device="cuda")
    dst = torch.full((n,), SENT, device="cuda")
    ops.ode_update(dev(pred), n, 1, 2.0, 0.0, dev(y), dst, dev(coef), ev, traj, traj_stride=n, traj_div=2)
    row = (e + 1) // 2
    assert torch.equal(traj[row], dst) and all(bool((traj[r] == SENT).all()) for r in range(3) if r != row)
    gated(f"ode_update trajectory, eval {e}", dst, R.ode_update(pred, n, 1, 2.0, 0.0, y, None, coef, e),
          R.ode_update(pred, n, 1, 2.0, 0.0, y, None, coef, e, dtype=F32))


@pytest.mark.parametrize("V,G,vd,combine", R.VQ_CASES)
def test_vq_eval(ops, V, G, vd, combine):
    """Gates of test_gumbel_vq_eval_against_reference_fixture (tests/test_e2e_gpu.py): targets and gather exact,
    perplexities rtol 1e-5 / atol 1e-5, and bitwise the same from one launch to the next (the statistics kernel's comment
    promises a deterministic result; its four per-wave sums used to meet in LDS atomics, and at V = 320 two launches on the
    same logits gave 71.17044 and 71.17047).  Observed on one MI355X: relative difference to fp64 at most 4e-7."""
    logits, vars_, ties = R.vq_inputs(V, G, vd, combine)
    tgt, q, code, prob = R.vq_eval(logits, vars_, combine, groups=G, num_vars=V)
    out = torch.full((R.VQ_ROWS, G * vd), SENT, device="cuda")
    targets = torch.full((R.VQ_ROWS, G), -5, dtype=torch.int32, device="cuda")
    stats = torch.full((2,), SENT, device="cuda")
    ld = dev(logits)
    assert ld.stride(0) > G * V
    ops.vq_eval(ld, dev(vars_), combine, out, targets, stats, G, V)
    for (r, gi), (idx, want) in ties.items():
        assert int(targets[r, gi]) == want, f"maxima at {idx[:4]} of row {r} group {gi}: got {int(targets[r, gi])}"
    assert torch.equal(targets.cpu(), tgt)
    assert torch.equal(out.cpu(), q)
    print(f"vq_eval V={V} G={G}: perplexities kernel {stats.tolist()}, fp64 {[float(code), float(prob)]}")
    torch.testing.assert_close(stats.cpu(), torch.stack([code, prob]).float(), rtol=1e-5, atol=1e-5)
    out2, stats2 = torch.full((R.VQ_ROWS, G * vd), SENT, device="cuda"), torch.full((2,), SENT, device="cuda")
    for _ in range(3):
        ops.vq_eval(ld, dev(vars_), combine, out2, targets, stats2, G, V)
        assert torch.equal(stats2, stats)
    out2.fill_(SENT)
    ops.vq_eval(ld, dev(vars_), combine, out2, targets, None, G, V)                  # without the statistics kernel
    assert torch.equal(out2, out)


def test_vq_eval_statistics_limit(ops, F5EError):
    """num_vars = 2048 is the statistics kernel's limit (5 x 2048 floats of LDS): accepted and right; 2049 is refused before
    the lookup is launched (out and targets keep their fill)."""
    logits, vars_, _ = R.vq_inputs(2048, 1, 8, False)
    tgt, q, code, prob = R.vq_eval(logits, vars_, False, groups=1, num_vars=2048)
    out = torch.full((R.VQ_ROWS, 8), SENT, device="cuda")
    targets = torch.full((R.VQ_ROWS, 1), -5, dtype=torch.int32, device="cuda")
    stats = torch.full((2,), SENT, device="cuda")
    ops.vq_eval(dev(logits), dev(vars_), False, out, targets, stats, 1, 2048)
    assert torch.equal(targets.cpu(), tgt) and torch.equal(out.cpu(), q)
    torch.testing.assert_close(stats.cpu(), torch.stack([code, prob]).float(), rtol=1e-5, atol=1e-5)
    out.fill_(SENT)
    targets.fill_(-5)
    with pytest.raises(F5EError):
        ops.vq_eval(torch.zeros(R.VQ_ROWS, 2049 + 12, device="cuda"), torch.zeros(2049, 8, device="cuda"), False, out, targets,
                    stats, 1, 2049)
    assert bool((out == SENT).all()) and bool((targets == -5).all())


# ------------------------------------------------------------------ bigvgan.hip: conv_post

@pytest.mark.parametrize("C,L", R.POST_CASES)
def test_bigvgan_post(ops, C, L):
    """No earlier gate: 4x the fp32 restatement + one ulp, for the clamp, the tanh and bias = None; where the fp64
    pre-activation is past +-1 by more than that, the clamp gives exactly +-1."""
    a, w, bias = R.post_inputs(C, L)
    ad, wd, bd = dev(a), dev(w), dev(bias)
    pre = R.conv_post(a, w, bias, pre=True)
    for tanh, b, bdv in ((False, bias, bd), (True, bias, bd), (False, None, None)):
        out = torch.full((R.POST_B, L), SENT, device="cuda")
        ops.bigvgan_post(ad, wd, bdv, out, tanh)
        gated(f"bigvgan_post C={C} L={L} tanh={tanh} bias={b is not None}", out, R.conv_post(a, w, b, None, tanh),
              R.conv_post(a, w, b, None, tanh, dtype=F32))
        if not tanh and b is not None:
            o = out.cpu()
            assert bool((o[pre > 1.001] == 1.0).all()) and bool((o[pre < -1.001] == -1.0).all()) and float(o.abs().max()) <= 1.0
