"""Direct parity, containment and refusals of the DiT sampler's front- and back-end kernels: f5e_convpos (both kernels), the
three STFT log-mel entry points, f5e_istft_head, f5e_sinus_embed and f5e_rope_table, called through f5e_tts_amd.ops, against
the fp64 restatements of tests/frontend_ops_ref.py (pinned on the CPU by tests/test_frontend_ops_cpu.py).

Case -> path (what nothing else in the suite executes):
  test_convpos                   every (D, G, N) of R.CONVPOS_CASES on the split-tap kernel (S = 2) AND on the ring kernel
                                 (S = CUs // (G tiles) + 1): N = 1 .. 17 (both zero paddings inside one halo), 63 / 64 / 65 and
                                 128 / 129 (one row in the last tile), groups of 16 / 32 / 48 channels (zero-padded weights,
                                 the ``c0 + c * 8 < D`` guard), ldx / ldo / ldo32 / ldr != D, both branches of mish's
                                 threshold; operands with an order-independent fp32 result, so mode 0 is held to the correctly
                                 rounded bf16 and the two kernels to each other bit for bit
  test_convpos_graph_replay      both kernels and modes captured and replayed
  test_stft_logmel               nw = 513 (a frame that reflects at both ends), nw % hop != 0, a hop that does not divide
                                 1024, ldw = nw + 3, 1 / 100 / 256 filters, impulses next to both edges, silence; dense ==
                                 banded on every case
  test_stft_logmel_ex            pad_left 0 / 384 / 512 / nw - 1, T = 1 and the largest admitted T, mag_eps 0 / 1e-9
  test_istft_head                T = 2 (the minimum) .. 33, hop 128 / 256 / 512, ldz = 1030, the exp clip at and next to
                                 log(100), phases up to +-1e3, non-zero DC / Nyquist phases
  test_sinus_embed, test_rope_table      dim 4 / 256 / 258, E 1 / 33, scale 1 / 1000; N 1 / 469 / 4096
  test_*_refusals                every host-side refusal (nothing is launched)

Gates.  Fixed conditions are torch.equal (sentinels, residuals, silence, dense == banded, _ex == banded, ring == split-tap,
graph replay == eager) and the bf16 interval membership.  Every tolerance is 4x the error of the fp32 CPU restatement
against fp64 on the same inputs (computed at run time) plus one fp32 ulp, plus |arg| 2^-23 relative for mish's one exp2;
each test prints the yardstick and the kernel's error side by side, and the observed pairs are in the docstrings."""
import ctypes as C
import math

import pytest
import torch

import frontend_ops_ref as R
from oracle import f5e_oracle as O

pytestmark = pytest.mark.gpu

BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
ULP = 2.0 ** -23
SENT = R.SENTINEL
NAN = float("nan")
GUARD = 64                                          # sentinel elements in front of and behind a contained buffer


@pytest.fixture(scope="module")
def ops():
    import f5e_tts_amd.ops as ops_mod
    ops_mod.require_device()
    return ops_mod


@pytest.fixture(scope="module")
def F5EError():
    from f5e_tts_amd import _C
    return _C.F5EError


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev(t):
    return t.cuda().contiguous()


def gated(what, got, ref64, ref32, rel=ULP, abs_extra=0.0):
    """|kernel - fp64| <= 4 max|fp32 restatement - fp64| + abs_extra + rel |fp64|, element by element (rel: a number or a
    tensor).  -> the gate, per element."""
    got, ref32 = got.double().cpu().reshape(ref64.shape), ref32.double().reshape(ref64.shape)
    yard = float((ref32 - ref64).abs().max())
    err = (got - ref64).abs()
    print(f"{what}: fp32 restatement vs fp64 {yard:.3e}, kernel vs fp64 {float(err.max()):.3e}")
    gate = 4 * yard + abs_extra + rel * ref64.abs()
    bad = ~(err <= gate)
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} past the gate, max err {float(err.max()):.3e}, yardstick {yard:.3e}"
    return gate


def framed(t, pad, fill):
    """t [rows, cols] as the [1:-1, :cols] view of a device buffer [rows + 2, cols + pad] that holds ``fill`` elsewhere."""
    rows, cols = t.shape
    buf = torch.full((rows + 2, cols + pad), fill, device="cuda", dtype=t.dtype)
    view = buf[1:rows + 1, :cols]
    view.copy_(t)
    return buf, view


def frame_intact(buf, fill):
    rows, cols = buf.shape[0] - 2, buf.shape[1] - (8 if buf.dtype == BF else 4)
    frame = torch.ones(buf.shape, dtype=torch.bool, device="cuda")
    frame[1:rows + 1, :cols] = False
    v = buf[frame]
    return bool(torch.isnan(v).all()) if fill != fill else bool((v == fill).all())


def contained(shape, dtype=F32):
    """A contiguous device tensor of ``shape`` (NaN: every element must be written) inside a longer sentinel buffer."""
    n = math.prod(shape)
    flat = torch.full((n + 2 * GUARD,), SENT, device="cuda", dtype=dtype)
    flat[GUARD:GUARD + n] = NAN
    return flat, flat[GUARD:GUARD + n].view(shape)


def contained_ok(flat):
    n = flat.numel() - 2 * GUARD
    return bool((flat[:GUARD] == SENT).all()) and bool((flat[GUARD + n:] == SENT).all()) and \
        bool(torch.isfinite(flat[GUARD:GUARD + n]).all())


# ------------------------------------------------------------------ conv.hip: f5e_convpos

def cycle(t, S):
    """[2, N, D] -> [S N, D]: sequence i = t[i % 2]."""
    return t.repeat((S + 1) // 2, 1, 1)[:S].reshape(S * t.shape[1], t.shape[2])


@pytest.mark.parametrize("D,G,N", R.CONVPOS_CASES)
def test_convpos(ops, cus, D, G, N):
    """Exact operands (tests/frontend_ops_ref.py): the pre-activation is the same fp32 number in any summation order, so
    mode 1 with a zero residual is mish alone (gate: 4x the fp32 restatement of mish + one ulp + |arg| 2^-23 for the exp2;
    past the threshold 20 the output is the pre-activation itself), a seeded residual adds one ulp of the sum, mode 0 must
    lie in [rn_bf16(ref - g), rn_bf16(ref + g)] element by element, and the ring kernel's output equals the split-tap
    kernel's bit for bit.  x is a view inside NaN (never read), outputs and residual views inside sentinels (never written).
    Observed on one MI355X (fp32 restatement vs fp64 | kernel vs fp64, the same figures from both kernels): N = 1
    6.4e-8 | 6.4e-8; (128, 2) N 15 .. 200 1.7e-7 .. 3.3e-7 | 2.7e-7 .. 5.9e-7; (32, 2) 9.5e-8 .. 1.6e-7 | 2.2e-7 .. 2.7e-7;
    (1024, 16) 2.4e-7 .. 3.4e-7 | 3.3e-7 .. 5.4e-7 (the kernel at most 2.4x the restatement).  Mode 0: 0.4 % (D = 1024) to 4.2 %
    (D = 32) of the elements have two admissible bf16 values, every other one is the correctly rounded bf16."""
    x, w, bias, _ = R.convpos_inputs(D, G, N)
    pre = R.convpos_pre(x, w, bias, G)                                   # [2, N, D] fp64, exact
    ref64, ref32 = R.mish(pre), R.mish(pre, F32)
    arg = pre.abs().clamp(max=20.0)
    res = torch.randn(2, N, D, generator=R.g(7 * D + N))
    wp, bd = dev(ops.pack_convpos_weight(w, G)), dev(bias)
    runs = {}
    for kern, S in (("split", R.CONVPOS_S_SPLIT), ("ring", R.convpos_s_ring(G, N, cus))):
        assert R.convpos_kernel(G, N, S, cus) == kern and S >= 2
        xbuf, xv = framed(cycle(x, S).to(BF), 8, NAN)
        xbits = xbuf.view(torch.int16).clone()
        assert xv.stride(0) == D + 8
        r64, r32, a, p = cycle(ref64, S), cycle(ref32, S), cycle(arg, S), cycle(pre, S)
        # mode 1, zero residual: mish alone
        obuf, ov = framed(torch.full((S * N, D), NAN), 4, SENT)
        zbuf, zv = framed(torch.zeros(S * N, D), 4, SENT)
        ops.convpos(xv, wp, bd, S, N, out_f32=ov, resid=zv)
        gate = gated(f"convpos {kern} D={D} G={G} N={N} S={S} mode 1", ov, r64, r32, rel=ULP + a * ULP)
        o1 = ov.cpu()
        assert frame_intact(obuf, SENT) and frame_intact(zbuf, SENT) and float(zv.abs().max()) == 0
        assert torch.equal(o1[p > 20].double(), p[p > 20])               # mish_f's ``x > 20 ? x`` branch
        # mode 1, seeded residual
        obuf, ov = framed(torch.full((S * N, D), NAN), 4, SENT)
        rbuf, rv = framed(cycle(res, S), 4, SENT)
        rbits = rbuf.clone()
        ops.convpos(xv, wp, bd, S, N, out_f32=ov, resid=rv)
        want = r64 + cycle(res, S).double()
        err = (ov.double().cpu() - want).abs()
        assert bool((err <= gate + ULP * want.abs()).all()), f"mode 1 + residual: max err {float(err.max()):.3e}"
        o1r = ov.cpu()
        assert frame_intact(obuf, SENT) and torch.equal(rbuf, rbits)
        # mode 0: the correctly rounded bf16 of a value within the gate
        bbuf, bv = framed(torch.full((S * N, D), NAN, dtype=BF), 8, SENT)
        ops.convpos(xv, wp, bd, S, N, out_bf16=bv)
        o0 = bv.cpu()
        lo, hi = R.rn_bf16(r64 - gate).float(), R.rn_bf16(r64 + gate).float()
        inside = (o0.float() >= lo) & (o0.float() <= hi)
        print(f"convpos {kern} mode 0: {int((lo != hi).sum())}/{lo.numel()} elements with two admissible bf16 values")
        assert bool(inside.all()), f"mode 0: {int((~inside).sum())}/{inside.numel()} outside the rounding interval"
        assert frame_intact(bbuf, SENT) and torch.equal(xbuf.view(torch.int16), xbits)
        runs[kern] = (o0.view(S, N, D), o1.view(S, N, D), o1r.view(S, N, D))
    for a_, b_ in zip(runs["split"], runs["ring"]):                       # exact pre-activations: identical bits
        for i in range(b_.shape[0]):
            assert torch.equal(b_[i], a_[i % 2]), f"ring sequence {i} differs from the split-tap kernel's"


@pytest.mark.parametrize("kern", ["split", "ring"])
def test_convpos_graph_replay(ops, cus, kern):
    D, G, N = R.CONVPOS_GRAPH_CASE
    S = R.CONVPOS_S_SPLIT if kern == "split" else R.convpos_s_ring(G, N, cus)
    assert R.convpos_kernel(G, N, S, cus) == kern
    x, w, bias, _ = R.convpos_inputs(D, G, N)
    xd, wp, bd = dev(cycle(x, S).to(BF)), dev(ops.pack_convpos_weight(w, G)), dev(bias)
    rd = dev(cycle(torch.randn(2, N, D, generator=R.g(9)), S))
    e0, e1 = torch.zeros(S * N, D, device="cuda", dtype=BF), torch.zeros(S * N, D, device="cuda")
    ops.convpos(xd, wp, bd, S, N, out_bf16=e0)
    ops.convpos(xd, wp, bd, S, N, out_f32=e1, resid=rd)
    r0, r1 = torch.zeros_like(e0), torch.zeros_like(e1)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        gr = ops.Graph()
        gr.begin()
        try:
            ops.convpos(xd, wp, bd, S, N, out_bf16=r0)
            ops.convpos(xd, wp, bd, S, N, out_f32=r1, resid=rd)
        finally:
            gr.end()
        for _ in range(2):
            r0.zero_()
            r1.zero_()
            gr.launch()
            st.synchronize()
            assert torch.equal(r0, e0) and torch.equal(r1, e1)
        gr.destroy()


def test_convpos_refusals(ops, F5EError):
    """Host-side checks only: each raises before anything is launched, and the outputs keep their zeros."""
    from f5e_tts_amd import _C
    S, N, D, G = 2, 3, 64, 1
    rows = S * N
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)   # noqa: E731
    x, w, b = z(rows, D, dtype=BF), z(G, 31, 64, 64, dtype=BF), z(D)
    o16, o32, r = z(rows, D, dtype=BF), z(rows, D), z(rows, D)
    flat16, flat32 = z(rows * 72 + 16, dtype=BF), z(rows * 72 + 16)
    bad_x = (z(rows, D), torch.zeros(rows, D, dtype=BF), z(S, N, D, dtype=BF), z(rows + 1, D, dtype=BF), z(rows - 1, D, dtype=BF),
             z(rows, 2 * D, dtype=BF)[:, ::2], flat16[:rows * 68].view(rows, 68)[:, :D],
             flat16[4:4 + rows * 72].view(rows, 72)[:, :D])
    for t in bad_x:                                   # dtype, device, rank, rows, column stride, row stride % 8, alignment
        with pytest.raises(F5EError):
            ops.convpos(t, w, b, S, N, out_bf16=o16)
    bad_w = (z(G, 31, 64, 32, dtype=BF), z(G, 30, 64, 64, dtype=BF), z(G, 31, 64, 64), z(31, 64, 64, dtype=BF),
             z(G, 31, 64, 128, dtype=BF)[..., ::2], z(3, 31, 64, 64, dtype=BF),
             z(31 * 4096 + 8, dtype=BF)[4:4 + 31 * 4096].view(1, 31, 64, 64))
    for t in bad_w:                                   # shape, dtype, rank, contiguity, D % G, alignment
        with pytest.raises(F5EError):
            ops.convpos(x, t, b, S, N, out_bf16=o16)
    with pytest.raises(F5EError):                     # D / G = 128
        ops.convpos(z(rows, 128, dtype=BF), w, z(128), S, N, out_bf16=z(rows, 128, dtype=BF))
    with pytest.raises(F5EError):                     # D / G = 8
        ops.convpos(z(rows, 16, dtype=BF), z(2, 31, 64, 64, dtype=BF), z(16), S, N, out_bf16=z(rows, 16, dtype=BF))
    for t in (z(D - 1), z(D + 1), z(D, dtype=F64), z(1, D), z(2 * D)[::2], flat32[1:1 + D]):    # short bias ... misaligned
        with pytest.raises(F5EError):
            ops.convpos(x, w, t, S, N, out_bf16=o16)
    for kw in ({}, dict(out_bf16=o16, out_f32=o32, resid=r), dict(out_bf16=o16, resid=r), dict(out_f32=o32)):
        with pytest.raises(F5EError):
            ops.convpos(x, w, b, S, N, **kw)
    bad_o16 = (z(rows - 1, D, dtype=BF), z(rows, D + 8, dtype=BF), z(rows, D), z(rows, 2 * D, dtype=BF)[:, ::2],
               flat16[:rows * 66].view(rows, 66)[:, :D], flat16[1:1 + rows * 72].view(rows, 72)[:, :D])
    for t in bad_o16:                                 # too few rows, width, dtype, column stride, row stride % 4, alignment
        with pytest.raises(F5EError):
            ops.convpos(x, w, b, S, N, out_bf16=t)
    bad_o32 = (z(rows - 1, D), z(rows, D + 4), z(rows, D, dtype=BF), z(rows, 2 * D)[:, ::2],
               flat32[:rows * 66].view(rows, 66)[:, :D], flat32[1:1 + rows * 68].view(rows, 68)[:, :D])
    for t in bad_o32:
        with pytest.raises(F5EError):
            ops.convpos(x, w, b, S, N, out_f32=t, resid=r)
        with pytest.raises(F5EError):
            ops.convpos(x, w, b, S, N, out_f32=o32, resid=t)
    for bad_sn in ((0, 3), (2, 0), (3, 3)):
        with pytest.raises(F5EError):
            ops.convpos(x, w, b, *bad_sn, out_bf16=o16)
    # the library's own checks, behind the wrapper's: leading dimensions below D and misaligned bases
    lib, st = _C.lib(), torch.cuda.current_stream().cuda_stream
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)   # noqa: E731
    calls = ((P(x), D - 8, 0, P(o16), D, None, 0, None, 0), (P(x), D, 0, P(o16), D - 4, None, 0, None, 0),
             (P(x), D, 1, None, 0, P(o32), D - 4, P(r), D), (P(x), D, 1, None, 0, P(o32), D, P(r), D - 4),
             (P(x, 8), D, 0, P(o16), D, None, 0, None, 0), (P(x), D, 0, P(o16, 4), D, None, 0, None, 0),
             (P(x), D, 1, None, 0, P(o32, 8), D, P(r), D), (P(x), D, 1, None, 0, P(o32), D, P(r, 8), D))
    for xp, ldx, mode, op, ldo, o32p, ldo32, rp, ldr in calls:
        assert lib.f5e_convpos(st, xp, ldx, P(w), P(b), mode, op, ldo, o32p, ldo32, rp, ldr, S, N, D, G) != 0
    assert lib.f5e_convpos(st, P(x), D, P(w), P(b, 4), 0, P(o16), D, None, 0, None, 0, S, N, D, G) != 0
    torch.cuda.synchronize()
    for t in (o16, o32, flat16, flat32):
        assert float(t.float().abs().max()) == 0


# ------------------------------------------------------------------ fft.hip: STFT log-mel

STFT_PARAMS = [(nw, hop, 100) for nw, hop in R.STFT_CASES] + [R.STFT_MELS_CASE + (m,) for m in R.STFT_MELS if m != 100]
FLOOR = torch.tensor(1e-5).log()                    # logf(1e-5f), correctly rounded: -11.512925148 = 0xC13834F1


def is_floor(t):
    bits = sorted({hex(b & 0xFFFFFFFF) for b in t.cpu().view(torch.int32).flatten().tolist()})
    print(f"silence: output bit patterns {bits}, logf(1e-5f) is {hex(int(FLOOR.view(torch.int32)) & 0xFFFFFFFF)}")
    return bool((t.cpu() == FLOOR).all()) and len(bits) == 1


def strided_wav(wav):
    """wav [B, nw] as the [:, :nw] view of a device buffer [B, nw + 3] with NaN past every row."""
    buf = torch.full((wav.shape[0], wav.shape[1] + R.STFT_LD_PAD), NAN, device="cuda")
    buf[:, :wav.shape[1]] = wav.cuda()
    return buf[:, :wav.shape[1]]


def stft_tables(ops, n_mels):
    win, tw = R.fft_tables()
    fb = O.mel_filterbank_htk(n_mels=n_mels)
    band = ops.band_filterbank(dev(fb))
    assert band is not None and band[1].shape == (n_mels, 3)     # 1, 100 and 256 HTK filters all fit the banded kernel
    return win, tw, fb, band


@pytest.mark.parametrize("nw,hop,n_mels", STFT_PARAMS)
def test_stft_logmel(ops, nw, hop, n_mels):
    """Dense and banded against fp64 torch.stft of the explicitly reflect-padded signal, in the log domain: 4x the fp32
    radix-2 restatement + one ulp on the noise and impulse rows; the silent row is logf(1e-5f) exactly; dense == banded bit
    for bit; wav rows are ldw = nw + 3 apart with NaN between them; nothing around ``out`` is written.  Observed on one
    MI355X (fp32 restatement | kernel): (513, 256) 9.1e-7 | 9.9e-7, (1300, 256) 2.7e-6 | 2.6e-6, (2048, 100) 1.7e-6 | 1.7e-6,
    (1024, 512) 5.1e-7 | 6.7e-7; (1300, 256) with 1 filter 5.4e-7 | 1.0e-6, with 256 filters 6.2e-6 | 6.2e-6.  Silence: the
    device's logf(1e-5f) is not the correctly rounded 0xC13834F1, so the kernels store the floor as that constant."""
    win, tw, fb, band = stft_tables(ops, n_mels)
    wav = R.stft_wav(nw)
    T = 1 + nw // hop
    ref64, ref32 = R.logmel(wav, win, tw, fb, hop), R.logmel(wav, win, tw, fb, hop, dtype=F32)
    wv = strided_wav(wav)
    assert wv.stride(0) == nw + 3
    dflat, dense = contained((3, T, n_mels))
    bflat, banded = contained((3, T, n_mels))
    ops.stft_logmel(wv, dev(win), dev(tw), dev(fb), dense, 1024, hop)
    ops.stft_logmel_banded(wv, dev(win), dev(tw), band[0], band[1], banded, 1024, hop)
    assert contained_ok(dflat) and contained_ok(bflat)
    assert torch.equal(dense, banded)
    gated(f"stft_logmel nw={nw} hop={hop} mels={n_mels}", dense[:2], ref64[:2], ref32[:2])
    assert is_floor(dense[2])


@pytest.mark.parametrize("nw", R.STFT_EX_NW)
def test_stft_logmel_ex(ops, nw):
    """pad_left x T x mag_eps, same gate; silence is the floor exactly when mag_eps = 0 (with 1e-9 it is a value like any
    other and goes through the gate); _ex(512, 1 + nw // hop, 0) == _banded bit for bit.  Observed on one MI355X (fp32
    restatement | kernel) over the 30 combinations: 3.4e-7 .. 2.7e-6 | 4.7e-7 .. 2.8e-6, the kernel at most 1.7x the
    restatement (pad_left 384, T 1: 3.4e-7 | 5.6e-7)."""
    win, tw, fb, band = stft_tables(ops, 100)
    wav, hop = R.stft_wav(nw), R.STFT_EX_HOP
    wv, wd, td = strided_wav(wav), dev(win), dev(tw)
    for pad in R.stft_ex_pads(nw):
        for T in sorted({1, R.stft_ex_tmax(nw, hop, pad)}):
            for eps in R.STFT_EX_EPS:
                ref64 = R.logmel(wav, win, tw, fb, hop, pad, T, eps)
                ref32 = R.logmel(wav, win, tw, fb, hop, pad, T, eps, dtype=F32)
                flat, out = contained((3, T, 100))
                ops.stft_logmel_banded_ex(wv, wd, td, band[0], band[1], out, 1024, hop, pad, eps)
                assert contained_ok(flat)
                live = 3 if eps else 2
                gated(f"stft_logmel_ex nw={nw} pad_left={pad} T={T} eps={eps}", out[:live], ref64[:live], ref32[:live])
                if not eps:
                    assert is_floor(out[2])
    T = 1 + nw // hop
    plain, ex = torch.empty(3, T, 100, device="cuda"), torch.empty(3, T, 100, device="cuda")
    ops.stft_logmel_banded(dev(wav), wd, td, band[0], band[1], plain, 1024, hop)       # contiguous rows: ldw = nw
    ops.stft_logmel_banded_ex(dev(wav), wd, td, band[0], band[1], ex, 1024, hop, 512, 0.0)
    assert torch.equal(plain, ex)


def test_stft_refusals(ops, F5EError):
    nw, hop, T = 1300, 256, 6
    win, tw, fb, band = stft_tables(ops, 100)
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)   # noqa: E731
    wav, wd, td, fbd = z(2, nw), dev(win), dev(tw), dev(fb)
    out = z(2, T, 100)
    dense = lambda **k: ops.stft_logmel(k.get("wav", wav), k.get("win", wd), k.get("tw", td), k.get("fb", fbd),   # noqa: E731
                                        k.get("out", out), k.get("n_fft", 1024), k.get("hop", hop))
    banded = lambda **k: ops.stft_logmel_banded(k.get("wav", wav), k.get("win", wd), k.get("tw", td), k.get("fc", band[0]),   # noqa: E731
                                                k.get("fbb", band[1]), k.get("out", out), 1024, k.get("hop", hop))
    ex = lambda **k: ops.stft_logmel_banded_ex(k.get("wav", wav), k.get("win", wd), k.get("tw", td), k.get("fc", band[0]),   # noqa: E731
                                               k.get("fbb", band[1]), k.get("out", out), 1024, hop, k.get("pad", 384), 1e-9)
    common = (dict(wav=z(2, nw, dtype=F64)), dict(wav=z(nw)), dict(wav=z(2, 2 * nw)[:, ::2]), dict(wav=torch.zeros(2, nw)),
              dict(win=z(1023)), dict(win=z(1025)), dict(win=z(1024, dtype=F64)), dict(tw=z(512)), dict(tw=z(511, 2)),
              dict(tw=z(512, 4)[:, ::2]), dict(out=z(2, T, 101)), dict(out=z(1, T, 100)),
              dict(out=z(2, T, 200)[..., ::2]), dict(out=z(2, T, 100, dtype=F64)), dict(out=z(2 * T, 100)))
    for k in common:
        for call in (dense, banded, ex):
            with pytest.raises(F5EError):
                call(**k)
    for k in (dict(out=z(2, T + 1, 100)), dict(out=z(2, T - 1, 100)), dict(hop=0), dict(wav=z(2, 512), out=z(2, 3, 100))):     # T = 1 + nw // hop exactly
        for call in (dense, banded):
            with pytest.raises(F5EError):
                call(**k)
    for k in (dict(fb=z(512, 100)), dict(fb=z(513, 200)[:, ::2]), dict(fb=z(513, 100, dtype=F64)), dict(fb=z(513, 257), out=z(2, T, 257)),
              dict(n_fft=512)):
        with pytest.raises(F5EError):
            dense(**k)
    for k in (dict(fbb=z(100, 2, dtype=I32)), dict(fbb=band[1].long()), dict(fbb=z(99, 3, dtype=I32)), dict(fc=z(2049)),
              dict(fc=z(10, 10)), dict(fc=band[0].double())):
        for call in (banded, ex):
            with pytest.raises(F5EError):
                call(**k)
    for k in (dict(pad=nw), dict(pad=-1), dict(out=z(2, 20, 100))):                               # the library's reflect-once rules
        with pytest.raises(F5EError):
            ex(**k)
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0


# ------------------------------------------------------------------ fft.hip: iSTFT head

@pytest.mark.parametrize("hop", R.ISTFT_HOP)
@pytest.mark.parametrize("T", R.ISTFT_T)
def test_istft_head(ops, T, hop):
    """Against fp64 torch.istft(center=True): 4x the fp32 radix-2 restatement + one ulp of max|ref| (every output is a
    quotient of sums over all 513 bins, so the absolute part is scaled by the case, not the element).  z is a [:, :1026]
    view of rows 1030 apart with NaN between them; frames_ws and out are written in full and nothing around them is.
    Observed on one MI355X (fp32 restatement | kernel) on outputs up to 3: T 2 1.6e-7 .. 3.6e-7 | 1.3e-7 .. 3.6e-7, T 3
    2.1e-7 .. 3.6e-7 | 2.2e-7 .. 4.6e-7, T 9 2.3e-7 .. 4.6e-7 | 2.3e-7 .. 4.9e-7, T 33 2.4e-7 .. 4.7e-7 | 2.4e-7 .. 5.1e-7."""
    win, tw = R.fft_tables()
    z, B = R.istft_inputs(T), R.ISTFT_B
    ref64, ref32 = R.istft_head(z, win, tw, B, T, hop), R.istft_head(z, win, tw, B, T, hop, dtype=F32)
    zbuf = torch.full((B * T, R.ISTFT_LDZ), NAN, device="cuda")
    zbuf[:, :1026] = z.cuda()
    fflat, frames = contained((B * T * 1024,))
    oflat, out = contained((B, hop * (T - 1)))
    ops.istft_head(zbuf[:, :1026], dev(win), dev(tw), frames, out, B, T, 1024, hop)
    assert contained_ok(fflat) and contained_ok(oflat)
    gated(f"istft_head T={T} hop={hop}", out, ref64, ref32, rel=0.0, abs_extra=ULP * float(ref64.abs().max()))


def test_istft_refusals(ops, F5EError):
    B, T, hop = 2, 3, 256
    win, tw = R.fft_tables()
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)   # noqa: E731
    zz, wd, td, fr, out = z(B * T, 1026), dev(win), dev(tw), z(B * T * 1024), z(B, hop * (T - 1))
    call = lambda **k: ops.istft_head(k.get("z", zz), k.get("win", wd), k.get("tw", td), k.get("fr", fr), k.get("out", out),   # noqa: E731
                                      B, k.get("T", T), k.get("n_fft", 1024), k.get("hop", hop))
    for k in (dict(z=z(B * T - 1, 1026)), dict(z=z(B * T + 1, 1026)), dict(z=z(B * T, 1025)), dict(z=z(B * T, 2052)[:, ::2]),
              dict(z=z(B * T, 1026, dtype=F64)), dict(z=z(B, T, 1026)), dict(fr=z(B * T * 1024 - 1)), dict(fr=z(B * T * 2048)[::2]),
              dict(out=z(B, hop * (T - 1) - 1)), dict(out=z(B, hop * T)), dict(out=z(B, 2 * hop * (T - 1))[:, ::2]),
              dict(out=z(B * hop * (T - 1))), dict(win=z(1023)), dict(tw=z(512)), dict(T=1, z=z(B, 1026), out=z(B, 0)),
              dict(n_fft=512), dict(hop=300, out=z(B, 600)), dict(hop=0, out=z(B, 0))):
        with pytest.raises(F5EError):
            call(**k)
    with pytest.raises(F5EError, match="envelope.*NOLA"):             # hop = n_fft: out[b][512 + 1024 f] would be 0 / 0
        call(hop=1024, out=z(B, 1024 * (T - 1)))
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0 and float(fr.abs().max()) == 0


# ------------------------------------------------------------------ elementwise.hip: sinus_embed, rope_table

def sincos_gate(what, got, arg32, ref64, parts32):
    """4x the error of torch.sin / torch.cos in fp32 on the same fp32 arguments, plus one fp32 ulp of 1."""
    yard = max(float((p.double() - r).abs().max()) for p, r in parts32)
    err = (got.double().cpu() - ref64).abs()
    print(f"{what}: |arg| up to {float(arg32.abs().max()):.1f}, fp32 torch sin/cos vs fp64 {yard:.3e}, kernel vs fp64 {float(err.max()):.3e}")
    assert bool((err <= 4 * yard + ULP).all()), f"{what}: max err {float(err.max()):.3e}, yardstick {yard:.3e}"


@pytest.mark.parametrize("dim,E,scale", R.SINUS_CASES)
def test_sinus_embed(ops, dim, E, scale):
    """The argument (scale t) freqs is two fp32 products and no add: the CPU forms the same bits, so the comparison is
    held to the accuracy of sincosf itself.  Observed on one MI355X (torch.sin / cos in fp32 | kernel, against fp64):
    scale 1000 (|arg| up to 1000) 2.0e-8 .. 3.6e-8 | 3.9e-8 .. 6.3e-8, scale 1 3.0e-8 .. 3.6e-8 | 2.9e-8 .. 4.6e-8; gate
    2.0e-7 .. 2.6e-7.  __sinf / __cosf in the kernel's place miss it at every case with scale 1000."""
    t, freqs = R.sinus_inputs(dim, E)
    arg = R.sinus_arg(t, freqs, scale)
    ref64 = R.sinus_embed(t, freqs, scale)
    flat, out = contained((E, dim))
    ops.sinus_embed(dev(t), dev(freqs), out, scale)
    assert contained_ok(flat)
    half = dim // 2
    sincos_gate(f"sinus_embed dim={dim} E={E} scale={scale}", out, arg, ref64,
                ((torch.sin(arg), ref64[:, :half]), (torch.cos(arg), ref64[:, half:])))
    zero = arg == 0
    assert bool((out.cpu()[:, :half][zero] == 0).all()) and bool((out.cpu()[:, half:][zero] == 1).all())   # t = 0: (0, 1) exactly


@pytest.mark.parametrize("N", R.ROPE_N)
def test_rope_table(ops, N):
    """Same gate; float(n) inv_freq[i] is one fp32 product.  Observed on one MI355X (torch | kernel): N 469 3.6e-8 | 6.1e-8,
    N 4096 (|arg| up to 4095) 3.6e-8 | 6.8e-8; N 1 is (1, 0) exactly."""
    inv = R.rope_inv_freq()
    arg = R.rope_arg(inv, N)
    ref64 = R.rope_table(inv, N)
    flat, out = contained((N, R.ROPE_HALF, 2))
    ops.rope_table(dev(inv), out)
    assert contained_ok(flat)
    sincos_gate(f"rope_table N={N}", out, arg, ref64, ((torch.cos(arg), ref64[..., 0]), (torch.sin(arg), ref64[..., 1])))
    assert bool((out[0, :, 0] == 1).all()) and bool((out[0, :, 1] == 0).all())


def test_sinus_rope_refusals(ops, F5EError):
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)   # noqa: E731
    E, dim = 5, 16
    out, cs = z(E, dim), z(7, 32, 2)
    for t, f, o in ((z(E + 1), z(8), out), (z(E - 1), z(8), out), (z(E), z(9), out), (z(E), z(7), out), (z(E, 1), z(8), out),
                    (z(E, dtype=F64), z(8), out), (z(E), z(8, dtype=F64), out), (z(2 * E)[::2], z(8), out), (z(E), z(16)[::2], out),
                    (torch.zeros(E), z(8), out), (z(E), z(8), z(E, 2 * dim)[:, ::2]), (z(E), z(8), z(E, dim, dtype=F64)),
                    (z(E), z(7), z(E, 15)), (z(E), z(1), z(E, 2)), (z(E * dim), z(8), z(E * dim))):
        with pytest.raises(F5EError):
            ops.sinus_embed(t, f, o)
    for inv, o in ((z(31), cs), (z(33), cs), (z(32, dtype=F64), cs), (z(64)[::2], cs), (z(1, 32), cs), (z(32), z(7, 32, 3)),
                   (z(32), z(7, 64)), (z(32), z(7, 32, 4)[..., ::2]), (z(32), z(7, 32, 2, dtype=F64)), (torch.zeros(32), cs)):
        with pytest.raises(F5EError):
            ops.rope_table(inv, o)
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0 and float(cs.abs().max()) == 0
