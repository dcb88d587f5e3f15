"""tests/frontend_ops_ref.py held to independent torch calls, the shared inputs checked for the properties the GPU cases of
tests/test_frontend_ops_gpu.py rely on (exact convpos operands, both mish branches, no empty mel bin, planted iSTFT values),
and the coverage tables: both convpos kernels x every group width x both modes x every N class, and every STFT / iSTFT case
class of the issue."""
import math

import pytest
import torch
import torch.nn.functional as F

import frontend_ops_ref as R

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16


def rel_l2(a, b):
    return float((a - b).abs().double().norm() / b.abs().double().norm())


# ------------------------------------------------------------------ convpos

@pytest.mark.parametrize("D,G,N", R.CONVPOS_CASES)
def test_convpos_operands_are_exact_in_any_order(D, G, N):
    """fp32 conv + bias equals the fp64 result bit for bit, in torch's order and with taps and channels reversed; the
    pre-activations are multiples of 2^-6 bounded far below 2^24 of them; both branches of the threshold 20 are reached."""
    x, w, bias, gp = R.convpos_inputs(D, G, N)
    cpg = D // G
    assert torch.equal(x.to(BF).float(), x) and torch.equal(w.to(BF).float(), w)         # exact in bf16
    assert torch.equal(x, x.round()) and torch.equal(w * 64, (w * 64).round()) and torch.equal(bias * 64, (bias * 64).round())
    assert float(x.abs().max()) <= 2 and float(w.abs().max()) <= 2 / 64
    assert 31 * cpg * 4 + 64 * R.MISH_PLANT < 2 ** 24                                     # 64 |any partial sum| at the worst
    pre = R.convpos_pre(x, w, bias, G)
    assert torch.equal(R.convpos_pre(x, w, bias, G, dtype=F32).double(), pre)
    assert torch.equal(R.convpos_pre_reversed(x, w, bias, G).double(), pre)
    assert torch.equal(pre * 64, (pre * 64).round())
    assert float(pre.max()) > 20 and float(pre.min()) < -20
    lo, hi = gp * cpg + 1, gp * cpg + cpg - 2
    rest = torch.ones(D, dtype=torch.bool)
    rest[[lo, hi]] = False
    assert float(pre[..., rest].abs().max()) < 20                                         # only the planted channels pass it


def test_convpos_reference_against_a_tap_loop():
    """The grouped conv1d call against the definition, one output row at a time, zeros outside the sequence."""
    D, G, N = 96, 3, 17
    x, w, bias, _ = R.convpos_inputs(D, G, N)
    cpg = D // G
    want = torch.zeros(2, N, D, dtype=F64)
    for s in range(2):
        for t in range(N):
            for k in range(31):
                tj = t + k - 15
                if 0 <= tj < N:
                    for gi in range(G):
                        want[s, t, gi * cpg:(gi + 1) * cpg] += w[gi * cpg:(gi + 1) * cpg, :, k].double() @ \
                            x[s, tj, gi * cpg:(gi + 1) * cpg].double()
    assert torch.equal(R.convpos_pre(x, w, bias, G), want + bias.double())


def test_mish_and_bf16_rounding_references():
    v = torch.cat((torch.linspace(-40, 40, 4001, dtype=F64), torch.tensor([20.0, 20.0 + 2 ** -40, 24.0, -24.0], dtype=F64)))
    assert float((R.mish(v) - F.mish(v)).abs().max()) <= 1e-15 * 40
    assert torch.equal(R.mish(v)[v > 20], v[v > 20])                  # past the threshold mish is the identity in fp64 too
    f = torch.randn(20000, generator=R.g(1)) * 5
    ties = torch.tensor([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0, 0x00008000], dtype=torch.int32).view(F32)
    f = torch.cat((f, ties, -ties))
    assert torch.equal(R.rn_bf16(f.double()), f.to(BF))
    # between fp32's grid points: 1 + 2^-8 + 2^-40 is past the tie and rounds up although its fp32 rounding is the tie itself
    assert float(R.rn_bf16(torch.tensor([1 + 2.0 ** -8 + 2.0 ** -40], dtype=F64))) == 1 + 2.0 ** -7
    assert float(R.rn_bf16(torch.tensor([1 + 2.0 ** -8 - 2.0 ** -40], dtype=F64))) == 1.0


def test_convpos_coverage_table():
    """With 256 CUs every (kernel, channels per group, mode, N class) cell is reached, each case lands on the kernel it
    names at S >= 2 sequences, and the guard ``c0 + c * 8 < D`` of the narrow groups is reached."""
    cells = set()
    for D, G, N in R.CONVPOS_CASES:
        s_ring = R.convpos_s_ring(G, N, 256)
        assert R.convpos_kernel(G, N, R.CONVPOS_S_SPLIT, 256) == "split" and R.convpos_kernel(G, N, s_ring, 256) == "ring"
        assert s_ring >= 2 and R.convpos_kernel(G, N, s_ring - 1, 256) == "split"        # the first S past the threshold
        assert s_ring * N * D <= 257 * 64 * 64 * 2
        for kern in ("split", "ring"):
            for mode in (0, 1):
                cells.add((kern, D // G, mode, R.convpos_n_class(N)))
    want = {(k, c, m, n) for k in ("split", "ring") for c in (16, 32, 48, 64) for m in (0, 1)
            for n in ("partial", "exact", "plus1", "multi")}
    assert cells == want, sorted(want - cells)
    assert {N for D, G, N in R.CONVPOS_CASES if (D, G) == (128, 2)} == set(R.CONVPOS_N)
    assert all((D, G, N) in R.CONVPOS_CASES for D, G in R.CONVPOS_DG for N in (17, 65, 130))
    assert any((G - 1) * (D // G) + 64 > D for D, G, _ in R.CONVPOS_CASES)               # last group's tile runs past D
    assert R.CONVPOS_GRAPH_CASE in R.CONVPOS_CASES


# ------------------------------------------------------------------ FFT restatement, STFT log-mel

def test_radix2_fft_against_torch_rfft():
    """The fp32 radix-2 restatement (forward and inverse) within 1e-5 relative L2 of torch's fp64 FFT; in fp64 it is exact
    to 1e-12 with fp64 twiddles."""
    win, tw = R.fft_tables()
    x = torch.randn(5, 1024, generator=R.g(2))
    ref = torch.fft.rfft(x.double())
    re, im = R.fft1024_radix2(x, torch.zeros_like(x), tw)
    assert rel_l2(torch.complex(re.double(), im.double())[:, :513], ref) < 1e-5
    k = torch.arange(512, dtype=F64)
    tw64 = torch.stack((torch.cos(2 * math.pi * k / 1024), -torch.sin(2 * math.pi * k / 1024)), -1)
    re, im = R.fft1024_radix2(x.double(), torch.zeros(5, 1024, dtype=F64), tw64)
    assert rel_l2(torch.complex(re, im)[:, :513], ref) < 1e-12
    full = torch.fft.fft(x.double())
    bre, bim = R.fft1024_radix2(full.real.float(), full.imag.float(), tw, inverse=True)
    assert rel_l2(bre / 1024, x) < 1e-5 and float(bim.abs().max()) < 1e-2


def filterbank(n_mels):
    from oracle import f5e_oracle as O
    return O.mel_filterbank_htk(n_mels=n_mels)


@pytest.mark.parametrize("nw,hop", R.STFT_CASES)
def test_logmel_references(nw, hop):
    """fp64 reference against torch.stft(center=True, pad_mode="reflect"); the fp32 radix-2 yardstick stays within 1e-4 of
    it in the log domain on the two live signals, and silence is the floor log(1e-5) exactly in both."""
    win, tw = R.fft_tables()
    fb = filterbank(100)
    wav = R.stft_wav(nw)
    ref = R.logmel(wav, win, tw, fb, hop)
    spec = torch.stft(wav.double(), 1024, hop, 1024, win.double(), center=True, pad_mode="reflect", return_complex=True)
    want = torch.log(torch.clamp(spec.abs().transpose(1, 2) @ fb.double(), min=1e-5))
    assert ref.shape == (3, 1 + nw // hop, 100) and float((ref - want).abs().max()) < 1e-11
    y32 = R.logmel(wav, win, tw, fb, hop, dtype=F32)
    assert y32.dtype == F32 and float((y32.double() - ref)[:2].abs().max()) < 1e-4
    floor = torch.tensor(1e-5).log()
    assert bool((y32[2] == floor).all()) and bool((ref[2] == math.log(1e-5)).all())
    assert float(ref[:2].min()) > math.log(1e-5) + 1                 # no live bin at the floor or made of round-off
    if nw == 513:                                                     # the middle frame reflects at both ends
        assert any(f * hop - 512 < 0 and f * hop + 511 >= nw for f in range(1 + nw // hop))


@pytest.mark.parametrize("nw", R.STFT_EX_NW)
def test_logmel_ex_reference_and_cases(nw):
    """pad_left / T / mag_eps: pad_left = 512 with the default T is the plain form; each frame equals an rfft of the
    hand-indexed reflected samples; the largest T touches the reflect-once limit."""
    win, tw = R.fft_tables()
    fb = filterbank(100)
    wav, hop = R.stft_wav(nw), R.STFT_EX_HOP
    assert torch.equal(R.logmel(wav, win, tw, fb, hop, 512, 1 + nw // hop, 0.0), R.logmel(wav, win, tw, fb, hop))
    assert set(R.stft_ex_pads(nw)) >= {0, 512, nw - 1} and (nw == 513 or 384 in R.stft_ex_pads(nw))
    for pad in R.stft_ex_pads(nw):
        tmax = R.stft_ex_tmax(nw, hop, pad)
        assert (tmax - 1) * hop - pad + 1023 <= 2 * (nw - 1) < tmax * hop - pad + 1023 and tmax >= 1
        for T in sorted({1, tmax}):
            for eps in R.STFT_EX_EPS:
                ref = R.logmel(wav, win, tw, fb, hop, pad, T, eps)
                i = torch.arange(1024) + (T - 1) * hop - pad           # the last frame, indexed by hand
                i = torch.where(i < 0, -i, i)
                i = torch.where(i >= nw, 2 * (nw - 1) - i, i)
                assert int(i.min()) >= 0 and int(i.max()) < nw
                sp = torch.fft.rfft(wav.double()[:, i] * win.double())
                want = torch.log(torch.clamp(torch.sqrt(sp.real ** 2 + sp.imag ** 2 + eps) @ fb.double(), min=1e-5))
                assert ref.shape == (3, T, 100) and float((ref[:, -1] - want).abs().max()) < 1e-11, (pad, T, eps)
                y32 = R.logmel(wav, win, tw, fb, hop, pad, T, eps, dtype=F32)
                assert float((y32.double() - ref)[:2].abs().max()) < 1e-4


def test_stft_case_classes():
    nws = {nw for nw, _ in R.STFT_CASES}
    assert (513, 256) in R.STFT_CASES and min(nws) == 513                               # the smallest allowed nw
    assert any(nw % hop for nw, hop in R.STFT_CASES) and any(1024 % hop for _, hop in R.STFT_CASES)
    assert (1024, 512) in R.STFT_CASES and R.STFT_MELS == (1, 100, 256) and R.STFT_MELS_CASE in R.STFT_CASES
    assert R.STFT_LD_PAD == 3 and set(R.STFT_EX_EPS) == {0.0, 1e-9}
    for m in R.STFT_MELS:                                                                # the banded form exists for each
        fb = filterbank(m)
        assert fb.shape == (513, m) and int((fb != 0).sum()) <= 2048 and float(fb.sum()) > 0


# ------------------------------------------------------------------ iSTFT head

@pytest.mark.parametrize("hop", R.ISTFT_HOP)
@pytest.mark.parametrize("T", R.ISTFT_T)
def test_istft_references(T, hop):
    """fp64 reference against irfft + overlap-add by hand (DC / Nyquist phases ignored); the fp32 yardstick within 1e-5 of
    max|ref|; the planted values are there."""
    win, tw = R.fft_tables()
    z = R.istft_inputs(T)
    B = R.ISTFT_B
    ref = R.istft_head(z, win, tw, B, T, hop)
    assert ref.shape == (B, hop * (T - 1))
    v = z.double()
    mag = torch.clamp(v[:, :513].exp(), max=100.0)
    re, im = mag * v[:, 513:].cos(), mag * v[:, 513:].sin()
    im[:, 0], im[:, 512] = 0.0, 0.0                                   # what irfft does with them, spelled out
    fr = (torch.fft.irfft(torch.complex(re, im), 1024) * win.double()).reshape(B, T, 1024)
    n = hop * (T - 1) + 1024
    acc, env = torch.zeros(B, n, dtype=F64), torch.zeros(n, dtype=F64)
    for f in range(T):
        acc[:, f * hop:f * hop + 1024] += fr[:, f]
        env[f * hop:f * hop + 1024] += win.double() ** 2
    want = (acc / env)[:, 512:512 + hop * (T - 1)]
    scale = float(ref.abs().max())
    assert float((ref - want).abs().max()) < 1e-12 * scale
    y32 = R.istft_head(z, win, tw, B, T, hop, dtype=F32)
    assert y32.dtype == F32 and float((y32.double() - ref).abs().max()) < 1e-5 * scale
    assert float(env[512:512 + hop * (T - 1)].min()) >= (0.5 if hop == 512 else 1.0) - 1e-6
    l100 = torch.tensor(R.LOG100)
    assert float(z[0, 3]) == R.LOG100 and float(z[0, 40]) > R.LOG100 > float(z[0, 41]) and float(z[0, 5]) == 9.0
    assert float(z[0, 40]) == float(torch.nextafter(l100, torch.tensor(9.0))) and float(z[0, 100]) == -30.0
    assert float(z[:, 513:].abs().max()) > 900 and float(z[:, 513].abs().min()) > 0 and float(z[:, 1025].abs().min()) > 0
    assert float(z[:, :513].max()) > R.LOG100                         # the clip decides somewhere


def test_istft_case_classes():
    assert R.ISTFT_T == (2, 3, 9, 33) and set(R.ISTFT_HOP) == {256, 128, 512} and R.ISTFT_LDZ == 1030 and R.ISTFT_B == 2
    w = torch.hann_window(1024).double()
    assert float(w[0]) == 0.0                                         # hop = 1024: out[b][512 + 1024 f] would be 0 / 0
    with pytest.raises(RuntimeError):                                 # torch refuses it (NOLA)
        torch.istft(torch.ones(1, 513, 3, dtype=torch.complex128), 1024, 1024, 1024, w, center=True)


# ------------------------------------------------------------------ sinus_embed, rope_table

@pytest.mark.parametrize("dim,E,scale", R.SINUS_CASES)
def test_sinus_reference(dim, E, scale):
    """Against the oracle's formula in fp64 (the argument differs by fp32 roundings only), and the argument itself against
    a scalar Python loop of fp32 products."""
    t, freqs = R.sinus_inputs(dim, E)
    assert t.shape == (E,) and freqs.shape == (dim // 2,) and (E * (dim // 2)) % 256 != 0
    arg = R.sinus_arg(t, freqs, scale)
    s32 = torch.tensor(scale, dtype=F32)
    for e in (0, E - 1):
        for k in (0, dim // 2 - 1):
            assert float(arg[e, k]) == float((s32 * t[e]) * freqs[k])
    ref = R.sinus_embed(t, freqs, scale)
    a64 = scale * t.double()[:, None] * freqs.double()[None]
    assert ref.shape == (E, dim) and float((ref - torch.cat((a64.sin(), a64.cos()), -1)).abs().max()) < 2e-4
    if E == 33:
        assert float(t[0]) == 0.0 and abs(float(t[-1]) - 1.0) < 1e-6


@pytest.mark.parametrize("N", R.ROPE_N)
def test_rope_reference(N):
    inv = R.rope_inv_freq()
    ref = R.rope_table(inv, N)
    ang = torch.outer(torch.arange(N).double(), inv.double())
    tol = 2.0 ** -24 * max(N - 1, 1) + 1e-15                           # the one fp32 rounding of the argument
    assert ref.shape == (N, 32, 2) and float((ref[..., 0] - ang.cos()).abs().max()) <= tol
    assert float((ref[..., 1] - ang.sin()).abs().max()) <= tol
    a32 = R.rope_arg(inv, N)
    assert float(a32[N - 1, 5]) == float(torch.tensor(float(N - 1)) * inv[5])
    assert float(a32.max()) == float(N - 1) and float((a32.double() - ang).abs().max()) <= 2.0 ** -24 * max(N - 1, 1)
