"""Plain PyTorch restatements of the DiT sampler's front- and back-end kernels (f5e_convpos of csrc/conv.hip, the STFT log-mel
entry points and f5e_istft_head of csrc/fft.hip, f5e_sinus_embed / f5e_rope_table of csrc/elementwise.hip), written from the
formula in each kernel's header comment, plus the seeded inputs and the case lists that tests/test_frontend_ops_cpu.py (pins
these restatements to independent torch calls, checks the inputs and the coverage) and tests/test_frontend_ops_gpu.py
(compares the HIP ops with them) share.

``dtype`` is the working precision: float64 for the reference, float32 for the yardstick that the GPU tests scale their gates
by.  The fp32 STFT / iSTFT yardsticks run the kernel's own algorithm (radix-2 decimation in time on bit-reversed input with
the fp32 twiddle table), not torch's FFT library, which is more accurate than any radix-2 fp32 FFT.  Nothing here imports
f5e_tts_amd."""
import math

import torch
import torch.nn.functional as F

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
SENTINEL = 77.0                                      # exact in bf16


def g(seed):
    return torch.Generator().manual_seed(seed)


# ================================================================== convpos

CONVPOS_DG = ((64, 1), (128, 2), (96, 3), (240, 5), (32, 2), (256, 16), (1024, 16))
CONVPOS_N = (1, 15, 16, 17, 49, 63, 64, 65, 79, 80, 128, 129, 130, 200)
# every N with (128, 2); every (D, G) with 17, 65, 130; and one exact tile for each narrow group width, so that the
# (kernel, cpg, mode, N class) table of test_frontend_ops_cpu.py has no empty cell
CONVPOS_CASES = tuple((128, 2, N) for N in CONVPOS_N) \
    + tuple((D, G, N) for D, G in CONVPOS_DG if (D, G) != (128, 2) for N in (17, 65, 130)) \
    + ((96, 3, 64), (240, 5, 64), (32, 2, 64))
CONVPOS_GRAPH_CASE = (128, 2, 65)
CONVPOS_S_SPLIT = 2
MISH_PLANT = 24.0                                    # bias of the two planted channels: pre-activations past +-20


def convpos_tiles(N):
    return (N + 63) // 64


def convpos_kernel(G, N, S, cus):
    """The dispatch rule of f5e_convpos: a grid that fits the chip in one round takes the split-tap kernel, any larger one
    the output-split ring kernel."""
    return "split" if G * convpos_tiles(N) * S <= cus else "ring"


def convpos_s_ring(G, N, cus):
    return cus // (G * convpos_tiles(N)) + 1


def convpos_n_class(N):
    return "partial" if N < 64 else "exact" if N % 64 == 0 else "plus1" if N % 64 == 1 else "multi"


def convpos_inputs(D, G, N):
    """x [2, N, D] integers in [-2, 2], w [D, D / G, 31] integers in [-2, 2] / 64, bias [D] integers in [-64, 64] / 64, with
    +24 and -24 planted on two channels of one group: every product and partial sum is a multiple of 2^-6 far below 2^24
    of them, so conv + bias is the same fp32 number in any summation order.  -> x, w, bias, planted group."""
    cpg = D // G
    seed = 1000 * D + 10 * N + G
    x = torch.randint(-2, 3, (CONVPOS_S_SPLIT, N, D), generator=g(seed)).float()
    w = torch.randint(-2, 3, (D, cpg, 31), generator=g(seed + 1)).float() / 64
    bias = torch.randint(-64, 65, (D,), generator=g(seed + 2)).float() / 64
    gp = (N + D) % G
    bias[gp * cpg + 1], bias[gp * cpg + cpg - 2] = MISH_PLANT, -MISH_PLANT
    return x, w, bias, gp


def convpos_pre(x, w, bias, G, dtype=F64):
    """conv + bias, [S, N, D]: grouped Conv1d(D, D, 31, padding 15) over each sequence on its own, zeros outside it."""
    y = F.conv1d(x.to(dtype).permute(0, 2, 1), w.to(dtype), bias.to(dtype), padding=15, groups=G)
    return y.permute(0, 2, 1).contiguous()


def convpos_pre_reversed(x, w, bias, G):
    """The same in fp32 with the taps and the channels of a group taken in descending order, one tap at a time."""
    S, N, D = x.shape
    cpg = D // G
    xp = F.pad(x, (0, 0, 15, 15)).reshape(S, N + 30, G, cpg).flip(-1)
    wg = w.reshape(G, cpg, cpg, 31).flip(2)                       # [g, oc, ic (descending), tap]
    acc = torch.zeros(S, N, G, cpg)
    for k in reversed(range(31)):
        acc += torch.einsum("sngc,goc->sngo", xp[:, k:k + N], wg[..., k])
    return acc.reshape(S, N, D) + bias


def mish(v, dtype=F64):
    """v tanh(softplus(v)), softplus with torch's threshold 20 (mish_f of f5e_common.h returns v itself past it)."""
    v = v.to(dtype)
    sp = torch.where(v > 20, v, torch.log1p(torch.exp(torch.clamp(v, max=20.0))))
    return v * torch.tanh(sp)


def rn_bf16(v):
    """fp64 -> the nearest bf16 (ties to even), rounded once: through fp32 a value next to a bf16 tie could round twice."""
    v = v.double()
    bits = v.float().view(torch.int32)
    lo = (bits & -65536).view(F32)                               # the bf16 neighbour towards zero, and the one away from it
    hi = ((bits & -65536) + 65536).view(F32)
    dlo, dhi = (v - lo.double()).abs(), (hi.double() - v).abs()
    pick_lo = (dlo < dhi) | ((dlo == dhi) & (((bits >> 16) & 1) == 0))
    return torch.where(pick_lo, lo, hi).to(BF)


# ================================================================== STFT log-mel

NFFT, NBIN = 1024, 513
STFT_CASES = ((513, 256), (1300, 256), (2048, 100), (1024, 512))   # (nw, hop): one frame reflects at both ends | nw % hop | 1024 % hop
STFT_MELS_CASE = (1300, 256)                                        # the shape that also runs with 1 and 256 filters
STFT_MELS = (1, 100, 256)
STFT_EX_NW = (513, 1300)
STFT_EX_HOP = 256
STFT_EX_EPS = (0.0, 1e-9)
STFT_LD_PAD = 3


def fft_tables():
    """(periodic Hann window [1024], twiddles [512, 2] = (cos, -sin)(2 pi k / 1024)) in fp32, as engine.fft_tables."""
    k = torch.arange(512, dtype=F64)
    tw = torch.stack((torch.cos(2 * math.pi * k / 1024), -torch.sin(2 * math.pi * k / 1024)), -1).float()
    return torch.hann_window(1024), tw


def stft_ex_pads(nw):
    return tuple(sorted({0, 384, 512, nw - 1} & set(range(nw))))


def stft_ex_tmax(nw, hop, pad_left):
    """The largest T of the library's reflect-once rule (T - 1) hop - pad_left + 1023 <= 2 (nw - 1)."""
    return (2 * (nw - 1) + pad_left - (NFFT - 1)) // hop + 1


def stft_wav(nw):
    """[3, nw]: white noise of amplitude 0.3 | unit impulses at 0, 1, 511, 512, nw - 2, nw - 1 on a 1e-3 noise floor |
    silence.  No mel bin of the first two is round-off leakage: every FFT bin holds signal."""
    wav = torch.zeros(3, nw)
    wav[0] = 0.3 * torch.randn(nw, generator=g(300 + nw))
    wav[1] = 1e-3 * torch.randn(nw, generator=g(301 + nw))
    wav[1, [0, 1, 511, 512, nw - 2, nw - 1]] = 1.0
    return wav


BITREV = torch.tensor([int(f"{i:010b}"[::-1], 2) for i in range(NFFT)])


def fft1024_radix2(re, im, tw, inverse=False):
    """fft1024 of fft.hip in the dtype of its operands: in-place radix-2 decimation in time over [..., 1024], input taken in
    bit-reversed order, stage s pairs i0 and i0 + 2^(s-1) with the twiddle tw[pos << (10 - s)] (conjugated for the inverse,
    which is not scaled)."""
    re, im = re[..., BITREV], im[..., BITREV]
    lead = re.shape[:-1]
    for s in range(1, 11):
        half = 1 << (s - 1)
        w = tw[torch.arange(half) << (10 - s)].to(re.dtype)
        wr, wi = w[:, 0], (-w[:, 1] if inverse else w[:, 1])
        re, im = re.reshape(*lead, NFFT >> s, 2, half), im.reshape(*lead, NFFT >> s, 2, half)
        ur, ui, vr, vi = re[..., 0, :], im[..., 0, :], re[..., 1, :], im[..., 1, :]
        tr, ti = wr * vr - wi * vi, wr * vi + wi * vr
        re = torch.stack((ur + tr, ur - tr), -2).reshape(*lead, NFFT)
        im = torch.stack((ui + ti, ui - ti), -2).reshape(*lead, NFFT)
    return re, im


def stft_frames(wav, hop, pad_left, T, dtype):
    """[B, T, 1024]: frame f = samples [f hop - pad_left, f hop - pad_left + 1024) of the reflect-padded signal."""
    B, nw = wav.shape
    right = (T - 1) * hop - pad_left + NFFT - nw
    p = F.pad(wav.to(dtype)[:, None], (pad_left, max(right, 0)), mode="reflect")[:, 0]
    return p[:, :(T - 1) * hop + NFFT].unfold(1, NFFT, hop)


def logmel(wav, window, tw, fb, hop, pad_left=NFFT // 2, T=None, mag_eps=0.0, dtype=F64):
    """log(clamp(sqrt(|STFT|^2 + mag_eps) . fb, 1e-5)) -> [B, T, n_mels]; T = 1 + nw // hop unless given.  fp64: torch.stft
    (center=False) of the explicitly reflect-padded signal; fp32: the kernel's radix-2 FFT with the fp32 twiddle table."""
    B, nw = wav.shape
    T = 1 + nw // hop if T is None else T
    if dtype == F64:
        right = (T - 1) * hop - pad_left + NFFT - nw
        p = F.pad(wav.double()[:, None], (pad_left, max(right, 0)), mode="reflect")[:, 0][:, :(T - 1) * hop + NFFT]
        spec = torch.stft(p, NFFT, hop, NFFT, window.double(), center=False, return_complex=True).transpose(1, 2)
        power = spec.real ** 2 + spec.imag ** 2
    else:
        fr = stft_frames(wav, hop, pad_left, T, dtype) * window.to(dtype)
        re, im = fft1024_radix2(fr, torch.zeros_like(fr), tw)
        power = (re * re + im * im)[..., :NBIN]
    mag = torch.sqrt(power + mag_eps) if mag_eps else torch.sqrt(power)
    return torch.log(torch.clamp(mag @ fb.to(dtype), min=1e-5))


# ================================================================== iSTFT head

ISTFT_T = (2, 3, 9, 33)
ISTFT_HOP = (256, 128, 512)
ISTFT_B, ISTFT_LDZ = 2, 1030
LOG100 = float(torch.tensor(100.0).log())                            # the fp32 nearest log(100)


def istft_inputs(T):
    """z [2 T, 1026] (513 log-magnitudes | 513 phases): log-magnitudes 1.5 N(0, 1) + 1 with log(100), one fp32 ulp either
    side of it, 9.0 and -30 planted in every row; phases N(0, 1), every fifth bin uniform in +-1e3 (DC and Nyquist too)."""
    rows = ISTFT_B * T
    z = torch.randn(rows, 2 * NBIN, generator=g(400 + T))
    z[:, :NBIN] = z[:, :NBIN] * 1.5 + 1.0
    l100 = torch.tensor(LOG100)
    up, dn = torch.nextafter(l100, torch.tensor(9.0)), torch.nextafter(l100, torch.tensor(0.0))
    for col, val in ((3, l100), (40, up), (41, dn), (5, 9.0), (100, -30.0), (512, 9.0)):
        z[:, col] = val
    big = (torch.rand(rows, NBIN, generator=g(401 + T)) * 2 - 1) * 1e3
    z[:, NBIN::5] = big[:, ::5]
    return z


def istft_head(z, window, tw, B, T, hop, dtype=F64):
    """mag = min(exp(.), 100), S = mag (cos p + i sin p), irfft * window, overlap-add / window envelope, trimmed by 512 at
    both ends -> [B, hop (T - 1)].  fp64: torch.istft(center=True); fp32: the kernel's radix-2 inverse and its two loops."""
    v = z.to(dtype)
    mag = torch.clamp(torch.exp(v[:, :NBIN]), max=100.0)
    re, im = mag * torch.cos(v[:, NBIN:2 * NBIN]), mag * torch.sin(v[:, NBIN:2 * NBIN])
    if dtype == F64:
        spec = torch.complex(re, im).reshape(B, T, NBIN).transpose(1, 2)
        return torch.istft(spec, NFFT, hop, NFFT, window.double(), center=True)
    im[:, 0], im[:, NBIN - 1] = 0.0, 0.0
    fre = torch.cat((re, re[:, 1:NBIN - 1].flip(1)), 1)
    fim = torch.cat((im, -im[:, 1:NBIN - 1].flip(1)), 1)
    w = window.to(dtype)
    frames = (fft1024_radix2(fre, fim, tw, inverse=True)[0] * (1.0 / NFFT) * w).reshape(B, T, NFFT)
    n = hop * (T - 1) + NFFT
    acc, env = torch.zeros(B, n, dtype=dtype), torch.zeros(n, dtype=dtype)
    for f in range(T):
        acc[:, f * hop:f * hop + NFFT] += frames[:, f]
        env[f * hop:f * hop + NFFT] += w * w
    return (acc / env)[:, NFFT // 2:NFFT // 2 + hop * (T - 1)]


# ================================================================== sinus_embed, rope_table

SINUS_CASES = tuple((dim, E, scale) for dim in (4, 256, 258) for E in (1, 33) for scale in (1000.0, 1.0))
ROPE_HALF = 32
ROPE_N = (1, 469, 4096)


def sway_grid(steps=32, sway=-1.0):
    t = torch.linspace(0, 1, steps + 1)
    return t + sway * (torch.cos(torch.pi / 2 * t) - 1 + t)


def sinus_inputs(dim, E):
    """t [E] (the 33-point sway grid, which holds 0 and 1, or [1]), freqs [dim / 2] = exp(-k log(1e4) / (dim / 2 - 1))."""
    half = dim // 2
    t = sway_grid() if E == 33 else torch.ones(E)
    return t, torch.exp(torch.arange(half).float() * -(math.log(10000) / (half - 1)))


def sinus_arg(t, freqs, scale):
    """(scale t[e]) freqs[k] in fp32: two roundings, no add, so the same bits wherever it is computed."""
    return (torch.tensor(scale, dtype=F32) * t.float())[:, None] * freqs.float()[None, :]


def sinus_embed(t, freqs, scale, dtype=F64):
    a = sinus_arg(t, freqs, scale).to(dtype)
    return torch.cat((torch.sin(a), torch.cos(a)), -1)


def rope_inv_freq(half=ROPE_HALF):
    return 1.0 / (10000 ** (torch.arange(0, 2 * half, 2).float() / (2 * half)))


def rope_arg(inv_freq, N):
    return torch.arange(N).float()[:, None] * inv_freq.float()[None, :]


def rope_table(inv_freq, N, dtype=F64):
    a = rope_arg(inv_freq, N).to(dtype)
    return torch.stack((torch.cos(a), torch.sin(a)), -1)
