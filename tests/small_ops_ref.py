"""Plain PyTorch restatements of the small kernels (csrc/norm.hip, the non-streaming half of csrc/ppg.hip, csrc/elementwise.hip,
f5e_bigvgan_post), written from the formula in each kernel's header comment, plus the seeded inputs and the case lists that
tests/test_small_ops_cpu.py (pins these restatements to independent torch calls, and checks the inputs) and
tests/test_small_ops_gpu.py (compares the HIP ops with them) share.

Every reference takes the arguments of its ``f5e_tts_amd.ops`` wrapper and returns its result instead of filling ``out``
(``out`` / ``xs`` / ``stats`` ... are accepted and ignored, or give a width).  ``dtype`` is the working precision: float64
for the reference, float32 for the yardstick that the GPU tests scale their gates by.  Nothing here imports f5e_tts_amd."""
import math

import torch

F64 = torch.float64


def g(seed):
    return torch.Generator().manual_seed(seed)


def _at_eval(t, eval_ptr, eval_stride):
    """The [mod_rows, D] view ``t`` moved along by eval * eval_stride floats (the tables hold one block per evaluation)."""
    e = int(eval_ptr) if eval_ptr is not None else 0
    return t if e == 0 else t.as_strided(t.shape, t.stride(), t.storage_offset() + e * eval_stride)


def _mod_row(rows, rows_per_seq, mod_rows):
    return (torch.arange(rows) // rows_per_seq) % mod_rows


# ------------------------------------------------------------------ norm.hip

def layernorm(x, out=None, gamma=None, beta=None, scale=None, shift=None, rows_per_seq=1, eval_ptr=None, eval_stride=0,
              eps=1e-6, dtype=F64):
    """y = (x - mean) / sqrt(biased var + eps) [* gamma + beta] [* (1 + scale[seq]) + shift[seq]], seq = (row / rows_per_seq)
    % mod_rows."""
    v = x.to(dtype)
    mu = v.sum(1, keepdim=True) / v.shape[1]
    c = v - mu
    y = c / torch.sqrt((c * c).sum(1, keepdim=True) / v.shape[1] + eps)
    if gamma is not None:
        y = y * gamma.to(dtype) + beta.to(dtype)
    if scale is not None:
        m = _mod_row(v.shape[0], rows_per_seq, scale.shape[0])
        y = y * (1 + _at_eval(scale, eval_ptr, eval_stride).to(dtype)[m]) + _at_eval(shift, eval_ptr, eval_stride).to(dtype)[m]
    return y


def adaln_pre(x, xs, scale, stats, row_mean=None, rows_per_seq=1, eval_ptr=None, eval_stride=0, dtype=F64):
    """-> (xs = (x - mean)(1 + scale[seq]), stats [rows, parts, 2] = parts equal shares of (0, M2) relative to the exact mean,
    row_mean).  ``stats``: the output tensor (its shape[1] is ``parts``) or ``parts`` itself."""
    parts = stats if isinstance(stats, int) else stats.shape[1]
    v = x.to(dtype)
    mu = v.sum(1) / v.shape[1]
    c = v - mu[:, None]
    m = _mod_row(v.shape[0], rows_per_seq, scale.shape[0])
    st = torch.zeros(v.shape[0], parts, 2, dtype=dtype)
    st[:, :, 1] = ((c * c).sum(1) / parts)[:, None]
    return c * (1 + _at_eval(scale, eval_ptr, eval_stride).to(dtype)[m]), st, mu


def l2norm(x, out=None, g=None, dtype=F64):
    """x / max(||x||, 1e-12) * sqrt(D) * g."""
    v = x.to(dtype)
    n = torch.sqrt((v * v).sum(1, keepdim=True))
    return v * (math.sqrt(v.shape[1]) / torch.clamp(n, min=1e-12)) * g.to(dtype)


# ------------------------------------------------------------------ ppg.hip

def glu(x, out=None, dtype=F64):
    """x [rows, 2C] -> x[:, :C] / (1 + exp(-x[:, C:]))."""
    v = x.to(dtype)
    C = v.shape[1] // 2
    return v[:, :C] / (1 + torch.exp(-v[:, C:]))


def dwconv(x, w_t, bias, out=None, keep=None, dtype=F64):
    """y[b, t, c] = bias[c] + sum_j w_t[j, c] x'[b, t + j - (K - 1) / 2, c] over the taps inside the sequence, x' = x with
    the frames of keep == 0 zeroed BEFORE the convolution."""
    v, w = x.to(dtype), w_t.to(dtype)
    if keep is not None:
        v = v * (keep.reshape(v.shape[0], v.shape[1], 1) != 0).to(dtype)
    B, T, C = v.shape
    K = w.shape[0]
    pad = (K - 1) // 2
    y = bias.to(dtype).expand(B, T, C).clone()
    for j in range(K):
        lo, hi = max(0, pad - j), min(T, T + pad - j)          # output frames t with 0 <= t + j - pad < T
        if lo < hi:
            y[:, lo:hi] += w[j] * v[:, lo + j - pad:hi + j - pad]
    return y


def softmax_rows(x, out, L, scale, kv_len=None, rows_per_seq=1, dtype=F64):
    """mask keys >= len (-inf), softmax of scale * x over the row, zero beyond len: pad columns up to the output width
    (``out``: the output tensor or its width) included.  len = min(kv_len[row / rows_per_seq], L), or L."""
    width = out if isinstance(out, int) else out.shape[1]
    rows = x.shape[0]
    ln = torch.full((rows,), L, dtype=torch.long)
    if kv_len is not None:
        ln = torch.clamp(kv_len.long()[torch.arange(rows) // rows_per_seq], max=L)
    live = torch.arange(L)[None, :] < ln[:, None]
    s = x[:, :L].to(dtype) * scale
    s = torch.where(live, s, torch.full_like(s, -math.inf))
    mx = s.max(1, keepdim=True).values
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))      # a row without keys: every term is exp(-inf) = 0
    e = torch.exp(s - mx)
    den = e.sum(1, keepdim=True)
    p = torch.where(live, e / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(e))
    y = torch.zeros(rows, width, dtype=dtype)
    y[:, :L] = p
    return y


# ------------------------------------------------------------------ elementwise.hip

def axpby(x, y, out=None, a=1.0, b=1.0, c=0.0, dtype=F64):
    r = a * x.to(dtype)
    if y is not None:
        r = r + b * y.to(dtype)
    return r + c


def ode_update(pred, branch_stride, mode, w0, w1, base, dst=None, coef=None, eval_ptr=None, dtype=F64):
    """dst = base + coef[eval] * v;  v = p0 | p0 + (p0 - p1) w0 | w0 (p2 - p1) + w1 (p1 - p0) + p0."""
    n = base.numel()
    p = pred.reshape(-1).to(dtype)
    p0, p1, p2 = p[:n], p[branch_stride:branch_stride + n], p[2 * branch_stride:2 * branch_stride + n]
    v = p0 if mode == 0 else (p0 + (p0 - p1) * w0 if mode == 1 else w0 * (p2 - p1) + w1 * (p1 - p0) + p0)
    h = coef.to(dtype)[int(eval_ptr) if eval_ptr is not None else 0]
    return base.reshape(-1).to(dtype) + h * v


def stitch(cond, y, mask_u8, out=None):
    return torch.where(mask_u8.reshape(-1, 1) != 0, cond.reshape(mask_u8.numel(), -1), y.reshape(mask_u8.numel(), -1))


def text_gather(ids, table, pos, keep, out=None, dtype=F64):
    """out[b, n] = (table[clamp(ids[b, n], 0, rows - 1)] + pos[min(n, max_pos - 1)]) * keep[b, n]."""
    B, N = ids.shape
    v = table.to(dtype)[torch.clamp(ids.long(), 0, table.shape[0] - 1)]
    if pos is not None:
        v = v + pos.to(dtype)[torch.clamp(torch.arange(N), max=pos.shape[0] - 1)][None]
    if keep is not None:
        v = v * keep.to(dtype)[..., None]
    return v


def vq_eval(logits, vars_, combine_groups, out=None, targets=None, stats=None, groups=1, num_vars=1, dtype=F64):
    """-> (targets [rows, G]: FIRST maximal index of every group, q [rows, G vd]: that codebook row per group (group 0's
    block of ``vars_`` for all groups when combine_groups), code perplexity, prob perplexity), both perplexities
    sum_g exp(-sum_v p log(p + 1e-7)) with p = the mean one-hot / the mean softmax over the rows."""
    rows, G, V = logits.shape[0], groups, num_vars
    lg = logits[:, :G * V].reshape(rows, G, V).to(dtype)
    top = lg.max(-1, keepdim=True).values
    tgt = torch.where(lg == top, torch.arange(V).expand(rows, G, V), torch.full((rows, G, V), V)).min(-1).values
    cb = vars_.reshape(1 if combine_groups else G, V, -1)
    q = torch.stack([cb[0 if combine_groups else gi][tgt[:, gi]] for gi in range(G)], 1).reshape(rows, -1)
    hard = torch.zeros(rows, G, V, dtype=dtype).scatter_(-1, tgt[..., None], 1.0).mean(0)
    e = torch.exp(lg - top)
    avg = (e / e.sum(-1, keepdim=True)).mean(0)
    ppl = lambda p: torch.exp(-(p * torch.log(p + 1e-7)).sum(-1)).sum()    # noqa: E731
    return tgt.to(torch.int32), q, ppl(hard), ppl(avg)


# ------------------------------------------------------------------ bigvgan.hip: conv_post

def conv_post(a, w, bias, out=None, use_tanh=False, dtype=F64, pre=False):
    """a [B, L, C], w [ksz, C] -> [B, L] = clamp(sum_k sum_c a[b, t + k - (ksz - 1) / 2, c] w[k, c] + bias, -1, 1) or tanh;
    ``pre``: the value before the clamp / tanh."""
    v, ww = a.to(dtype), w.to(dtype)
    B, L, _ = v.shape
    K = ww.shape[0]
    pad = (K - 1) // 2
    y = torch.zeros(B, L, dtype=dtype)
    for k in range(K):
        lo, hi = max(0, pad - k), min(L, L + pad - k)
        if lo < hi:
            y[:, lo:hi] += (v[:, lo + k - pad:hi + k - pad] * ww[k]).sum(-1)
    if bias is not None:
        y = y + bias.to(dtype)[0]
    return y if pre else (torch.tanh(y) if use_tanh else torch.clamp(y, -1.0, 1.0))


# ================================================================== cases and seeded inputs (shared by both test files)

GRID_CAP_ELEMENTWISE = 2048 * 256          # grid_for of elementwise.hip: work items in one trip of the grid-stride loop
GRID_CAP_PPG = 4096 * 256                  # grid_for of ppg.hip

LN_FIXED_D = (1280, 1536, 1792, 2048)      # layernorm_kernel<5..8>
LN_SMALL_D = (256, 1024)                   # in-place / both-given variants also at instantiations 1 and 4
LN_ANY_D = (4, 64, 100, 252, 260, 516, 1000, 2044)
ADALN_D = (256, 512, 1280, 2048)
L2_D = (256, 768, 1024, 2048)
GLU_CASES = ((1, 4), (5, 64), (77, 256), (4100, 1024))
DWCONV_CASES = tuple((2, T, C, K) for K in (1, 3, 15, 31) for T in (1, 7, 53) for C in (4, 64)) + ((2, 2049, 1024, 15),)
SOFTMAX_L = (1, 63, 64, 65, 200)
AXPBY_N = (1, 255, 257, GRID_CAP_ELEMENTWISE + 77)
BIG_N = GRID_CAP_ELEMENTWISE + 77
STITCH_CASE = (5300, 100)
TEXT_GATHER_CASE = (2, 2100, 512, 64, 30)  # B, N, TD, max_pos, table_rows
VQ_CASES = tuple((V, G, vd, comb) for V in (10, 64, 65, 320) for G in (1, 2) for vd in (8, 100) for comb in (False, True))
POST_CASES = tuple((C, L) for C in (12, 24) for L in (1, 255, 256, 257, 700))
FBANK_CASES = tuple((nw, m) for nw in (400, 559, 560) for m in (23, 80))


def shrunk(case):
    """The CPU twin of a case whose size only exists to pass a grid cap."""
    return {(4100, 1024): (9, 1024), (2, 2049, 1024, 15): (2, 40, 1024, 15), TEXT_GATHER_CASE: (2, 70, 512, 64, 30),
            STITCH_CASE: (53, 100), BIG_N: 1077}.get(case, case)


def ln_inputs(rows, D, seed=0):
    """x, gamma, beta, tab [2 evaluations, 2 modulation rows, 6 D] (scale = tab[e, :, D:2D], shift = tab[e, :, :D])."""
    x = torch.randn(rows, D, generator=g(100 + seed)) * 3 + 1
    return (x, 1 + 0.3 * torch.randn(D, generator=g(101 + seed)), torch.randn(D, generator=g(102 + seed)),
            torch.randn(2, 2, 6 * D, generator=g(103 + seed)) * 0.5)


def l2_inputs(rows, D):
    x = torch.randn(rows, D, generator=g(110)) * 2
    x[3] = 0.0                                                  # ||x|| = 0: the 1e-12 clamp of F.normalize
    return x, 1 + 0.3 * torch.randn(D, generator=g(111))


GLU_SPECIAL = (30.0, -30.0, 100.0, -100.0)


def glu_inputs(rows, C):
    """x [rows, 2C]: gates ~ 4 N(0, 1) clamped to +-20, and at flat positions p % 101 < 4 the saturating gates +30, -30,
    +100, -100 (kind 1..4; 0 elsewhere)."""
    x = torch.randn(rows, 2 * C, generator=g(120))
    x[:, C:] = torch.clamp(4 * x[:, C:], -20.0, 20.0)
    flat = torch.arange(rows * C).reshape(rows, C) % 101
    kind = torch.where(flat < 4, flat + 1, torch.zeros_like(flat))
    for i, val in enumerate(GLU_SPECIAL):
        x[:, C:][kind == i + 1] = val
    return x, kind


def dwconv_keep(B, T):
    """0 / 1 [B, T] over frames that all hold non-zero data: dead where (t + b) % 3 == 1, live where (t + b) % 3 == 2, and
    the remaining third live in the head t < len_b and dead in the ragged tail (len = max(T - T/4 - 1, 1), T/2)."""
    t, b = torch.arange(T)[None, :], torch.arange(B)[:, None]
    ln = torch.tensor([max(T - T // 4 - 1, 1), T // 2] * B)[:B, None]
    ph = (t + b) % 3
    return ((ph == 2) | ((ph == 0) & (t < ln))).float()


def dwconv_inputs(B, T, C, K):
    x = torch.randn(B, T, C, generator=g(130)) + 0.5             # the masked frames are NOT zero: an ignored mask shows
    return (x, torch.randn(K, C, generator=g(131)) / math.sqrt(K), torch.randn(C, generator=g(132)), dwconv_keep(B, T))


SOFTMAX_ROWS, SOFTMAX_RPS, SOFTMAX_SCALE, SENTINEL = 7, 2, 0.7, 77.0


def softmax_inputs(L, big=False):
    """buf [7, ld] (ld = roundup4(L) + 4, pad columns = SENTINEL), kv_len [4] = 0, 3, L, L + 9, scale.  |scale x| <= 4.9, so
    every exponent argument is within 9.8; ``big``: scale x in +-1e4."""
    ld = (L + 3) // 4 * 4 + 4
    buf = torch.full((SOFTMAX_ROWS, ld), SENTINEL)
    if big:
        buf[:, :L] = torch.clamp(3000 * torch.randn(SOFTMAX_ROWS, L, generator=g(140)), -1e4, 1e4)
        return buf, torch.tensor([0, 3, L, L + 9], dtype=torch.int32), 1.0
    buf[:, :L] = torch.clamp(2 * torch.randn(SOFTMAX_ROWS, L, generator=g(141)), -7.0, 7.0)
    return buf, torch.tensor([0, 3, L, L + 9], dtype=torch.int32), SOFTMAX_SCALE


VQ_ROWS, VQ_LD_PAD, VQ_TOP = 7, 12, 9.0


def vq_inputs(V, G, vd, combine):
    """logits [7, G V + 12] (pad columns hold +50: a kernel that reads them wins the argmax with them), vars, and the
    hand-built tie rows {(row, group): (maximal indices, expected target)}; every other logit is <= 5 < VQ_TOP."""
    logits = torch.full((VQ_ROWS, G * V + VQ_LD_PAD), 50.0)
    logits[:, :G * V] = torch.clamp(torch.randn(VQ_ROWS, G * V, generator=g(150)), max=5.0)
    ties = {}
    plans = [((5, 6), 5), (tuple(range(V)), 0)]                  # {5, 6} -> 5; a constant row -> 0
    if V > 134:
        # one lane's three trips; one lane's second and third trip; the smaller index in the HIGHER lane
        plans += [((3, 67, 131), 3), ((70, 134), 70), ((70, 133), 70)]
    for r, (idx, want) in enumerate(plans):
        gi = (r + 1) % G                                         # both groups get tie rows when G = 2
        logits[r, gi * V + torch.tensor(idx)] = VQ_TOP
        ties[(r, gi)] = (idx, want)
    vars_ = torch.randn((1 if combine else G) * V, vd, generator=g(151))
    return logits, vars_, ties


def text_gather_inputs(B, N, TD, max_pos, table_rows):
    ids = torch.randint(0, table_rows, (B, N), generator=g(160), dtype=torch.int32)
    ids[0, 1], ids[1, N - 1], ids[0, N // 2], ids[1, 0] = -1, table_rows, table_rows + 5, -7
    return (ids, torch.randn(table_rows, TD, generator=g(161)), torch.randn(max_pos, TD, generator=g(162)),
            (torch.rand(B, N, generator=g(163)) > 0.2).float())


POST_B, POST_K = 2, 7


def post_inputs(C, L):
    """a [2, L, C] with a per-frame ramp 0.02 .. 1, so the pre-activations run from well inside (-1, 1) to well past it."""
    a = torch.randn(POST_B, L, C, generator=g(170)) * torch.linspace(0.02, 1.0, L)[None, :, None]
    return a, 0.5 * torch.randn(POST_K, C, generator=g(171)), torch.tensor([0.1])


def cast_inputs(n):
    """fp32 values whose bf16 rounding is decided by the rule, not the data: exact ties (low half 0x8000) above an even and
    an odd bf16 mantissa, the largest finite fp32 (rounds to inf), +-inf, quiet and signalling NaNs (one whose high half
    alone reads as inf), +-0 and denormals, followed by seeded normal data."""
    bits = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0xFF7FFFFF,
            0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC00123, 0x00000000, 0x80000000,
            0x00000001, 0x00008000, 0x00018000, 0x0000FFFF, 0x007FFFFF, 0x807FFFFF, 0x80008000, 0x00800000]
    sp = torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)
    x = torch.randn(n, generator=g(180)) * 10
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    x[n - k:] = sp[:k].flip(0)                                  # and in the last trip of the grid-stride loop
    return x


def fbank_inputs(nw):
    """wav [3, nw]: noise with a DC offset, silence, a full-scale +-1 square wave (half period 37 samples) plus DC."""
    wav = torch.zeros(3, nw)
    wav[0] = 0.05 * torch.randn(nw, generator=g(190)) + 0.02
    wav[2] = torch.where((torch.arange(nw) // 37) % 2 == 0, 1.0, -1.0) + 0.25
    return wav
