"""fp64 restatements of the fp32 GEMM (csrc/gemm_f32.hip), GRN (csrc/norm.hip), dwconv7 and im2col (csrc/conv.hip), written
from the formulas in the kernels' header comments, plus the seeded inputs, the case lists and a plain-Python restatement of
the GEMM's host dispatch.  tests/test_fp32_ops_cpu.py pins the restatements to independent torch calls and checks the
preconditions the GPU cases rely on; tests/test_fp32_ops_gpu.py compares the HIP ops with them.  Nothing here imports
f5e_tts_amd.

GEMM inputs are small integers (A, W in [-8, 8], bias in [-16, 16], addend in [-64, 64], ch_scale a power of two in
[1/4, 4], row_scale in {0, 1, 2}), all stored as fp32: with K <= 2048 every product, every partial sum in any order and
every epilogue step is exactly representable, so the kernel has to equal the reference bit for bit."""
import functools
import math
from collections import namedtuple

import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
SENTINEL = 77.0                             # exactly representable in bf16 too
ACT_NONE, ACT_SILU, ACT_GELU_ERF, ACT_GELU_TANH, ACT_RELU, ACT_MISH = range(6)    # f5e_tts_amd._C (checked on the CPU)


def g(seed):
    return torch.Generator().manual_seed(seed)


# ================================================================== activations (f5e_common.h, the same formulas)

def act_exp_arg(v, act):
    """The argument of the activation's one exponential (0 where it has none): what ``__expf`` / ``v_exp_f32`` round."""
    v = v.to(F64)
    if act == ACT_SILU:
        return -v
    if act == ACT_GELU_TANH:
        return -2.0 * math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)
    if act == ACT_MISH:
        return torch.clamp(v, max=20.0)
    return torch.zeros_like(v)


def apply_act(v, act):
    """silu x / (1 + e^-x); gelu 0.5 x (1 + erf(x / sqrt 2)); tanh-gelu x / (1 + e^-2u), u = sqrt(2 / pi)(x + 0.044715 x^3)
    (= 0.5 x (1 + tanh u)); relu; mish x n / (n + 2), n = e (e + 2), e = exp(min(x, 20)), x itself past 20.  In v's dtype."""
    if act == ACT_NONE:
        return v
    if act == ACT_RELU:
        return torch.clamp(v, min=0.0)
    if act == ACT_SILU:
        return v / (1 + torch.exp(-v))
    if act == ACT_GELU_ERF:
        return 0.5 * v * (1 + torch.erf(v * 0.7071067811865476))
    if act == ACT_GELU_TANH:
        c = 2.0 * math.sqrt(2.0 / math.pi)
        return v / (1 + torch.exp(-(c * (v + 0.044715 * v * v * v))))
    if act == ACT_MISH:
        e = torch.exp(torch.clamp(v, max=20.0))
        n = e * (e + 2)
        return torch.where(v > 20.0, v, v * (n / (n + 2)))
    raise ValueError(act)


# ================================================================== gemm_f32: cases

_DEFAULTS = dict(a_rows=0,                  # 0: M rows
                 a_act=ACT_NONE, act=ACT_NONE, bias=True, cs=False, add_rows=0,   # add_rows 0: no addend
                 inplace=False,             # the addend IS the out view (add_rows = M)
                 rs=False, outs="f32",      # "f32" | "bf16" | "both"
                 a_off=0, w_off=0,          # column offset of the A / W view inside its buffer (elements)
                 out_off=0, out_pad=0,      # out = buf[:, off:off + N] of a buffer that is N + pad wide (ldo = N + pad)
                 bf_off=0, bf_pad=0, add_off=0, add_pad=0, bias_off=0, cs_off=0,
                 randn=False)               # seeded normal inputs instead of integers (the a_act cases)
Case = namedtuple("Case", ("M", "N", "K") + tuple(_DEFAULTS), defaults=tuple(_DEFAULTS.values()))
A_PAD, W_PAD = 4, 8                         # lda = K + 4, ldw = K + 8: the leading dimensions are never the widths


def cid(c):
    """A readable pytest id: M x N x K and every field that is not at its default."""
    extra = [f"{k}={getattr(c, k)}" for k, v in _DEFAULTS.items() if getattr(c, k) != v]
    return f"{c.M}x{c.N}x{c.K}" + ("," + ",".join(extra) if extra else "")


FULL = dict(bias=True, cs=True, add_rows=3, rs=True, outs="both")     # the whole epilogue on one case

# Ring and tail of gemm_f32_dma_kernel<32, 64, 2, 2, 4> (NSTAGE 4): KT = 1, 1, 1, 2, 2, 3, 4, 4, 5, 6, 9; the last two K's of
# the tuple complete the (ring state x ragged) grid: KT = NSTAGE - 1 with a ragged tail and KT > NSTAGE without one
RING32_K = (4, 60, 64, 68, 128, 192, 196, 256, 260, 324, 516, 132, 320)
RING32 = tuple(Case(33, 68, K, **FULL) for K in RING32_K)
# the same ring states under the scalar epilogue (N % 4 != 0; the leading dimensions stay multiples of 4)
RING32_SCALAR = tuple(Case(33, 67, K, out_pad=1, bf_pad=1, add_pad=1, **FULL) for K in (64, 68, 192, 132, 256, 196, 320, 260))
# gemm_f32_dma_kernel<64, 64, 2, 2, 3> (NSTAGE 3; tile product >= 128): one row in the last M tile | a partial last quad tile
# on the vector path | N % 4 != 0.  KT = 1, 1, 2, 2, 3, 3, 4, 5, 7, and K = 256: KT > NSTAGE without a ragged tail
RING64_SHAPES = ((449, 1024), (512, 964), (450, 961))
RING64_K = (4, 64, 68, 128, 132, 192, 196, 260, 388, 256)
RING64 = tuple(Case(M, N, K, **FULL) for (M, N) in RING64_SHAPES for K in RING64_K) + \
    (Case(448, 1152, 132, **FULL),)         # 7 x 18 = 126 tiles: just below the 128-tile rule, the 32-row kernel
# the plain kernel through a base that is 4 bytes past a 16-byte boundary (lda, ldw stay multiples of 4)
MISALIGNED_K = (4, 12, 16, 20, 32, 36, 100)
MISALIGNED = tuple(Case(65, 65, K, out_pad=3, bf_pad=3, add_pad=3, **FULL, **{which: 1})
                   for which in ("a_off", "w_off") for K in MISALIGNED_K)
EDGES = tuple(Case(M, 68, 68, **FULL) for M in (1, 31, 32, 33, 63, 64, 65)) + \
    tuple(Case(33, N, 68, **FULL) for N in (1, 3, 4, 5, 60, 63, 64, 65, 68))

# Epilogue forms (M 33, K 68): name -> (case with everything on, the one vec condition it breaks or None)
_FORM = dict(M=33, N=68, K=68, **FULL)
FORMS = {
    "sliced_aligned": (Case(**{**_FORM, "out_off": 4, "out_pad": 8, "bf_off": 4, "bf_pad": 8, "add_off": 4, "add_pad": 8}), None),
    "n67": (Case(**{**_FORM, "N": 67, "out_pad": 1, "bf_pad": 1, "add_pad": 1}), "N"),
    "ldo": (Case(**{**_FORM, "out_pad": 2}), "ldo"),
    "out_base": (Case(**{**_FORM, "out_off": 1, "out_pad": 4}), "out"),
    "bf_base": (Case(**{**_FORM, "bf_off": 1, "bf_pad": 4}), "out_bf16"),
    "ldo_bf16": (Case(**{**_FORM, "bf_pad": 2}), "ldo_bf16"),
    "bias_base": (Case(**{**_FORM, "bias_off": 1}), "bias"),
    "cs_base": (Case(**{**_FORM, "cs_off": 1}), "ch_scale"),
    "add_base": (Case(**{**_FORM, "add_off": 1, "add_pad": 4}), "addend"),
    "ld_add": (Case(**{**_FORM, "add_pad": 2}), "ld_add"),
}


def form_variants(c):
    """The form with out only / out_bf16 only / both, times with and without each of bias, ch_scale, addend, row_scale."""
    return tuple(c._replace(outs=o, bias=b, cs=s, add_rows=a, rs=r) for o in ("f32", "bf16", "both")
                 for b in (False, True) for s in (False, True) for a in (0, c.add_rows) for r in (False, True))


_SCALAR = dict(N=67, out_pad=1, bf_pad=1, add_pad=1)
WRAPS = tuple(Case(**{**_FORM, "a_rows": 13, "add_rows": ar, **ep}) for ar in (1, 3, 33) for ep in ({}, _SCALAR))
INPLACE = tuple(Case(**{**_FORM, "M": M, "add_rows": 0, "inplace": True, "outs": "f32", "out_pad": 8 if N == 68 else 1, "N": N})
                for M in (33, 65) for N in (68, 67))

EXACT_ACTS = (ACT_NONE, ACT_RELU)
INEXACT_ACTS = (ACT_SILU, ACT_GELU_ERF, ACT_GELU_TANH, ACT_MISH)
# one case per kernel: 32-row DMA | 64-row DMA | plain (misaligned A).  No addend: every step after the activation is a
# multiplication, so the relative allowance for the exponential carries through to the result
_ACT_EP = dict(bias=True, cs=True, rs=True, outs="both")
ACT_SHAPES = (Case(33, 68, 196, **_ACT_EP), Case(450, 1024, 132, **_ACT_EP),
              Case(65, 65, 100, a_off=1, out_pad=3, bf_pad=3, **_ACT_EP))
ACT_CASES = tuple(c._replace(act=a) for c in ACT_SHAPES for a in INEXACT_ACTS)
# a_act = SILU: the plain kernel on aligned operands, randn inputs.  K 64: four whole 16-wide steps; 100: ragged; 260
A_ACT_SHAPES = ((33, 68, 100), (65, 65, 64), (130, 100, 260))
A_ACT_CASES = tuple(Case(M, N, K, a_act=ACT_SILU, act=a, randn=True, bias=True, outs="f32")
                    for (M, N, K) in A_ACT_SHAPES for a in (ACT_NONE, ACT_GELU_ERF))

EXACT_CASES = RING32 + RING32_SCALAR + RING64 + MISALIGNED + EDGES + WRAPS + INPLACE + \
    tuple(v for c, _ in FORMS.values() for v in form_variants(c))
ALL_GEMM_CASES = EXACT_CASES + ACT_CASES + A_ACT_CASES


# ================================================================== gemm_f32: the host dispatch, restated

NSTAGE = {"plain": 2, "dma32": 4, "dma64": 3}      # LDS buffers of gemm_f32_kernel; ring slots of the two DMA instantiations
VEC_CONDITIONS = ("N", "ldo", "ldo_bf16", "ld_add", "bias", "ch_scale", "addend", "out", "out_bf16")


def vec_broken(N, byte_offsets, lds):
    """The conditions of the vector epilogue that fail (csrc/gemm_f32.hip, f5e_gemm_f32, lines 339-340: ``a.vec = ...``).
    byte_offsets: address % 16 of bias, ch_scale, addend, out and address % 8 of out_bf16 (0 for an absent operand, like the
    null pointer); lds: ldo, ldo_bf16, ld_add (0 when absent)."""
    bad = set()
    if N % 4 or N < 4:
        bad.add("N")
    bad |= {k for k in ("ldo", "ldo_bf16", "ld_add") if lds[k] % 4}
    bad |= {k for k in ("bias", "ch_scale", "addend", "out") if byte_offsets[k] % 16}
    if byte_offsets["out_bf16"] % 8:
        bad.add("out_bf16")
    return bad


def gemm_f32_path(M, N, K, a_act, byte_offsets, lds):
    """-> (kernel, vec, KT, ragged), mirroring f5e_gemm_f32 in csrc/gemm_f32.hip: ``a.vec`` as computed there (lines
    339-340); the LDS-DMA kernels only ``if (a_act == F5E_ACT_NONE && (((uintptr_t)A | (uintptr_t)W) & 15) == 0)`` (line
    341), the 32-row one when ``((M + 63) / 64) * ((N + 63) / 64) < 128`` (line 343), else the 64-row one (line 344);
    otherwise ``gemm_f32_kernel`` (lines 346-348), which has the scalar epilogue only.  KT: K steps of 64 (``launch_dma``,
    line 309: ``kt = (a.K + 63) / 64``) or of 16 (``gemm_f32_kernel``, line 63: ``KT = (a.K + BK - 1) / BK``); ragged: the
    last step is partial.  byte_offsets also holds address % 16 of A and W."""
    vec = not vec_broken(N, byte_offsets, lds)
    if a_act == ACT_NONE and byte_offsets["A"] % 16 == 0 and byte_offsets["W"] % 16 == 0:
        kern = "dma32" if ((M + 63) // 64) * ((N + 63) // 64) < 128 else "dma64"
        return kern, vec, (K + 63) // 64, K % 64 != 0
    return "plain", False, (K + 15) // 16, K % 16 != 0


def ring_state(kernel, KT):
    n = NSTAGE[kernel]
    return "<NSTAGE-1" if KT < n - 1 else "=NSTAGE-1" if KT == n - 1 else "=NSTAGE" if KT == n else ">NSTAGE"


def case_layout(c):
    """(byte_offsets, lds) that the case claims, every buffer starting on a 16-byte boundary."""
    has_f32, has_bf, has_add = c.outs in ("f32", "both"), c.outs in ("bf16", "both"), c.add_rows > 0 or c.inplace
    add_off, add_ld = (c.out_off, c.N + c.out_pad) if c.inplace else (c.add_off, c.N + c.add_pad)
    off = dict(A=4 * c.a_off % 16, W=4 * c.w_off % 16, bias=4 * c.bias_off % 16 if c.bias else 0,
               ch_scale=4 * c.cs_off % 16 if c.cs else 0, addend=4 * add_off % 16 if has_add else 0,
               out=4 * c.out_off % 16 if has_f32 else 0, out_bf16=2 * c.bf_off % 8 if has_bf else 0)
    lds = dict(ldo=c.N + c.out_pad if has_f32 else 0, ldo_bf16=c.N + c.bf_pad if has_bf else 0, ld_add=add_ld if has_add else 0)
    return off, lds


def case_path(c):
    off, lds = case_layout(c)
    return gemm_f32_path(c.M, c.N, c.K, c.a_act, off, lds)


# ================================================================== gemm_f32: inputs and reference

def placed(t, off, ld, extra_rows=2, fill=SENTINEL):
    """t [rows, cols] as the as_strided((rows, cols), (ld, 1), off) view of a flat sentinel-filled buffer of rows + 2 rows of
    ld elements -> (flat, spec); ``view(flat, spec)`` gives the view on any copy of the buffer."""
    rows, cols = t.shape
    assert off + cols <= ld
    flat = torch.full(((rows + extra_rows) * ld,), fill, dtype=t.dtype)
    spec = ((rows, cols), (ld, 1), off)
    flat.as_strided(*spec).copy_(t)
    return flat, spec


def view(flat, spec):
    return flat.as_strided(*spec)


@functools.lru_cache(maxsize=8)
def gemm_inputs(M, N, K, a_rows, add_rows, randn):
    """Seeded operands (CPU, fp32) and the pre-activation Z = A[m % a_rows] W^T in fp64 (exact for the integer inputs)."""
    a_rows = a_rows or M
    s = 7000 + 131 * M + 17 * N + K
    if randn:
        A, W = torch.randn(a_rows, K, generator=g(s)), torch.randn(N, K, generator=g(s + 1)) / math.sqrt(K)
        bias, add = torch.randn(N, generator=g(s + 2)), torch.randn(max(add_rows, 1), N, generator=g(s + 3))
    else:
        ri = lambda lo, hi, shape, k: torch.randint(lo, hi + 1, shape, generator=g(s + k)).float()    # noqa: E731
        A, W, bias, add = ri(-8, 8, (a_rows, K), 0), ri(-8, 8, (N, K), 1), ri(-16, 16, (N,), 2), ri(-64, 64, (max(add_rows, 1), N), 3)
    cs = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0])[torch.randint(0, 5, (N,), generator=g(s + 4))]
    rs = torch.randint(0, 3, (M,), generator=g(s + 5)).float()
    rs[M // 2] = 0.0 if M > 2 else 2.0                          # at least one zero row (but never the only row)
    return dict(A=A, W=W, bias=bias, cs=cs, add=add, rs=rs)


@functools.lru_cache(maxsize=8)
def gemm_z(M, N, K, a_rows, randn, a_act):
    t = gemm_inputs(M, N, K, a_rows, 0, randn)
    Aa = apply_act(t["A"].double(), a_act)[torch.arange(M) % (a_rows or M)]
    return Aa @ t["W"].double().T


def act_scale(c):
    """2^-s with |Z + bias| 2^-s <= 20 for the case's integer inputs: W and bias are multiplied by it (exactly)."""
    t = gemm_inputs(c.M, c.N, c.K, c.a_rows, max(c.add_rows, 0), c.randn)
    top = float((gemm_z(c.M, c.N, c.K, c.a_rows, c.randn, c.a_act) + t["bias"].double()).abs().max())
    return 2.0 ** -max(0, math.ceil(math.log2(max(top, 1.0) / 20.0)))


def gemm_operands(c):
    """The case's operand values (CPU, fp32): A, W, bias, cs, add, rs, or None where the case has none.  The inexact
    activation cases scale W and bias by a power of two so that the activation's argument stays within +-20."""
    add_rows = c.M if c.inplace else c.add_rows
    t = dict(gemm_inputs(c.M, c.N, c.K, c.a_rows, add_rows, c.randn))
    if c.act in INEXACT_ACTS and not c.randn:
        sc = act_scale(c)
        t["W"], t["bias"] = t["W"] * sc, t["bias"] * sc
    if not c.bias:
        t["bias"] = None
    if not c.cs:
        t["cs"] = None
    if not add_rows:
        t["add"] = None
    if not c.rs:
        t["rs"] = None
    return t


def gemm_pre(c, t):
    """Z + bias in fp64: the activation's argument."""
    z = gemm_z(c.M, c.N, c.K, c.a_rows, c.randn, c.a_act)
    if c.act in INEXACT_ACTS and not c.randn:
        z = z * act_scale(c)
    return z if t["bias"] is None else z + t["bias"].double()


def gemm_ref(c, t=None, dtype=F64):
    """C = epi(actA(A[m % a_rows]) W^T), epi(v) = ((act(v + bias)) * ch_scale + addend[m % add_rows]) * row_scale[m].
    dtype float32: the same epilogue evaluated in fp32 on the (exact) fp32 argument: the yardstick of the gated cases."""
    t = gemm_operands(c) if t is None else t
    v = apply_act(gemm_pre(c, t).to(dtype), c.act)
    if t["cs"] is not None:
        v = v * t["cs"].to(dtype)
    if t["add"] is not None:
        v = v + t["add"].to(dtype)[torch.arange(c.M) % t["add"].shape[0]]
    if t["rs"] is not None:
        v = v * t["rs"].to(dtype)[:, None]
    return v


def gemm_abs_bound(c, t=None):
    """|actA(A)| |W|^T + |bias| in fp64: what the standard summation bound scales with."""
    t = gemm_operands(c) if t is None else t
    Aa = apply_act(t["A"].double(), c.a_act).abs()[torch.arange(c.M) % t["A"].shape[0]]
    b = Aa @ t["W"].double().abs().T
    return b if t["bias"] is None else b + t["bias"].double().abs()


def exact_magnitude_bound(K):
    """The largest epilogue value in units of 1/4 (ch_scale's granularity): ((64 K + 16) 4 + 64) 2, times 4."""
    return ((64 * K + 16) * 4 + 64) * 2 * 4


# ================================================================== GRN, dwconv7, im2col

def grn(x, gamma, beta, dtype=F64, want_gx=False):
    """gx[b, c] = sqrt(sum_t x[b, t, c]^2); y = gamma (x gx / (mean_c gx + 1e-6)) + beta + x   (modules.py:231-234)."""
    v = x.to(dtype)
    gx = torch.sqrt((v * v).sum(1, keepdim=True))
    y = gamma.to(dtype) * (v * (gx / (gx.sum(2, keepdim=True) / v.shape[2] + 1e-6))) + beta.to(dtype) + v
    return (y, gx[:, 0]) if want_gx else y


GRN_T = (1, 15, 16, 17, 112, 113, 128, 129, 241)
# (B, T, C, kind): "" plain; "x1" x one float past a 16-byte boundary; "g1" gamma likewise; "zero" batch row 1 all zero
GRN_CASES = tuple((2, T, 68, "") for T in GRN_T) + ((2, 17, 4, ""), (2, 33, 68, "x1"), (2, 33, 68, "g1"),
                                                     (1, 1100, 1024, ""), (1, 4100, 66, ""), (3, 17, 68, "zero"), (3, 17, 66, "zero"))
GRN_APPLY_CAP = 1024 * 256                  # f5e_grn: grid of grn_apply_kernel capped at 1024 workgroups of 256 items


def grn_shrunk(case):
    """The CPU twin of a case whose size only exists to pass the grid cap."""
    return {(1, 1100, 1024, ""): (1, 9, 1024, ""), (1, 4100, 66, ""): (1, 41, 66, "")}.get(case, case)


def grn_path(B, T, C, kind):
    """-> (vec, trips of grn_apply_kernel's grid-stride loop), mirroring f5e_grn (csrc/norm.hip)."""
    vec = C % 4 == 0 and kind not in ("x1", "g1")
    items = T * C // 4 if vec else T * C
    return vec, -(-items // GRN_APPLY_CAP)


def grn_inputs(B, T, C, kind=""):
    x = torch.randn(B, T, C, generator=g(300)) * 2
    if kind == "zero":
        x[1] = 0.0
    return x, torch.randn(C, generator=g(301)), torch.randn(C, generator=g(302))


def dwconv7(x, w_t, bias, dtype=F64):
    """y[b, t, c] = bias[c] + sum_{j < 7} w_t[j, c] x[b, t + j - 3, c] over the taps inside [0, T)."""
    v, w = x.to(dtype), w_t.to(dtype)
    B, T, C = v.shape
    y = bias.to(dtype).expand(B, T, C).clone()
    for j in range(7):
        lo, hi = max(0, 3 - j), min(T, T + 3 - j)
        if lo < hi:
            y[:, lo:hi] += w[j] * v[:, lo + j - 3:hi + j - 3]
    return y


DWCONV7_CASES = tuple((3, T, C) for T in (1, 2, 3, 4, 7, 50) for C in (4, 512)) + ((2, 2100, 1024),)
CONV_GRID_CAP = 4096 * 256                  # grid_for of conv.hip


def dwconv7_inputs(B, T, C):
    """Integer-valued, so the result is exact in fp32 in any order (|y| <= 16 + 7 * 8 * 8); no frame is zero."""
    ri = lambda lo, hi, shape, k: torch.randint(lo, hi + 1, shape, generator=g(310 + k)).float()    # noqa: E731
    x = ri(1, 8, (B, T, C), 0) * (2 * ri(0, 1, (B, T, C), 1) - 1)
    return x, ri(-8, 8, (7, C), 2), ri(-16, 16, (C,), 3)


def im2col(x, ksize, pad):
    """col[b, t, j, ic] = x[b, t + j - pad, ic], or 0 outside [0, T)  -> [B, T, ksize * Cin]."""
    B, T, Cin = x.shape
    col = torch.zeros(B, T, ksize, Cin, dtype=x.dtype)
    for j in range(ksize):
        lo, hi = max(0, pad - j), min(T, T + pad - j)
        if lo < hi:
            col[:, lo:hi, j] = x[:, lo + j - pad:hi + j - pad]
    return col.reshape(B, T, ksize * Cin)


IM2COL_K, IM2COL_T, IM2COL_CIN, IM2COL_B = (1, 2, 7, 31), (1, 5, 50), (1, 3, 100), 2
IM2COL_BIG = (2, 750, 100, 7, 3)            # B, T, Cin, ksize, pad: 1 050 000 elements, past one trip of 4096 x 256


def im2col_pads(ksize, T):
    return sorted({0, (ksize - 1) // 2, ksize - 1, T + 2})


def im2col_inputs(B, T, Cin):
    """Non-zero integers: a zero in col is always a padding zero."""
    x = torch.randint(1, 100, (B, T, Cin), generator=g(320)).float()
    return x * (2 * torch.randint(0, 2, (B, T, Cin), generator=g(321)).float() - 1)
