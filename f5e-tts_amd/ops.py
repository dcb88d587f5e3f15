"""Torch-tensor front for the C ABI: pointer extraction, shape inference and loud validation.  PyTorch here only owns
device memory and the stream; every computation happens in libf5e_hip.so."""
from __future__ import annotations

import ctypes as C
import threading
from typing import Optional

import torch

from . import _C
from ._C import ACT_GELU_ERF, ACT_GELU_TANH, ACT_MISH, ACT_NONE, ACT_RELU, ACT_SILU, check, lib  # noqa: F401

Tensor = torch.Tensor
_checked_device = False


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def require_device() -> None:
    """Raise unless a gfx950 device is current and the library is loadable."""
    global _checked_device
    if not _checked_device:
        if not torch.cuda.is_available():
            raise _C.F5EError("f5e_tts_amd needs a ROCm GPU (gfx950); torch.cuda.is_available() is False and there "
                              "is no CPU fallback")
        check(lib().f5e_check_device(), "f5e_check_device")
        _checked_device = True


def _p(t: Optional[Tensor], dtype=None, name="tensor"):
    if t is None:
        return None
    if not t.is_cuda:
        raise _C.F5EError(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise _C.F5EError(f"{name} must be {dtype} (got {t.dtype})")
    if not t.is_contiguous():
        raise _C.F5EError(f"{name} must be contiguous")
    return C.c_void_p(t.data_ptr())


BF, F32, I32, U8 = torch.bfloat16, torch.float32, torch.int32, torch.uint8
F16 = torch.float16
# the 16-bit weight types of the _w16 ops and their F5E_W_* codes
W16_TYPES = {F16: _C.W_FP16, BF: _C.W_BF16}


def _rows(t: Tensor, dtypes, name: str, cols: int, vec: int = 4, whole_rows: bool = False):
    """(pointer, row stride) of a 2-D row-strided view: unit column stride, any row stride >= cols.  ``vec`` = elements per
    vector access of the kernel (4: 16-byte fp32 / 8-byte bf16 accesses -> the base address must be aligned to them and the
    row stride a multiple of 4; 1: scalar accesses).  ``whole_rows``: the kernel touches all of the last row's stride, not
    only its first ``cols`` elements.  Everything is refused here, before any launch."""
    if not t.is_cuda:
        raise _C.F5EError(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
    if t.dtype not in dtypes:
        raise _C.F5EError(f"{name} must be {' or '.join(str(d) for d in dtypes)} (got {t.dtype})")
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < cols or (t.stride(1) != 1 and t.shape[1] > 1):
        raise _C.F5EError(f"{name} must be a [rows, >= {cols}] view with unit column stride (got shape {tuple(t.shape)}, "
                          f"strides {tuple(t.stride())})")
    rows = t.shape[0]
    ld = t.stride(0) if rows > 1 else max(t.stride(0), t.shape[1])     # the stride of a size-1 dimension is arbitrary
    if ld < cols or ld % vec:
        raise _C.F5EError(f"{name}: row stride {ld} must be >= {cols}" + (f" and a multiple of {vec}" if vec > 1 else ""))
    if t.data_ptr() % (vec * t.element_size()):
        raise _C.F5EError(f"{name}: base address must be {vec * t.element_size()}-byte aligned")
    have = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
    need = rows * ld if whole_rows else (rows - 1) * ld + cols
    if have < need:
        raise _C.F5EError(f"{name}: {rows} rows of stride {ld} need {need} elements, the storage holds {have}")
    return C.c_void_p(t.data_ptr()), ld


def _err(msg: str):
    raise _C.F5EError(msg)


def _flat(t: Optional[Tensor], dtype, name: str, n: int):
    """Pointer of a contiguous ``dtype`` GPU tensor that holds at least ``n`` elements (None stays None)."""
    if t is not None and (t.dtype != dtype or t.numel() < n):
        _err(f"{name} must be {dtype} with at least {n} elements (got {t.dtype}, {t.numel()})")
    return _p(t, dtype, name)


def _table(t: Tensor, name: str, cols: int):
    """(pointer, row stride, rows) of an f32 [rows, >= cols] modulation-table view (gate, scale, c, d): unit column stride,
    16-byte aligned rows."""
    if t.ndim != 2 or t.dtype != F32 or t.shape[0] < 1 or t.shape[1] < cols or (t.stride(1) != 1 and t.shape[1] > 1):
        _err(f"{name} must be an f32 [rows, >= {cols}] view with unit column stride (got {t.dtype}, shape {tuple(t.shape)}, "
             f"strides {tuple(t.stride())})")
    if not t.is_cuda:
        _err(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
    ld = t.stride(0) if t.shape[0] > 1 or t.stride(0) % 4 == 0 else (t.shape[1] + 3) // 4 * 4
    if ld % 4 or t.data_ptr() % 16:
        _err(f"{name}: row stride {ld} must be a multiple of 4 and the base 16-byte aligned")
    return C.c_void_p(t.data_ptr()), ld, t.shape[0]


LN_PARTS = (4, 8, 12, 16)


def ln_consumer(stats: Tensor, c: Tensor, d: Tensor, rows_per_seq: int, row_mean: Tensor, eval_ptr: Optional[Tensor] = None,
                cd_eval_stride: int = 0, eps: float = 1e-6) -> "_C.LnFuse":
    """Consumer side of the fused AdaLN (see f5e_ln_fuse): stats f32 [>= M, parts, 2] (tile means relative to row_mean),
    parts = K / 64 in {4, 8, 12, 16}; c, d f32 [1, >= N] views; row_mean f32 [>= M]: the rows' centring offsets, moved along
    by this launch.  The GEMM wrapper checks M, N and K against these."""
    if stats.ndim != 3 or stats.shape[2] != 2 or stats.dtype != F32 or stats.shape[1] not in LN_PARTS:
        _err(f"ln_consumer: stats must be f32 [rows, parts, 2] with parts in {LN_PARTS} (got {stats.dtype}, shape {tuple(stats.shape)})")
    if row_mean.dtype != F32 or row_mean.ndim != 1:
        _err(f"ln_consumer: row_mean must be f32 [rows] (got {row_mean.dtype}, shape {tuple(row_mean.shape)})")
    if c.ndim != 2 or d.ndim != 2 or c.stride(0) != d.stride(0) or c.shape != d.shape:
        _err("ln_consumer: c and d tables must be 2-D and share shape and row stride")
    if eval_ptr is not None and cd_eval_stride <= 0:
        _err("ln_consumer: eval_ptr needs cd_eval_stride")
    f = _C.LnFuse()
    f.stats, f.parts = _p(stats, F32, "stats").value, stats.shape[1]
    f.c, f.cd_stride, f.cd_rows = _table(c, "ln_consumer: c", 1)
    f.d = _table(d, "ln_consumer: d", 1)[0]
    f.cd_eval_stride, f.rows_per_seq, f.eps = cd_eval_stride, rows_per_seq, eps
    f.eval_ptr = _p(eval_ptr, I32, "eval_ptr").value if eval_ptr is not None else None
    f.row_mean = _p(row_mean, F32, "row_mean").value
    f._keep = (stats, c, d, eval_ptr, row_mean)
    return f


def ln_producer(xs_out: Tensor, next_scale: Tensor, stats_out: Tensor, row_mean: Tensor) -> "_C.LnFuse":
    """Producer side: xs_out bf16 [>= M, >= N] row-strided view; next_scale f32 [gate_rows, >= N] view with the gate's row
    stride; stats_out f32 [>= M, N // 64, 2]; row_mean f32 [>= M]: the rows' centring offsets (read).  The GEMM wrapper
    checks M and N against these."""
    if stats_out.ndim != 3 or stats_out.shape[2] != 2 or stats_out.dtype != F32:
        _err(f"ln_producer: stats_out must be f32 [rows, N / 64, 2] (got {stats_out.dtype}, shape {tuple(stats_out.shape)})")
    if row_mean.dtype != F32 or row_mean.ndim != 1:
        _err(f"ln_producer: row_mean must be f32 [rows] (got {row_mean.dtype}, shape {tuple(row_mean.shape)})")
    f = _C.LnFuse()
    f.xs_out, f.ld_xs = _rows(xs_out, (BF,), "xs_out", stats_out.shape[1] * 64)
    f.next_scale = _table(next_scale, "ln_producer: next_scale", stats_out.shape[1] * 64)[0]
    f.stats_out = _p(stats_out, F32, "stats_out").value
    f.row_mean = _p(row_mean, F32, "row_mean").value
    f._keep = (xs_out, next_scale, stats_out, row_mean)
    return f


def _ln_ref(ln):
    return C.byref(ln) if ln is not None else None


def _check_consumer(ln, M: int, N: int, K: int, name: str):
    if ln is None:
        return
    if not ln.stats or ln.stats_out:
        _err(f"{name}: ln must come from ln_consumer")
    stats, c, _, _, row_mean = ln._keep
    if stats.shape[0] < M or stats.shape[1] * 64 != K:
        _err(f"{name}: stats must be [>= {M}, {K // 64}, 2] (got shape {tuple(stats.shape)})")
    if row_mean.numel() < M:
        _err(f"{name}: row_mean must hold {M} rows (got {row_mean.numel()})")
    if c.shape[1] < N:
        _err(f"{name}: the c / d tables must be at least {N} wide (got {c.shape[1]})")


def _check_producer(ln, M: int, N: int, gate: Tensor, name: str):
    if ln is None:
        return
    if not ln.stats_out or ln.stats:
        _err(f"{name}: ln must come from ln_producer")
    xs_out, next_scale, stats_out, row_mean = ln._keep
    if N % 64 or stats_out.shape[0] < M or stats_out.shape[1] != N // 64:
        _err(f"{name}: stats_out must be [>= {M}, N / 64 = {N / 64:g}, 2] (got shape {tuple(stats_out.shape)})")
    if row_mean.numel() < M or xs_out.shape[0] < M:
        _err(f"{name}: row_mean and xs_out must hold {M} rows (got {row_mean.numel()}, {xs_out.shape[0]})")
    if next_scale.shape[0] != gate.shape[0] or (gate.shape[0] > 1 and next_scale.stride(0) != gate.stride(0)):
        _err(f"{name}: next_scale must have the gate's rows and row stride")


def adaln_pre(x: Tensor, xs: Tensor, scale: Tensor, stats: Tensor, row_mean: Tensor, rows_per_seq: int,
              eval_ptr: Optional[Tensor] = None, eval_stride: int = 0):
    """Head of the fused-AdaLN chain: row_mean[row] = mean(x[row]), xs = bf16((x - mean) (1 + scale[r])), stats[row] =
    `parts` equal shares of (0, M2) (tile means relative to row_mean).  x f32 [rows, D], xs bf16 [>= rows, >= D] row-strided
    views; scale f32 [mod_rows, >= D]; stats f32 [>= rows, parts, 2]; row_mean f32 [>= rows]."""
    require_device()
    if x.ndim != 2:
        _err(f"adaln_pre: x must be [rows, D] (got shape {tuple(x.shape)})")
    rows, D = x.shape
    px, ldx = _rows(x, (F32,), "x", D)
    pxs, ld_xs = _rows(xs, (BF,), "xs", D)
    if xs.shape[0] < rows:
        _err(f"adaln_pre: xs has {xs.shape[0]} rows, fewer than x's {rows}")
    if stats.ndim != 3 or stats.shape[2] != 2 or stats.shape[0] < rows:
        _err(f"adaln_pre: stats must be f32 [>= {rows}, parts, 2] (got shape {tuple(stats.shape)})")
    if eval_ptr is not None and eval_stride <= 0:
        _err("adaln_pre: eval_ptr needs eval_stride")
    ps, mod_stride, mod_rows = _table(scale, "adaln_pre: scale", D)
    check(lib().f5e_adaln_pre(_stream(), px, ldx, pxs, ld_xs, ps, mod_stride, mod_rows, rows_per_seq,
                              _p(eval_ptr, I32, "eval_ptr"), eval_stride, _p(stats, F32, "stats"), stats.shape[1],
                              _flat(row_mean, F32, "row_mean", rows), rows, D), "f5e_adaln_pre")


def _gemm_operands(a: Tensor, w: Tensor, name: str):
    """(M, N, K, pa, lda, pw, ldw) of a [M, K] and w [N, K]: bf16 row-strided views (16-byte aligned rows: the LDS-DMA's unit)."""
    if a.ndim != 2 or w.ndim != 2 or a.shape[0] < 1 or w.shape[0] < 1:
        _err(f"{name}: a and w must be non-empty 2-D tensors (got shapes {tuple(a.shape)}, {tuple(w.shape)})")
    (M, K), N = a.shape, w.shape[0]
    if w.shape[1] != K:
        _err(f"{name}: w is [{N}, {w.shape[1]}], a is [{M}, {K}]: the K dimensions differ")
    if K % 64 or N % 4:
        _err(f"{name}: K = {K} must be a multiple of 64 and N = {N} a multiple of 4")
    pa, lda = _rows(a, (BF,), "a", K, vec=8)
    pw, ldw = _rows(w, (BF,), "w", K, vec=8)
    return M, N, K, pa, lda, pw, ldw


def gemm_bf16_bias(a: Tensor, w: Tensor, bias: Optional[Tensor], out: Tensor, act: int = ACT_NONE, tile_hint: int = 0,
                   ln=None):
    """out[M,N] = act(a[M,K] @ w[N,K].T + bias); out bf16 or f32 (no activation).  a, w, out: row-strided views with unit
    column stride (row strides multiples of 8 / 8 / 4 elements); bias f32 [>= N].  ln: ``ln_consumer(...)``.  Everything is
    refused here, before any launch."""
    require_device()
    M, N, K, pa, lda, pw, ldw = _gemm_operands(a, w, "gemm_bf16_bias")
    po, ldo = _rows(out, (BF, F32), "out", N)
    if out.shape[0] < M or out.data_ptr() % 16:
        _err(f"gemm_bf16_bias: out has {out.shape[0]} rows (a has {M}) at address % 16 = {out.data_ptr() % 16}: needs as many rows "
             f"as a and a 16-byte aligned base (the ping-pong kernel stores 16-byte pieces)")
    if act not in (ACT_NONE, ACT_GELU_TANH) or (act != ACT_NONE and out.dtype == F32):
        _err(f"gemm_bf16_bias: activation {act} with a {out.dtype} out (none or GELU(tanh); an f32 out takes none)")
    _check_consumer(ln, M, N, K, "gemm_bf16_bias")
    check(lib().f5e_gemm_bf16_bias_ln(_stream(), pa, lda, pw, ldw, _flat(bias, F32, "bias", N), po, ldo, M, N, K, act,
                                      1 if out.dtype == F32 else 0, tile_hint, _ln_ref(ln)), "f5e_gemm_bf16_bias")
    return out


def gemm_bf16_gate_residual(a: Tensor, w: Tensor, bias: Optional[Tensor], resid: Tensor, gate: Tensor,
                            rows_per_seq: int, seq_len: Optional[Tensor] = None, eval_ptr: Optional[Tensor] = None,
                            eval_stride: int = 0, tile_hint: int = 0, ln=None):
    """resid[M,N] += gate[seq % rows] * (a @ w.T + bias), rows past seq_len skipped.  resid f32 [>= M, >= N] row-strided view;
    gate: [rows, >= N] f32 view; seq_len int32 [>= ceil(M / rows_per_seq)].  ln: ``ln_producer(...)`` to also emit the next
    fused-AdaLN consumer's inputs.  Everything is refused here, before any launch."""
    require_device()
    M, N, K, pa, lda, pw, ldw = _gemm_operands(a, w, "gemm_bf16_gate_residual")
    pr, ldr = _rows(resid, (F32,), "resid", N)
    if resid.shape[0] < M:
        _err(f"gemm_bf16_gate_residual: resid has {resid.shape[0]} rows, fewer than a's {M}")
    pg, gate_stride, gate_rows = _table(gate, "gemm_bf16_gate_residual: gate", N)
    if rows_per_seq < 1:
        _err(f"gemm_bf16_gate_residual: rows_per_seq = {rows_per_seq}")
    if eval_ptr is not None and eval_stride <= 0:
        _err("gemm_bf16_gate_residual: eval_ptr needs eval_stride")
    _check_producer(ln, M, N, gate, "gemm_bf16_gate_residual")
    check(lib().f5e_gemm_bf16_gate_residual_ln(
        _stream(), pa, lda, pw, ldw, _flat(bias, F32, "bias", N), pr, ldr, pg, gate_stride, gate_rows,
        _p(eval_ptr, I32, "eval_ptr"), eval_stride, rows_per_seq,
        _flat(seq_len, I32, "seq_len", -(-M // rows_per_seq)), M, N, K, tile_hint, _ln_ref(ln)), "f5e_gemm_bf16_gate_residual")
    return resid


def gemm_bf16_qkv_rope(a: Tensor, w: Tensor, bias: Optional[Tensor], q: Tensor, k: Tensor, vt: Tensor, heads: int,
                       rope_heads: int, cos_sin: Tensor, rows_per_seq: int, tile_hint: int = 0,
                       q_norm_w: Optional[Tensor] = None, k_norm_w: Optional[Tensor] = None, ln=None):
    """Fused to_q / to_k / to_v + RoPE (f5e_gemm_bf16_qkv_rope): w [3 * heads * 64, K]; q, k [S, heads, n_pad, 64] and vt
    [S, heads, 64, n_pad] bf16, contiguous, S >= ceil(M / rows_per_seq); cos_sin f32 [>= rows_per_seq, 32, 2].  Everything is
    refused here, before any launch."""
    require_device()
    M, N, K, pa, lda, pw, ldw = _gemm_operands(a, w, "gemm_bf16_qkv_rope")
    if heads < 1 or N != 3 * heads * 64:
        _err(f"gemm_bf16_qkv_rope: w has {N} rows, not 3 * heads * 64 = {3 * heads * 64}")
    if q.ndim != 4 or rows_per_seq < 1:
        _err(f"gemm_bf16_qkv_rope: q must be [S, heads, n_pad, 64] (got shape {tuple(q.shape)}), rows_per_seq >= 1")
    n_pad = q.shape[2]
    if n_pad % 64 or n_pad < rows_per_seq:
        _err(f"gemm_bf16_qkv_rope: n_pad = {n_pad} must be a multiple of 64 and >= rows_per_seq = {rows_per_seq}")
    need = -(-M // rows_per_seq) * heads * n_pad * 64
    _check_consumer(ln, M, N, K, "gemm_bf16_qkv_rope")
    check(lib().f5e_gemm_bf16_qkv_rope_ln(
        _stream(), pa, lda, pw, ldw, _flat(bias, F32, "bias", N), _flat(q, BF, "q", need), _flat(k, BF, "k", need),
        _flat(vt, BF, "vt", need), n_pad, heads, rope_heads, _flat(cos_sin, F32, "cos_sin", rows_per_seq * 64),
        _flat(q_norm_w, F32, "q_norm_w", 64), _flat(k_norm_w, F32, "k_norm_w", 64), rows_per_seq, M, K, tile_hint,
        _ln_ref(ln)), "f5e_gemm_bf16_qkv_rope")


def qk_frag_index(n_pad: int) -> Tensor:
    """offset[pos, d] of the fragment-major Q/K layout (attention.hip): [pos/32][d/16][pos%32][(d/8)%2][d%8]."""
    pos = torch.arange(n_pad)[:, None]
    d = torch.arange(64)[None, :]
    return (((pos // 32) * 4 + d // 16) * 32 + pos % 32) * 16 + ((d // 8) % 2) * 8 + d % 8


def v_frag_index(n_pad: int) -> Tensor:
    """offset[key, d] of the fragment-major V layout: [key/32][(key%32)/16][d/32][d%32][h][j], key%16 = 8(j>>2)+4h+(j&3)."""
    key = torch.arange(n_pad)[:, None]
    d = torch.arange(64)[None, :]
    k16 = key % 16
    j = (k16 // 8) * 4 + k16 % 4
    h = (k16 // 4) % 2
    return (((((key // 32) * 2 + (key % 32) // 16) * 2 + d // 32) * 32 + d % 32) * 2 + h) * 8 + j


def flash_attn(q: Tensor, k: Tensor, vt: Tensor, out: Tensor, rows_per_seq: int, kv_len: Optional[Tensor] = None,
               waves: int = 0):
    """q, k, vt: [S, H, n_pad, 64]-sized bf16 buffers in the fragment-major layouts; ``waves`` = KV splits (0 auto)."""
    require_device()
    S, H, n_pad, _ = q.shape
    check(lib().f5e_flash_attn(_stream(), _p(q, BF, "q"), _p(k, BF, "k"), _p(vt, BF, "vt"), _p(out, BF, "out"),
                               out.stride(0), _p(kv_len, I32, "kv_len"), S, H, rows_per_seq, n_pad, waves),
          "f5e_flash_attn")
    return out


def joint_attn(qx: Tensor, kx: Tensor, vtx: Tensor, qc: Optional[Tensor], kc: Tensor, vtc: Tensor, out_x: Tensor,
               out_c: Optional[Tensor], N: int, Nt: int, kv_len: Optional[Tensor] = None, waves: int = 0):
    """MMDiT joint attention (f5e_joint_attn): keys = audio keys < kv_len[s] (all N if None) ++ all Nt text keys.
    qx, kx, vtx: [S, H, n_pad_x, 64]-sized and qc, kc, vtc: [S, H, n_pad_c, 64]-sized bf16 fragment-major buffers;
    out_x bf16 [S*N, >= H*64], out_c bf16 [S*Nt, >= H*64] or None (text queries skipped); ``waves`` = KV splits."""
    require_device()
    S, H, n_pad_x, _ = qx.shape
    n_pad_c = kc.shape[2]
    if kx.shape != qx.shape or vtx.numel() != qx.numel() or kc.shape[:2] != (S, H) or vtc.numel() != kc.numel():
        raise _C.F5EError("joint_attn: audio buffers [S, H, n_pad_x, 64], text buffers [S, H, n_pad_c, 64]")
    if out_c is not None and (qc is None or qc.shape != kc.shape):
        raise _C.F5EError("joint_attn: out_c needs qc of kc's shape")
    if out_x.shape[0] != S * N or (out_c is not None and out_c.shape[0] != S * Nt):
        raise _C.F5EError(f"joint_attn: out_x must have S*N = {S * N} rows and out_c S*Nt = {S * Nt}")
    if kv_len is not None and kv_len.numel() < S:
        raise _C.F5EError(f"joint_attn: kv_len needs one entry per sequence ({S})")
    check(lib().f5e_joint_attn(_stream(), _p(qx, BF, "qx"), _p(kx, BF, "kx"), _p(vtx, BF, "vtx"), _p(qc, BF, "qc"),
                               _p(kc, BF, "kc"), _p(vtc, BF, "vtc"), _p(out_x, BF, "out_x"), out_x.stride(0),
                               _p(out_c, BF, "out_c"), out_c.stride(0) if out_c is not None else 0,
                               _p(kv_len, I32, "kv_len"), S, H, N, n_pad_x, Nt, n_pad_c, waves), "f5e_joint_attn")
    return out_x, out_c


def layernorm(x: Tensor, out: Tensor, gamma: Optional[Tensor] = None, beta: Optional[Tensor] = None,
              scale: Optional[Tensor] = None, shift: Optional[Tensor] = None, rows_per_seq: int = 1,
              eval_ptr: Optional[Tensor] = None, eval_stride: int = 0, eps: float = 1e-6):
    """x f32 [rows, D], out f32 or bf16 [rows, D] (may be x itself); scale/shift: f32 [mod_rows, D].  x, out, scale and shift
    may be views with unit column stride and any row stride that is a multiple of 4, on a 16-byte aligned base (8-byte for a
    bf16 out): the kernels use vector accesses."""
    require_device()
    if x.ndim != 2 or out.shape != x.shape:
        raise _C.F5EError(f"layernorm: x and out must be [rows, D] of one shape (got {tuple(x.shape)}, {tuple(out.shape)})")
    rows, D = x.shape
    for t, nm in ((gamma, "gamma"), (beta, "beta")):
        if t is not None and t.numel() != D:
            raise _C.F5EError(f"layernorm: {nm} must have D = {D} elements")
    if (scale is None) != (shift is None):
        raise _C.F5EError("layernorm: scale and shift go together")
    xp, ldx = _rows(x, (F32,), "x", D)
    op, ldo = _rows(out, (F32, BF), "out", D)
    sp = hp = None
    mod_rows = mod_stride = 0
    if scale is not None:
        if shift.shape != scale.shape or scale.shape[1:] != (D,):
            raise _C.F5EError(f"layernorm: scale and shift must be [mod_rows, {D}]")
        mod_rows = scale.shape[0]
        (sp, mod_stride), (hp, shift_stride) = _rows(scale, (F32,), "scale", D), _rows(shift, (F32,), "shift", D)
        if shift_stride != mod_stride:
            raise _C.F5EError("scale and shift must share a row stride")
    check(lib().f5e_layernorm(_stream(), xp, ldx, op, ldo,
                              1 if out.dtype == BF else 0, _p(gamma, F32, "gamma"), _p(beta, F32, "beta"), sp, hp,
                              mod_stride, mod_rows, rows_per_seq, _p(eval_ptr, I32, "eval_ptr"), eval_stride, rows, D,
                              eps), "f5e_layernorm")
    return out


def l2norm(x: Tensor, out: Tensor, g: Tensor):
    """out = x / ||x|| * sqrt(D) * g (x_transformers.RMSNorm); x f32 [rows, D], out bf16 or f32, g f32 [D].  x and out may be
    views with unit column stride and any row stride that is a multiple of 4, on a 16-byte (bf16 out: 8-byte) aligned base."""
    require_device()
    if x.ndim != 2 or out.shape != x.shape or g.numel() != x.shape[1]:
        raise _C.F5EError(f"l2norm: x and out [rows, D], g [D] (got {tuple(x.shape)}, {tuple(out.shape)}, {tuple(g.shape)})")
    rows, D = x.shape
    (xp, ldx), (op, ldo) = _rows(x, (F32,), "x", D), _rows(out, (F32, BF), "out", D)
    check(lib().f5e_l2norm(_stream(), xp, ldx, op, ldo,
                           1 if out.dtype == BF else 0, _p(g, F32, "g"), rows, D), "f5e_l2norm")
    return out


def _shape3(x: Tensor, name: str):
    """(B, T, C) of a [B, T, C] activation; the pointer checks (f32, GPU, contiguous) stay with ``_p``."""
    if x.ndim != 3 or min(x.shape) < 1:
        raise _C.F5EError(f"{name} must be a non-empty [B, T, C] tensor (got shape {tuple(x.shape)})")
    return x.shape


def _shaped(t: Tensor, shape, name: str):
    if tuple(t.shape) != tuple(shape):
        raise _C.F5EError(f"{name} must be {list(shape)} (got shape {tuple(t.shape)})")


def grn(x: Tensor, out: Tensor, gamma: Tensor, beta: Tensor, ws: Tensor):
    """out = gamma (x gx / (mean_c gx + 1e-6)) + beta + x, gx = the L2 norm over T; x, out f32 [B, T, C], gamma, beta f32 [C],
    ws: f32 scratch of at least B * C elements (receives gx).  Everything is refused here, before any launch."""
    B, T, Cc = _shape3(x, "grn: x")
    _shaped(out, x.shape, "grn: out")
    _shaped(gamma, (Cc,), "grn: gamma")
    _shaped(beta, (Cc,), "grn: beta")
    if ws.numel() < B * Cc:
        raise _C.F5EError(f"grn: ws must hold B * C = {B * Cc} elements (got {ws.numel()})")
    require_device()
    check(lib().f5e_grn(_stream(), _p(x, F32, "x"), _p(out, F32, "out"), _p(ws, F32, "ws"), _p(gamma, F32, "gamma"),
                        _p(beta, F32, "beta"), B, T, Cc), "f5e_grn")
    return out


def _gemm_view(t: Tensor, dtype, name: str, cols: int, rows: int, overlap: bool = False, op: str = "gemm_f32"):
    """A row-strided operand of ``gemm_f32`` of which the kernel touches ``cols`` elements in each of ``rows`` rows: 2-D,
    ``dtype``, on the GPU, unit column stride, at least ``cols`` wide, and the storage behind the view holds
    (rows - 1) * row stride + cols elements.  Any alignment (the scalar epilogue and the plain kernel take what the vector
    paths cannot).  ``overlap``: rows may overlap (row stride < cols), for operands that are only read."""
    if t.ndim != 2 or not t.is_cuda or t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)) \
            or (t.shape[1] > 1 and t.stride(1) != 1):
        raise _C.F5EError(f"{op}: {name} must be a 2-D {dtype} GPU tensor with unit column stride (got {t.dtype}, "
                          f"{t.device}, shape {tuple(t.shape)}, strides {tuple(t.stride())})")
    if t.shape[1] < cols:
        raise _C.F5EError(f"{op}: {name} has {t.shape[1]} columns, fewer than the {cols} the problem needs")
    ld = t.stride(0)
    if rows > 1 and ld < (0 if overlap else cols):
        raise _C.F5EError(f"{op}: {name}: row stride {ld} is smaller than the {cols} columns of a row")
    if rows <= t.shape[0]:
        return                        # inside the view itself, which torch keeps inside its storage
    have = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
    need = (rows - 1) * ld + cols
    if have < need:
        raise _C.F5EError(f"{op}: {name}: {rows} rows of stride {ld} need {need} elements, the storage holds {have}")


def _gemm_f32(op: str, w_dtypes, a, w, bias, out, out_bf16, M, a_act, act, ch_scale, addend, row_scale, K):
    """``gemm_f32`` and ``gemm_f32_w16``: one set of checks, the entry point follows ``w.dtype``."""
    require_device()
    for t, nm, dts in ((a, "a", (F32,)), (w, "w", w_dtypes)):
        if t.ndim != 2 or not t.is_cuda or t.dtype not in dts or (t.stride(1) != 1 and t.shape[1] > 1):
            raise _C.F5EError(f"{op}: {nm} must be a 2-D {'f32' if dts == (F32,) else 'fp16 / bf16'} GPU tensor with unit column "
                              f"stride (got {getattr(t, 'dtype', None)})")
    a_rows = a.shape[0]
    K = a.shape[1] if K is None else int(K)
    N = w.shape[0]
    M = a_rows if M is None else int(M)
    if K > a.shape[1] or K > w.shape[1]:
        raise _C.F5EError(f"{op}: K = {K} is larger than a's width {a.shape[1]} or w's width {w.shape[1]}")
    if out is None and out_bf16 is None:
        raise _C.F5EError(f"{op}: needs out or out_bf16")
    if M > 0 and N > 0 and K > 0:     # the library refuses the empty problem itself
        _gemm_view(a, F32, "a", K, min(M, a_rows), overlap=True, op=op)
        _gemm_view(w, w_dtypes, "w", K, N, overlap=True, op=op)
        if out is not None:
            _gemm_view(out, F32, "out", N, M, op=op)
        if out_bf16 is not None:
            _gemm_view(out_bf16, BF, "out_bf16", N, M, op=op)
        if addend is not None:
            if addend.ndim == 2 and addend.shape[0] < 1:      # its data_ptr() is null: the library would see no addend at all
                raise _C.F5EError(f"{op}: addend must have at least one row")
            _gemm_view(addend, F32, "addend", N, min(M, addend.shape[0]) if addend.ndim == 2 else 1, op=op)
        for t, nm, n in ((bias, "bias", N), (ch_scale, "ch_scale", N), (row_scale, "row_scale", M)):
            if t is not None and t.numel() < n:
                raise _C.F5EError(f"{op}: {nm} must hold at least {n} elements (got {t.numel()})")
    ad = addend
    if w.dtype != F32 and (w.data_ptr() % 8 or w.stride(0) % 4):    # the fp32 op takes any alignment; 16-bit loads are 8 bytes
        raise _C.F5EError(f"{op}: w must be 8-byte aligned with a row stride that is a multiple of 4 (got offset "
                          f"{w.data_ptr() % 8}, stride {w.stride(0)})")
    front = (_stream(), C.c_void_p(a.data_ptr()), a.stride(0), a_rows, a_act, C.c_void_p(w.data_ptr()), w.stride(0))
    rest = (_p(bias, F32, "bias"), act, _p(ch_scale, F32, "ch_scale"),
            C.c_void_p(ad.data_ptr()) if ad is not None else None, ad.stride(0) if ad is not None else 0,
            ad.shape[0] if ad is not None else 0, _p(row_scale, F32, "row_scale"),
            C.c_void_p(out.data_ptr()) if out is not None else None, out.stride(0) if out is not None else 0,
            C.c_void_p(out_bf16.data_ptr()) if out_bf16 is not None else None,
            out_bf16.stride(0) if out_bf16 is not None else 0, M, N, K)
    if w.dtype == F32:
        check(lib().f5e_gemm_f32(*front, *rest), "f5e_gemm_f32")
    else:
        check(lib().f5e_gemm_f32_w16(*front, W16_TYPES[w.dtype], *rest), "f5e_gemm_f32_w16")
    return out if out is not None else out_bf16


def gemm_f32(a: Tensor, w: Tensor, bias: Optional[Tensor] = None, *, out: Optional[Tensor] = None,
             out_bf16: Optional[Tensor] = None, M: Optional[int] = None, a_act: int = ACT_NONE, act: int = ACT_NONE,
             ch_scale: Optional[Tensor] = None, addend: Optional[Tensor] = None, row_scale: Optional[Tensor] = None,
             K: Optional[int] = None):
    """fp32 MFMA GEMM; ``a`` [a_rows, >=K] and ``w`` [N, >=K] may be column-sliced views (row stride = ld; ``a``'s may be
    smaller than its width: overlapping rows).  out f32 / out_bf16 bf16 [>= M rows of storage, >= N] and addend f32
    [add_rows, >= N] are row-strided views with unit column stride, of any alignment; bias, ch_scale [>= N] and row_scale
    [>= M] are contiguous.  Row m reads a[m % a_rows] and addend[m % add_rows].  Everything is refused here, before any launch."""
    return _gemm_f32("gemm_f32", (F32,), a, w, bias, out, out_bf16, M, a_act, act, ch_scale, addend, row_scale, K)


def gemm_f32_w16(a: Tensor, w: Tensor, bias: Optional[Tensor] = None, *, out: Optional[Tensor] = None,
                 out_bf16: Optional[Tensor] = None, M: Optional[int] = None, a_act: int = ACT_NONE, act: int = ACT_NONE,
                 ch_scale: Optional[Tensor] = None, addend: Optional[Tensor] = None, row_scale: Optional[Tensor] = None,
                 K: Optional[int] = None):
    """``gemm_f32`` with a 16-bit weight (f5e_gemm_f32_w16): ``w`` fp16 or bf16 [N, >= K], 8-byte aligned, row stride a multiple
    of 4; it is widened to fp32 in registers, everything else is fp32 and as ``gemm_f32`` takes it.  Bit-equal to
    ``gemm_f32(a, w.float(), ...)`` with that widened copy 16-byte aligned (a contiguous ``w.float()`` is; ``gemm_f32`` sums in
    another order for a widened view that is not, and this op cannot know of it), at half the bytes of ``w``.  Everything is
    refused here, before any launch."""
    return _gemm_f32("gemm_f32_w16", tuple(W16_TYPES), a, w, bias, out, out_bf16, M, a_act, act, ch_scale, addend, row_scale, K)


def pack_convpos_weight(w: Tensor, groups: int = 16) -> Tensor:
    """Conv1d weight [D][D/groups][31] -> bf16 [groups][31][64 oc][64 ic] (zero padded to 64 x 64 per group)."""
    D, cpg, taps = w.shape
    out = torch.zeros(groups, taps, 64, 64, dtype=w.dtype, device=w.device)
    out[:, :, :cpg, :cpg] = w.view(groups, cpg, cpg, taps).permute(0, 3, 1, 2)
    return out.to(BF).contiguous()


def _vec(t: Tensor, dtype, name: str, shape, align: int = 4):
    """Pointer of a contiguous ``dtype`` GPU tensor of exactly ``shape`` whose base is ``align``-byte aligned."""
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        _err(f"{name} must be {dtype} {list(shape)} (got {t.dtype}, shape {tuple(t.shape)})")
    ptr = _p(t, dtype, name)
    if t.data_ptr() % align:
        _err(f"{name}: base address must be {align}-byte aligned")
    return ptr


def convpos(x: Tensor, w_packed: Tensor, bias: Tensor, S: int, N: int, *, out_bf16: Optional[Tensor] = None,
            out_f32: Optional[Tensor] = None, resid: Optional[Tensor] = None):
    """Grouped Conv1d(D, D, 31, padding 15) + Mish over S sequences of N rows (f5e_convpos).  x bf16 [S * N, D] view (unit
    column stride, row stride a multiple of 8, 16-byte aligned base); w_packed bf16 [G, 31, 64, 64] (``pack_convpos_weight``),
    D / G in {16, 32, 48, 64}; bias f32 [D].  Exactly one output: out_bf16 = mish(conv + bias) bf16 [S * N, D], or out_f32 =
    mish(conv + bias) + resid, both f32 [S * N, D]; outputs and resid are views with unit column stride and a row stride
    that is a multiple of 4, and need not be contiguous.  Everything is refused here or by the library, before any launch."""
    S, N = int(S), int(N)
    if S < 1 or N < 1:
        _err(f"convpos: needs S >= 1 and N >= 1 (got {S}, {N})")
    if x.ndim != 2 or x.shape[0] != S * N:
        _err(f"convpos: x must be [S * N, D] = [{S * N}, D] (got shape {tuple(x.shape)})")
    D = x.shape[1]
    if w_packed.ndim != 4 or tuple(w_packed.shape[1:]) != (31, 64, 64) or w_packed.shape[0] < 1:
        _err(f"convpos: w_packed must be bf16 [G, 31, 64, 64] (got shape {tuple(w_packed.shape)})")
    G = w_packed.shape[0]
    if D % G or D // G not in (16, 32, 48, 64):
        _err(f"convpos: D / G = {D} / {G} must be 16, 32, 48 or 64")
    if (out_bf16 is None) == (out_f32 is None):
        _err("convpos: exactly one of out_bf16 and out_f32 must be given")
    if (resid is None) != (out_f32 is None):
        _err("convpos: resid goes with out_f32, and only with it")
    require_device()
    xp, ldx = _rows(x, (BF,), "convpos: x", D, vec=8)
    wp = _vec(w_packed, BF, "convpos: w_packed", (G, 31, 64, 64), 16)
    bp = _vec(bias, F32, "convpos: bias", (D,), 16)
    op, ldo, o32p, ldo32, rp, ldr = None, 0, None, 0, None, 0
    if out_bf16 is not None:
        _shaped(out_bf16, (S * N, D), "convpos: out_bf16")
        op, ldo = _rows(out_bf16, (BF,), "convpos: out_bf16", D)
    else:
        _shaped(out_f32, (S * N, D), "convpos: out_f32")
        _shaped(resid, (S * N, D), "convpos: resid")
        o32p, ldo32 = _rows(out_f32, (F32,), "convpos: out_f32", D)
        rp, ldr = _rows(resid, (F32,), "convpos: resid", D)
    check(lib().f5e_convpos(_stream(), xp, ldx, wp, bp, 0 if out_f32 is None else 1, op, ldo, o32p, ldo32, rp, ldr, S, N, D, G),
          "f5e_convpos")
    return out_bf16 if out_f32 is None else out_f32


def dwconv7(x: Tensor, w_t: Tensor, bias: Tensor, out: Tensor):
    """Depthwise Conv1d(C, C, 7, padding 3), channels-last: x, out f32 [B, T, C], w_t f32 [7, C] (tap-major), bias f32 [C].
    Everything is refused here or by the library (C % 4), before any launch."""
    B, T, Cc = _shape3(x, "dwconv7: x")
    _shaped(out, x.shape, "dwconv7: out")
    _shaped(w_t, (7, Cc), "dwconv7: w_t")
    _shaped(bias, (Cc,), "dwconv7: bias")
    require_device()
    check(lib().f5e_dwconv7(_stream(), _p(x, F32, "x"), _p(w_t, F32, "w_t"), _p(bias, F32, "bias"), _p(out, F32, "out"),
                            B, T, Cc), "f5e_dwconv7")
    return out


def im2col(x: Tensor, col: Tensor, ksize: int, pad: int):
    """col[b, t, j * Cin + ic] = x[b, t + j - pad, ic], zero outside [0, T): x f32 [B, T, Cin], col f32 [B, T, ksize * Cin].
    Everything is refused here, before any launch."""
    B, T, Cin = _shape3(x, "im2col: x")
    ksize, pad = int(ksize), int(pad)
    if ksize < 1 or pad < 0:
        raise _C.F5EError(f"im2col: needs ksize >= 1 and pad >= 0 (got {ksize}, {pad})")
    _shaped(col, (B, T, ksize * Cin), "im2col: col")
    require_device()
    check(lib().f5e_im2col(_stream(), _p(x, F32, "x"), _p(col, F32, "col"), B, T, Cin, ksize, pad), "f5e_im2col")
    return col


def pack_conv2d_sub_weight(w: Tensor) -> Tensor:
    """Conv2d weight [C_out][C_in][kt][kf] -> [C_out][kt][kf][C_in], the [N][K] matrix of ``conv2d_sub``."""
    return w.permute(0, 2, 3, 1).contiguous()


def conv2d_sub(x: Tensor, w_packed: Tensor, bias: Optional[Tensor], stride: int, *, out: Optional[Tensor] = None,
               act: int = ACT_RELU) -> Tensor:
    """Strided Conv2d without padding as an implicit GEMM (f5e_conv2d_sub_f32): x f32 [B, T_in, F_in, C] channels-last,
    w_packed f32 [C, kt, kf, C] (``pack_conv2d_sub_weight``), bias f32 [C] or None -> act(conv) f32 [B, T_out, F_out, C].
    No workspace.  Everything is refused here or by the library before any launch."""
    require_device()
    if x.ndim != 4 or w_packed.ndim != 4:
        raise _C.F5EError(f"conv2d_sub: x [B, T, F, C] and w [C, kt, kf, C] (got {tuple(x.shape)}, {tuple(w_packed.shape)})")
    B, T_in, F_in, Cc = x.shape
    N, kt, kf, Cw = w_packed.shape
    if N != Cc or Cw != Cc or Cc % 16:
        raise _C.F5EError(f"conv2d_sub: a C -> C convolution with C a multiple of 16 (x has {Cc}, w is {tuple(w_packed.shape)})")
    if T_in < kt or F_in < kf or stride < 1:
        raise _C.F5EError(f"conv2d_sub: input [{T_in}, {F_in}] is smaller than the kernel [{kt}, {kf}] (stride {stride})")
    if bias is not None and bias.numel() != Cc:
        raise _C.F5EError(f"conv2d_sub: bias must have C = {Cc} elements")
    T_out, F_out = (T_in - kt) // stride + 1, (F_in - kf) // stride + 1
    if out is None:
        out = torch.empty(B, T_out, F_out, Cc, device=x.device, dtype=F32)
    if tuple(out.shape) != (B, T_out, F_out, Cc):
        raise _C.F5EError(f"conv2d_sub: out must be [{B}, {T_out}, {F_out}, {Cc}] (got {tuple(out.shape)})")
    check(lib().f5e_conv2d_sub_f32(_stream(), _p(x, F32, "x"), _p(w_packed, F32, "w_packed"), _p(bias, F32, "bias"),
                                   _p(out, F32, "out"), B, T_in, F_in, Cc, kt, kf, stride, act), "f5e_conv2d_sub_f32")
    return out


def sinus_embed(t: Tensor, freqs: Tensor, out: Tensor, scale: float = 1000.0):
    """out[e] = cat(sin(a), cos(a)), a = (scale t[e]) freqs[k]: t f32 [E], freqs f32 [dim / 2], out f32 [E, dim], all contiguous
    on the GPU.  Everything is refused here or by the library (dim even and >= 4), before any launch."""
    if out.ndim != 2 or out.shape[0] < 1 or out.shape[1] % 2:
        _err(f"sinus_embed: out must be f32 [E, dim] with dim even (got shape {tuple(out.shape)})")
    E, dim = out.shape
    require_device()
    check(lib().f5e_sinus_embed(_stream(), _vec(t, F32, "sinus_embed: t", (E,)), _vec(freqs, F32, "sinus_embed: freqs", (dim // 2,)),
                                _p(out, F32, "sinus_embed: out"), E, dim, scale), "f5e_sinus_embed")
    return out


def rope_table(inv_freq: Tensor, out: Tensor):
    """out[n, i] = (cos, sin)(n inv_freq[i]): inv_freq f32 [half], out f32 [N, half, 2], both contiguous on the GPU.
    Everything is refused here, before any launch."""
    if out.ndim != 3 or out.shape[2] != 2 or min(out.shape) < 1:
        _err(f"rope_table: out must be f32 [N, half, 2] (got shape {tuple(out.shape)})")
    N, half, _ = out.shape
    require_device()
    check(lib().f5e_rope_table(_stream(), _vec(inv_freq, F32, "rope_table: inv_freq", (half,)), _p(out, F32, "rope_table: out"),
                               N, half), "f5e_rope_table")
    return out


def text_gather(ids: Tensor, table: Tensor, pos: Optional[Tensor], keep: Optional[Tensor], out: Tensor):
    require_device()
    B, N, TD = out.shape
    check(lib().f5e_text_gather(_stream(), _p(ids, I32, "ids"), _p(table, F32, "table"), _p(pos, F32, "pos"),
                                _p(keep, F32, "keep"), _p(out, F32, "out"), B, N, TD,
                                pos.shape[0] if pos is not None else 1, table.shape[0]), "f5e_text_gather")
    return out


def ode_update(pred: Tensor, branch_stride: int, mode: int, w0: float, w1: float, base: Tensor, dst: Tensor,
               coef: Tensor, eval_ptr: Optional[Tensor], traj: Optional[Tensor] = None,
               done_ctr: Optional[Tensor] = None, traj_stride: int = 0, traj_div: int = 1):
    """done_ctr (int32[1], zero): the kernel itself advances *eval_ptr after every block has read it.
    traj_stride > 0: ``traj`` is the whole [rows, ...] trajectory and row (*eval_ptr + 1) // traj_div gets the copy."""
    require_device()
    check(lib().f5e_ode_update_traj(_stream(), _p(pred, F32, "pred"), branch_stride, mode, w0, w1, _p(base, F32, "base"),
                                    _p(dst, F32, "dst"), C.c_void_p(traj.data_ptr()) if traj is not None else None,
                                    traj_stride, traj_div, _p(coef, F32, "coef"), _p(eval_ptr, I32, "eval_ptr"),
                                    _p(done_ctr, I32, "done_ctr"), base.numel()), "f5e_ode_update")
    return dst


def sample_loop(loop: "_C.LoopPlan"):
    """Enqueue loop.steps ODE steps (network evaluation(s) + guidance combine + Euler / midpoint update) on the current stream."""
    require_device()
    check(lib().f5e_sample_loop(_stream(), C.byref(loop)), "f5e_sample_loop")


def advance_eval(eval_ptr: Tensor):
    require_device()
    check(lib().f5e_advance_eval(_stream(), _p(eval_ptr, I32, "eval_ptr")), "f5e_advance_eval")


def stitch(cond: Tensor, y: Tensor, mask_u8: Tensor, out: Tensor):
    require_device()
    Cc = cond.shape[-1]
    check(lib().f5e_stitch(_stream(), _p(cond, F32, "cond"), _p(y, F32, "y"), _p(mask_u8, U8, "mask"),
                           _p(out, F32, "out"), cond.numel() // Cc, Cc), "f5e_stitch")
    return out


def cast_bf16(x: Tensor, out: Tensor):
    require_device()
    check(lib().f5e_cast_bf16(_stream(), _p(x, F32, "x"), _p(out, BF, "out"), x.numel()), "f5e_cast_bf16")
    return out


def cast_f32(x: Tensor, out: Tensor):
    require_device()
    check(lib().f5e_cast_f32(_stream(), _p(x, BF, "x"), _p(out, F32, "out"), x.numel()), "f5e_cast_f32")
    return out


def axpby(x: Tensor, y: Optional[Tensor], out: Tensor, a: float = 1.0, b: float = 1.0, c: float = 0.0):
    """out = a x + b y + c (y optional), f32 contiguous tensors of equal size."""
    require_device()
    if y is not None and y.numel() != x.numel() or out.numel() != x.numel():
        raise _C.F5EError("axpby: size mismatch")
    check(lib().f5e_axpby(_stream(), _p(x, F32, "x"), _p(y, F32, "y"), _p(out, F32, "out"), a, b, c, x.numel()),
          "f5e_axpby")
    return out


def vq_eval(logits: Tensor, vars_: Tensor, combine_groups: bool, out: Tensor, targets: Tensor,
            stats: Optional[Tensor], groups: int, num_vars: int):
    require_device()
    rows = logits.shape[0]
    check(lib().f5e_vq_eval(_stream(), _p(logits, F32, "logits"), logits.stride(0), _p(vars_, F32, "vars"),
                            1 if combine_groups else 0, _p(out, F32, "out"), _p(targets, I32, "targets"),
                            _p(stats, F32, "stats"), rows, groups, num_vars, vars_.shape[-1]), "f5e_vq_eval")
    return out


def mas_workspace_bytes(B: int, Ty: int, Tx: int) -> int:
    """Scratch bytes of ``mas_path`` for a [B, Ty, Tx] problem (host call)."""
    n = C.c_ulonglong()
    check(lib().f5e_mas_workspace_bytes(B, Ty, Tx, C.byref(n)), "f5e_mas_workspace_bytes")
    return int(n.value)


def mas_path(logp: Tensor, t_y: Tensor, t_x: Tensor, token_of_frame: Tensor, durations: Optional[Tensor] = None,
             workspace: Optional[Tensor] = None):
    """Monotonic alignment search (f5e_mas_path): logp f32 [B, Ty, Tx] (frame x token; batch / row strides free, unit
    column stride), t_y / t_x i32 [B] on the device -> token_of_frame i32 [B, Ty] (-1 past t_y), durations i32 [B, Tx]
    (optional).  workspace: a device tensor of at least ``mas_workspace_bytes`` bytes (allocated here when None)."""
    require_device()
    if logp.ndim != 3 or not logp.is_cuda or logp.dtype != F32 or logp.stride(2) != 1:
        raise _C.F5EError("mas_path: logp must be an f32 GPU tensor [B, Ty, Tx] with unit column stride; there is no "
                          "CPU path")
    B, Ty, Tx = logp.shape
    if t_y.numel() != B or t_x.numel() != B or token_of_frame.shape != (B, Ty) or \
            (durations is not None and durations.shape != (B, Tx)):
        raise _C.F5EError(f"mas_path: lengths [{B}], token_of_frame [{B}, {Ty}], durations [{B}, {Tx}]")
    workspace, nbytes = _workspace(workspace, mas_workspace_bytes(B, Ty, Tx), torch.int64, logp.device)
    check(lib().f5e_mas_path(_stream(), C.c_void_p(logp.data_ptr()), logp.stride(0), logp.stride(1), _p(t_y, I32, "t_y"),
                             _p(t_x, I32, "t_x"), _p(token_of_frame, I32, "token_of_frame"),
                             _p(durations, I32, "durations"), _p(workspace, None, "workspace"), nbytes, B, Ty, Tx),
          "f5e_mas_path")
    return token_of_frame, durations


def ctc_align_workspace_bytes(B: int, T: int, L: int) -> int:
    """Scratch bytes of ``ctc_align`` for B sequences of up to T frames and L labels (host call)."""
    n = C.c_ulonglong()
    check(lib().f5e_ctc_align_workspace_bytes(B, T, L, C.byref(n)), "f5e_ctc_align_workspace_bytes")
    return int(n.value)


def _ctc_scores(scores: Tensor, name: str):
    if scores.ndim != 3 or not scores.is_cuda or scores.dtype != F32 or scores.stride(2) != 1:
        raise _C.F5EError(f"{name}: scores must be an f32 GPU tensor [B, T, V] with unit class stride; there is no CPU path")
    return scores.shape


def _row_stride(t: Tensor, width: int) -> int:
    """Row stride of a [.., rows, width] view: the stride of a size-1 dimension is arbitrary (0 for a NumPy new axis) and
    never used, so one row reports at least its own width."""
    return t.stride(-2) if t.shape[-2] > 1 else max(width, t.stride(-2))


def _workspace(workspace: Optional[Tensor], need: int, dtype, device):
    """(workspace, its bytes): ``need`` bytes of ``dtype`` words are allocated when the caller passed None."""
    if workspace is None:
        workspace = torch.empty((need + dtype.itemsize - 1) // dtype.itemsize, dtype=dtype, device=device)
    return workspace, workspace.numel() * workspace.element_size()


def ctc_align(scores: Tensor, labels: Tensor, t_len: Tensor, l_len: Tensor, blank: int = 0, *,
              align: Optional[Tensor] = None, tok_start: Optional[Tensor] = None, tok_end: Optional[Tensor] = None,
              score: Optional[Tensor] = None, spans: bool = True, workspace: Optional[Tensor] = None):
    """CTC forced alignment (f5e_ctc_align): scores f32 [B, T, V] (log-probabilities or raw logits; batch / row strides free,
    unit class stride, only read), labels i32 [B, L], t_len / l_len i32 [B] on the device -> (align i32 [B, T]: the class of
    every frame's state, -1 past t_len; tok_start, tok_end i32 [B, L]; score f32 [B]).  Outputs are allocated here when not
    given; ``spans=False`` skips the three optional ones that were not passed.  workspace: a device tensor of at least
    ``ctc_align_workspace_bytes`` bytes (allocated here when None)."""
    B, T, V = _ctc_scores(scores, "ctc_align")
    if labels.ndim != 2 or labels.shape[0] != B or labels.stride(1) != 1 or labels.dtype != I32 or not labels.is_cuda:
        raise _C.F5EError(f"ctc_align: labels must be an i32 GPU tensor [{B}, L] with unit label stride")
    require_device()
    L = labels.shape[1]
    dev = scores.device
    if align is None:
        align = torch.empty(B, T, dtype=I32, device=dev)
    if spans:
        tok_start = torch.empty(B, L, dtype=I32, device=dev) if tok_start is None else tok_start
        tok_end = torch.empty(B, L, dtype=I32, device=dev) if tok_end is None else tok_end
        score = torch.empty(B, dtype=F32, device=dev) if score is None else score
    if t_len.numel() != B or l_len.numel() != B or align.shape != (B, T) or \
            any(o is not None and o.shape != (B, L) for o in (tok_start, tok_end)) or \
            (score is not None and score.shape != (B,)):
        raise _C.F5EError(f"ctc_align: lengths [{B}], align [{B}, {T}], tok_start / tok_end [{B}, {L}], score [{B}]")
    workspace, nbytes = _workspace(workspace, ctc_align_workspace_bytes(B, T, L), torch.int64, dev)
    ld, ld_labels = _row_stride(scores, V), (labels.stride(0) if B > 1 else L)
    check(lib().f5e_ctc_align(_stream(), C.c_void_p(scores.data_ptr()), scores.stride(0), ld,
                              C.c_void_p(labels.data_ptr()), ld_labels, _p(t_len, I32, "t_len"),
                              _p(l_len, I32, "l_len"), int(blank), _p(align, I32, "align"), _p(tok_start, I32, "tok_start"),
                              _p(tok_end, I32, "tok_end"), _p(score, F32, "score"), _p(workspace, None, "workspace"),
                              nbytes, B, T, L, V), "f5e_ctc_align")
    return align, tok_start, tok_end, score


def ctc_greedy(scores: Tensor, t_len: Tensor, blank: int = 0, pad_id: int = -1, *, hyp: Optional[Tensor] = None,
               hyp_len: Optional[Tensor] = None, frame_logp: Optional[Tensor] = None, want_logp: bool = False):
    """CTC best-path decoding (f5e_ctc_greedy): scores f32 [B, T, V] as in ``ctc_align``, t_len i32 [B] on the device ->
    (hyp i32 [B, T] padded with -1, hyp_len i32 [B], frame_logp f32 [B, T] or None).  Frames past t_len take ``pad_id`` when
    it is >= 0 (the reference's eos fill) and are skipped when it is -1.  frame_logp (max - logsumexp of every row) is
    computed when a tensor is passed or ``want_logp`` is set."""
    B, T, V = _ctc_scores(scores, "ctc_greedy")
    require_device()
    dev = scores.device
    hyp = torch.empty(B, T, dtype=I32, device=dev) if hyp is None else hyp
    hyp_len = torch.empty(B, dtype=I32, device=dev) if hyp_len is None else hyp_len
    if frame_logp is None and want_logp:
        frame_logp = torch.empty(B, T, dtype=F32, device=dev)
    if t_len.numel() != B or hyp.shape != (B, T) or hyp_len.shape != (B,) or \
            (frame_logp is not None and frame_logp.shape != (B, T)):
        raise _C.F5EError(f"ctc_greedy: t_len / hyp_len [{B}], hyp / frame_logp [{B}, {T}]")
    check(lib().f5e_ctc_greedy(_stream(), C.c_void_p(scores.data_ptr()), scores.stride(0), _row_stride(scores, V),
                               _p(t_len, I32, "t_len"), int(blank), int(pad_id), _p(hyp, I32, "hyp"),
                               _p(hyp_len, I32, "hyp_len"), _p(frame_logp, F32, "frame_logp"), B, T, V), "f5e_ctc_greedy")
    return hyp, hyp_len, frame_logp


def ctc_loss_workspace_bytes(B: int, T: int) -> int:
    """Scratch bytes of ``ctc_loss`` for B sequences of up to T frames (host call)."""
    n = C.c_ulonglong()
    check(lib().f5e_ctc_loss_workspace_bytes(B, T, C.byref(n)), "f5e_ctc_loss_workspace_bytes")
    return int(n.value)


def ctc_loss(scores: Tensor, labels: Tensor, t_len: Tensor, l_len: Tensor, blank: int = 0, *,
             logp: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tensor:
    """CTC likelihood of a transcript (f5e_ctc_loss): scores f32 [B, T, V] as in ``ctc_align`` (raw logits or
    log-probabilities, the kernel normalises every frame; only read), labels i32 [B, L] (L may be 0; adjacent equal labels
    are fine), t_len / l_len i32 [B] on the device -> logp f32 [B] = log of the sum over all CTC paths =
    ``-torch.nn.functional.ctc_loss(reduction="none")``; -inf for a sequence without a path.  No gradient.  workspace: a
    device tensor of at least ``ctc_loss_workspace_bytes`` bytes (allocated here when None)."""
    B, T, V = _ctc_scores(scores, "ctc_loss")
    if labels.ndim != 2 or labels.shape[0] != B or (labels.shape[1] > 1 and labels.stride(1) != 1) or \
            labels.dtype != I32 or not labels.is_cuda:
        raise _C.F5EError(f"ctc_loss: labels must be an i32 GPU tensor [{B}, L] with unit label stride")
    require_device()
    L = labels.shape[1]
    dev = scores.device
    if logp is None:
        logp = torch.empty(B, dtype=F32, device=dev)
    if t_len.numel() != B or l_len.numel() != B or logp.shape != (B,):
        raise _C.F5EError(f"ctc_loss: lengths [{B}], logp [{B}]")
    workspace, nbytes = _workspace(workspace, ctc_loss_workspace_bytes(B, T), F32, dev)
    ld, ld_labels = _row_stride(scores, V), (labels.stride(0) if B > 1 and L > 0 else L)
    check(lib().f5e_ctc_loss(_stream(), C.c_void_p(scores.data_ptr()), scores.stride(0), ld,
                             C.c_void_p(labels.data_ptr() if L > 0 else None), ld_labels, _p(t_len, I32, "t_len"),
                             _p(l_len, I32, "l_len"), int(blank), _p(logp, F32, "logp"), _p(workspace, None, "workspace"),
                             nbytes, B, T, L, V), "f5e_ctc_loss")
    return logp


def ctc_beam_workspace_bytes(B: int, T: int, beam: int) -> int:
    """Scratch bytes of ``ctc_beam_search`` for B sequences of up to T frames at beam size ``beam`` (host call)."""
    n = C.c_ulonglong()
    check(lib().f5e_ctc_beam_workspace_bytes(B, T, beam, C.byref(n)), "f5e_ctc_beam_workspace_bytes")
    return int(n.value)


def ctc_beam_search(scores: Tensor, t_len: Tensor, beam: int, blank: int = 0, *, ld_hyp: Optional[int] = None,
                    hyp: Optional[Tensor] = None, hyp_len: Optional[Tensor] = None, score: Optional[Tensor] = None,
                    workspace: Optional[Tensor] = None):
    """CTC prefix beam search (f5e_ctc_beam): scores f32 [B, T, V] as in ``ctc_align`` (raw logits or log-probabilities, the
    kernel normalises every frame), t_len i32 [B] on the device -> (hyp i32 [B, beam, ld_hyp] padded with -1, best first;
    hyp_len i32 [B, beam], the true lengths; score f32 [B, beam]).  ld_hyp defaults to T, which no prefix exceeds.
    workspace: a device tensor of at least ``ctc_beam_workspace_bytes`` bytes (allocated here when None)."""
    B, T, V = _ctc_scores(scores, "ctc_beam_search")
    if t_len.dtype != I32 or not t_len.is_cuda or t_len.numel() != B:
        raise _C.F5EError(f"ctc_beam_search: t_len must be an i32 GPU tensor [{B}]")
    beam = int(beam)
    if not 1 <= beam <= min(16, V):
        raise _C.F5EError(f"ctc_beam_search: beam must lie in 1..min(16, V = {V}), got {beam}")
    require_device()
    dev = scores.device
    if hyp is not None:
        if hyp.ndim != 3 or not hyp.is_contiguous():
            raise _C.F5EError(f"ctc_beam_search: hyp must be a contiguous i32 tensor [{B}, {beam}, ld_hyp]")
        ld_hyp = hyp.shape[2]
    ld_hyp = T if ld_hyp is None else int(ld_hyp)
    hyp = torch.empty(B, beam, ld_hyp, dtype=I32, device=dev) if hyp is None else hyp
    hyp_len = torch.empty(B, beam, dtype=I32, device=dev) if hyp_len is None else hyp_len
    score = torch.empty(B, beam, dtype=F32, device=dev) if score is None else score
    if ld_hyp < 1 or hyp.shape != (B, beam, ld_hyp) or hyp_len.shape != (B, beam) or score.shape != (B, beam) or \
            not (hyp_len.is_contiguous() and score.is_contiguous()):
        raise _C.F5EError(f"ctc_beam_search: hyp [{B}, {beam}, ld_hyp >= 1], hyp_len / score [{B}, {beam}], contiguous")
    workspace, nbytes = _workspace(workspace, ctc_beam_workspace_bytes(B, T, beam), torch.int64, dev)
    check(lib().f5e_ctc_beam(_stream(), C.c_void_p(scores.data_ptr()), scores.stride(0), _row_stride(scores, V),
                             _p(t_len, I32, "t_len"), int(blank),
                             beam, _p(hyp, I32, "hyp"), ld_hyp, _p(hyp_len, I32, "hyp_len"), _p(score, F32, "score"),
                             _p(workspace, None, "workspace"), nbytes, B, T, V), "f5e_ctc_beam")
    return hyp, hyp_len, score


class CTCBeamState:
    """The resumable search's state: ``buf`` (device memory, opaque) and the geometry it was initialised for."""

    def __init__(self, buf: Tensor, B: int, T_cap: int, chunk_cap: int, beam: int):
        self.buf, self.B, self.T_cap, self.chunk_cap, self.beam = buf, B, T_cap, chunk_cap, beam

    @property
    def nbytes(self) -> int:
        return self.buf.numel() * self.buf.element_size()

    def init(self) -> "CTCBeamState":
        """f5e_ctc_beam_state_init: every sequence back at the empty prefix (one small launch, no memset)."""
        require_device()
        check(lib().f5e_ctc_beam_state_init(_stream(), _p(self.buf, None, "state"), self.nbytes, self.B, self.T_cap,
                                            self.chunk_cap, self.beam), "f5e_ctc_beam_state_init")
        return self


def _beam_state_geometry(B: int, T_cap: int, chunk_cap: int, beam: int, name: str):
    B, T_cap, chunk_cap, beam = int(B), int(T_cap), int(chunk_cap), int(beam)
    if not 1 <= beam <= 16:
        raise _C.F5EError(f"{name}: beam must lie in 1..16, got {beam}")
    if not (1 <= B <= 65535 and 1 <= T_cap <= 1 << 20 and 1 <= chunk_cap <= 16384):
        raise _C.F5EError(f"{name}: need 1 <= B <= 65535, 1 <= T_cap <= 2^20 and 1 <= chunk_cap <= 16384 "
                          f"(got {B}, {T_cap}, {chunk_cap})")
    return B, T_cap, chunk_cap, beam


def ctc_beam_state_bytes(B: int, T_cap: int, chunk_cap: int, beam: int) -> int:
    """Bytes of the resumable search's state (host call)."""
    B, T_cap, chunk_cap, beam = _beam_state_geometry(B, T_cap, chunk_cap, beam, "ctc_beam_state_bytes")
    n = C.c_ulonglong()
    check(lib().f5e_ctc_beam_state_bytes(B, T_cap, chunk_cap, beam, C.byref(n)), "f5e_ctc_beam_state_bytes")
    return int(n.value)


def ctc_beam_state(B: int, T_cap: int, chunk_cap: int, beam: int, *, buf: Optional[Tensor] = None,
                   device="cuda") -> CTCBeamState:
    """An initialised state of ``ctc_beam_chunk`` for B sequences of up to T_cap frames in all, fed at most chunk_cap frames
    per call, at beam size ``beam``.  ``buf``: caller-owned device memory of at least ``ctc_beam_state_bytes`` bytes
    (allocated here when None)."""
    B, T_cap, chunk_cap, beam = _beam_state_geometry(B, T_cap, chunk_cap, beam, "ctc_beam_state")
    require_device()
    need = ctc_beam_state_bytes(B, T_cap, chunk_cap, beam)
    if buf is None:
        buf = torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
    if not buf.is_cuda or not buf.is_contiguous() or buf.numel() * buf.element_size() < need or buf.data_ptr() % 8:
        raise _C.F5EError(f"ctc_beam_state: buf must be contiguous, 8-byte aligned device memory of >= {need} bytes")
    return CTCBeamState(buf, B, T_cap, chunk_cap, beam).init()


def ctc_beam_chunk(scores: Tensor, n_frames: Tensor, state: CTCBeamState, blank: int = 0, *, want_result: bool = True,
                   ld_hyp: Optional[int] = None, hyp: Optional[Tensor] = None, hyp_len: Optional[Tensor] = None,
                   score: Optional[Tensor] = None):
    """One chunk of the resumable CTC prefix beam search (f5e_ctc_beam_chunk): scores f32 [B, T_chunk, V] as in
    ``ctc_beam_search``, n_frames i32 [B] on the device (the chunk's frames that belong to each sequence; 0 = idle) ->
    (hyp i32 [B, beam, ld_hyp], hyp_len i32 [B, beam], score f32 [B, beam]): the result on every frame fed so far, in the
    layout of ``ctc_beam_search`` and, after the last chunk, bit for bit what one ``ctc_beam_search`` call on all the frames
    returns.  ``want_result=False`` skips the readout and returns None.  ld_hyp defaults to ``state.T_cap``."""
    B, T, V = _ctc_scores(scores, "ctc_beam_chunk")
    if not isinstance(state, CTCBeamState):
        raise _C.F5EError("ctc_beam_chunk: state must come from ctc_beam_state")
    beam = state.beam
    if B != state.B or not 1 <= T <= state.chunk_cap:
        raise _C.F5EError(f"ctc_beam_chunk: scores [{B}, {T}, {V}] against a state for B = {state.B}, chunk_cap = "
                          f"{state.chunk_cap}: need the same B and 1 <= T_chunk <= chunk_cap")
    if n_frames.dtype != I32 or not n_frames.is_cuda or n_frames.numel() != B:
        raise _C.F5EError(f"ctc_beam_chunk: n_frames must be an i32 GPU tensor [{B}]")
    if beam > V or not 0 <= int(blank) < V:
        raise _C.F5EError(f"ctc_beam_chunk: need beam ({beam}) <= V ({V}) and 0 <= blank < V")
    require_device()
    dev = scores.device
    if want_result:
        if hyp is not None:
            if hyp.ndim != 3 or not hyp.is_contiguous():
                raise _C.F5EError(f"ctc_beam_chunk: hyp must be a contiguous i32 tensor [{B}, {beam}, ld_hyp]")
            ld_hyp = hyp.shape[2]
        ld_hyp = state.T_cap if ld_hyp is None else int(ld_hyp)
        hyp = torch.empty(B, beam, ld_hyp, dtype=I32, device=dev) if hyp is None else hyp
        hyp_len = torch.empty(B, beam, dtype=I32, device=dev) if hyp_len is None else hyp_len
        score = torch.empty(B, beam, dtype=F32, device=dev) if score is None else score
        if ld_hyp < 1 or hyp.shape != (B, beam, ld_hyp) or hyp_len.shape != (B, beam) or score.shape != (B, beam) or \
                not (hyp_len.is_contiguous() and score.is_contiguous()):
            raise _C.F5EError(f"ctc_beam_chunk: hyp [{B}, {beam}, ld_hyp >= 1], hyp_len / score [{B}, {beam}], contiguous")
    elif hyp is not None or hyp_len is not None or score is not None:
        raise _C.F5EError("ctc_beam_chunk: want_result=False takes no output tensors")
    else:
        ld_hyp = 0
    check(lib().f5e_ctc_beam_chunk(_stream(), C.c_void_p(scores.data_ptr()), scores.stride(0), _row_stride(scores, V),
                                   _p(n_frames, I32, "n_frames"),
                                   T, V, int(blank), beam, _p(state.buf, None, "state"), state.nbytes,
                                   _p(hyp, I32, "hyp"), ld_hyp, _p(hyp_len, I32, "hyp_len"), _p(score, F32, "score"),
                                   B, state.T_cap, state.chunk_cap), "f5e_ctc_beam_chunk")
    return (hyp, hyp_len, score) if want_result else None


def token_logp(logits: Tensor, target: Tensor, out: Optional[Tensor] = None):
    """out[r] = logits[r, target[r]] - logsumexp(logits[r]) (f5e_token_logp): logits f32 [rows, V] on the device (row stride
    free, unit class stride), target i32 [rows]; a negative target gives 0."""
    if logits.ndim != 2 or not logits.is_cuda or logits.dtype != F32 or logits.stride(1) != 1:
        raise _C.F5EError("token_logp: logits must be an f32 GPU tensor [rows, V] with unit class stride; there is no CPU "
                          "path")
    rows, V = logits.shape
    if target.dtype != I32 or not target.is_cuda or target.shape != (rows,) or not target.is_contiguous():
        raise _C.F5EError(f"token_logp: target must be a contiguous i32 GPU tensor [{rows}]")
    require_device()
    out = torch.empty(rows, dtype=F32, device=logits.device) if out is None else out
    if out.shape != (rows,) or not out.is_contiguous():
        raise _C.F5EError(f"token_logp: out must be a contiguous f32 tensor [{rows}]")
    check(lib().f5e_token_logp(_stream(), C.c_void_p(logits.data_ptr()), logits.stride(0) if rows > 1 else max(V, logits.stride(0)),
                               _p(target, I32, "target"), _p(out, F32, "out"), rows, V), "f5e_token_logp")
    return out


def log_softmax_rows(x: Tensor, out: Optional[Tensor] = None):
    """out[r] = x[r] - logsumexp(x[r]) (f5e_log_softmax_rows): x f32 [rows, V] on the device (row stride free, unit column
    stride); out likewise (allocated here when None; may be x)."""
    for n_, t_ in (("x", x), ("out", out)):
        if t_ is not None and (t_.ndim != 2 or not t_.is_cuda or t_.dtype != F32 or t_.stride(1) != 1):
            raise _C.F5EError(f"log_softmax_rows: {n_} must be an f32 GPU tensor [rows, V] with unit column stride; there is "
                              "no CPU path")
    rows, V = x.shape
    require_device()
    out = torch.empty(rows, V, dtype=F32, device=x.device) if out is None else out
    if out.shape != (rows, V):
        raise _C.F5EError(f"log_softmax_rows: out must be [{rows}, {V}]")
    ld = [t_.stride(0) if rows > 1 else max(V, t_.stride(0)) for t_ in (x, out)]
    check(lib().f5e_log_softmax_rows(_stream(), C.c_void_p(x.data_ptr()), ld[0], C.c_void_p(out.data_ptr()), ld[1], rows, V),
          "f5e_log_softmax_rows")
    return out


def attn_decode_f32(qkv: Tensor, kc: Tensor, vc: Tensor, p: int, heads: int, scale: float, anc: Optional[Tensor] = None,
                    out: Optional[Tensor] = None, begin: Optional[Tensor] = None):
    """Cached single-query self-attention of decode step ``p`` (f5e_attn_decode_f32): qkv f32 [R, >= 3 D] (q | k | v of the
    step), kc / vc f32 [R, Umax, D] views of the layer's caches (row and position strides free, unit channel stride, the same
    strides for both), anc i32 [R, >= p] or None -> out f32 [R, D].  Slot [r, p] of both caches receives the step's k / v;
    position j < p is read from cache row ``anc[r, j]`` (row r when None).  ``begin`` i32 [R] on the device (None: the launch
    as it always was): row r reads positions begin[r] .. p only (f5e_attn_decode_from_f32, the step after a left-padded
    prompt)."""
    if qkv.ndim != 2 or kc.ndim != 3 or kc.shape != vc.shape or kc.stride() != vc.stride():
        raise _C.F5EError("attn_decode_f32: qkv [R, >= 3 D] and kc, vc [R, Umax, D] with equal strides; there is no CPU path")
    R, Umax, D = kc.shape
    for t, nm in ((kc, "kc"), (vc, "vc")):
        if not t.is_cuda or t.dtype != F32 or t.stride(2) != 1:
            raise _C.F5EError(f"attn_decode_f32: {nm} must be an f32 GPU tensor with unit channel stride")
    if qkv.shape[0] != R or D % heads or not 0 <= int(p) < Umax:
        raise _C.F5EError(f"attn_decode_f32: qkv rows {qkv.shape[0]} != {R}, heads {heads} must divide {D}, 0 <= p < {Umax}")
    pos_stride = kc.stride(1) if Umax > 1 else max(D, kc.stride(1))
    row_stride = kc.stride(0) if R > 1 else max(kc.stride(0), (Umax - 1) * pos_stride + D)
    have = kc.untyped_storage().nbytes() // 4 - kc.storage_offset()
    if pos_stride < D or row_stride < (Umax - 1) * pos_stride + D or have < (R - 1) * row_stride + (Umax - 1) * pos_stride + D \
            or pos_stride % 4 or row_stride % 4 or kc.data_ptr() % 16:
        raise _C.F5EError(f"attn_decode_f32: cache strides ({row_stride}, {pos_stride}) must be multiples of 4 spanning "
                          f"[{R}, {Umax}, {D}] inside the storage, kc 16-byte aligned")
    qp, ldq = _rows(qkv, (F32,), "attn_decode_f32: qkv", 3 * D)
    ap, ld_anc = None, 0
    if anc is not None:
        if anc.ndim != 2 or anc.shape[0] != R:
            raise _C.F5EError(f"attn_decode_f32: anc must be an i32 GPU tensor [{R}, >= p]")
        ap, ld_anc = _rows(anc, (I32,), "attn_decode_f32: anc", max(int(p), 1), vec=1)
    require_device()
    out = torch.empty(R, D, dtype=F32, device=qkv.device) if out is None else out
    if out.shape != (R, D):
        raise _C.F5EError(f"attn_decode_f32: out must be [{R}, {D}]")
    op, ldo = _rows(out, (F32,), "attn_decode_f32: out", D, vec=1)
    if begin is not None:
        check(lib().f5e_attn_decode_from_f32(_stream(), qp, ldq, C.c_void_p(kc.data_ptr()), C.c_void_p(vc.data_ptr()), row_stride,
                                             pos_stride, ap, ld_anc, _vec(begin, I32, "attn_decode_f32: begin", (R,)), op, ldo, R,
                                             Umax, heads, D // heads, int(p), float(scale)), "f5e_attn_decode_from_f32")
        return out
    check(lib().f5e_attn_decode_f32(_stream(), qp, ldq, C.c_void_p(kc.data_ptr()), C.c_void_p(vc.data_ptr()), row_stride,
                                    pos_stride, ap, ld_anc, op, ldo, R, Umax, heads, D // heads, int(p), float(scale)),
          "f5e_attn_decode_f32")
    return out


def attn_prefill_f32(qkv: Tensor, kc: Tensor, vc: Tensor, U: int, heads: int, scale: float, begin: Optional[Tensor] = None,
                     out: Optional[Tensor] = None):
    """Causal self-attention of a prompt in one pass (f5e_attn_prefill_f32): qkv f32 [R * U, >= 3 D] (q | k | v of positions
    0 .. U - 1 of every row), kc / vc f32 [R, Umax, D] views of the layer's caches (the strides ``attn_decode_f32`` takes),
    begin i32 [R] on the device or None -> out f32 [R * U, D].  Query i of row r sees keys begin[r] .. i (a query below
    begin[r] yields zeros); slots [r, :U] of both caches receive the k / v columns of qkv, nothing else of them is written."""
    if qkv.ndim != 2 or kc.ndim != 3 or kc.shape != vc.shape or kc.stride() != vc.stride():
        raise _C.F5EError("attn_prefill_f32: qkv [R * U, >= 3 D] and kc, vc [R, Umax, D] with equal strides; there is no CPU path")
    R, Umax, D = kc.shape
    for t, nm in ((kc, "kc"), (vc, "vc")):
        if not t.is_cuda or t.dtype != F32 or t.stride(2) != 1:
            raise _C.F5EError(f"attn_prefill_f32: {nm} must be an f32 GPU tensor with unit channel stride")
    U = int(U)
    if not 1 <= U <= Umax or qkv.shape[0] != R * U or D % heads:
        raise _C.F5EError(f"attn_prefill_f32: need 1 <= U = {U} <= {Umax} cached positions, {R} * U = {qkv.shape[0]} rows of qkv "
                          f"and heads {heads} dividing {D}")
    pos_stride = kc.stride(1) if Umax > 1 else max(D, kc.stride(1))
    row_stride = kc.stride(0) if R > 1 else max(kc.stride(0), (Umax - 1) * pos_stride + D)
    for t in (kc, vc):
        have = t.untyped_storage().nbytes() // 4 - t.storage_offset()
        if pos_stride < D or row_stride < (Umax - 1) * pos_stride + D or have < (R - 1) * row_stride + (Umax - 1) * pos_stride + D \
                or pos_stride % 4 or row_stride % 4 or t.data_ptr() % 16:
            raise _C.F5EError(f"attn_prefill_f32: cache strides ({row_stride}, {pos_stride}) must be multiples of 4 spanning "
                              f"[{R}, {Umax}, {D}] inside the storage, kc and vc 16-byte aligned")
    qp, ldq = _rows(qkv, (F32,), "attn_prefill_f32: qkv", 3 * D)
    bp = None if begin is None else _vec(begin, I32, "attn_prefill_f32: begin", (R,))
    require_device()
    out = torch.empty(R * U, D, dtype=F32, device=qkv.device) if out is None else out
    if out.shape != (R * U, D):
        raise _C.F5EError(f"attn_prefill_f32: out must be [{R * U}, {D}]")
    op, ldo = _rows(out, (F32,), "attn_prefill_f32: out", D)
    check(lib().f5e_attn_prefill_f32(_stream(), qp, ldq, C.c_void_p(kc.data_ptr()), C.c_void_p(vc.data_ptr()), row_stride,
                                     pos_stride, bp, op, ldo, R, U, Umax, heads, D // heads, float(scale)), "f5e_attn_prefill_f32")
    return out


def attn_append_f32(qkv: Tensor, kc: Tensor, vc: Tensor, U: int, p0: int, heads: int, scale: float,
                    begin: Optional[Tensor] = None, out: Optional[Tensor] = None):
    """Causal self-attention of U new positions behind a cache (f5e_attn_append_f32): qkv f32 [R * U, >= 3 D] (q | k | v of
    positions p0 .. p0 + U - 1 of every row), kc / vc f32 [R, Umax, D] views of the layer's caches (the strides
    ``attn_prefill_f32`` takes), begin i32 [R] on the device or None -> out f32 [R * U, D].  Query u of row r sees the cached
    positions begin[r] .. p0 - 1 and the new ones 0 .. u (a query below begin[r] yields zeros); slots [r, p0:p0 + U] of both
    caches receive the k / v columns of qkv, nothing else of them is written and nothing at or beyond p0 is read."""
    if qkv.ndim != 2 or kc.ndim != 3 or kc.shape != vc.shape or kc.stride() != vc.stride():
        raise _C.F5EError("attn_append_f32: qkv [R * U, >= 3 D] and kc, vc [R, Umax, D] with equal strides; there is no CPU path")
    R, Umax, D = kc.shape
    for t, nm in ((kc, "kc"), (vc, "vc")):
        if not t.is_cuda or t.dtype != F32 or t.stride(2) != 1:
            raise _C.F5EError(f"attn_append_f32: {nm} must be an f32 GPU tensor with unit channel stride")
    U, p0 = int(U), int(p0)
    if U < 1 or p0 < 0 or p0 + U > Umax or qkv.shape[0] != R * U or D % heads:
        raise _C.F5EError(f"attn_append_f32: need U = {U} >= 1 new positions from p0 = {p0} >= 0 inside the {Umax} cached ones, "
                          f"{R} * U = {qkv.shape[0]} rows of qkv and heads {heads} dividing {D}")
    pos_stride = kc.stride(1) if Umax > 1 else max(D, kc.stride(1))
    row_stride = kc.stride(0) if R > 1 else max(kc.stride(0), (Umax - 1) * pos_stride + D)
    for t in (kc, vc):
        have = t.untyped_storage().nbytes() // 4 - t.storage_offset()
        if pos_stride < D or row_stride < (Umax - 1) * pos_stride + D or have < (R - 1) * row_stride + (Umax - 1) * pos_stride + D \
                or pos_stride % 4 or row_stride % 4 or t.data_ptr() % 16:
            raise _C.F5EError(f"attn_append_f32: cache strides ({row_stride}, {pos_stride}) must be multiples of 4 spanning "
                              f"[{R}, {Umax}, {D}] inside the storage, kc and vc 16-byte aligned")
    qp, ldq = _rows(qkv, (F32,), "attn_append_f32: qkv", 3 * D)
    bp = None if begin is None else _vec(begin, I32, "attn_append_f32: begin", (R,))
    require_device()
    out = torch.empty(R * U, D, dtype=F32, device=qkv.device) if out is None else out
    if out.shape != (R * U, D):
        raise _C.F5EError(f"attn_append_f32: out must be [{R * U}, {D}]")
    op, ldo = _rows(out, (F32,), "attn_append_f32: out", D)
    check(lib().f5e_attn_append_f32(_stream(), qp, ldq, C.c_void_p(kc.data_ptr()), C.c_void_p(vc.data_ptr()), row_stride,
                                    pos_stride, bp, op, ldo, R, U, Umax, heads, D // heads, p0, float(scale)), "f5e_attn_append_f32")
    return out


SKINNY_MAX_M = 16
_skinny_ws: dict = {}
_skinny_needs: dict = {}


def gemm_f32_skinny_workspace(N: int, K: int) -> int:
    """Scratch bytes of ``gemm_f32_skinny`` for an [N, K] weight (host arithmetic on N, K and the CU count; 0: K is not split)."""
    n = C.c_ulonglong(0)
    check(lib().f5e_gemm_f32_skinny_workspace(int(N), int(K), C.byref(n)), "f5e_gemm_f32_skinny_workspace")
    return int(n.value)


def gemm_f32_w16_skinny_workspace(N: int, K: int) -> int:
    """Scratch bytes of ``gemm_f32_w16_skinny`` (f5e_gemm_f32_w16_skinny_workspace): the K split, and so the answer, is
    ``gemm_f32_skinny``'s."""
    n = C.c_ulonglong(0)
    check(lib().f5e_gemm_f32_w16_skinny_workspace(int(N), int(K), C.byref(n)), "f5e_gemm_f32_w16_skinny_workspace")
    return int(n.value)


def _skinny_need(N: int, K: int, device) -> int:
    """``gemm_f32_skinny_workspace`` once per shape and device (the answer depends on the device's CU count)."""
    key = (N, K, device)
    if key not in _skinny_needs:
        _skinny_needs[key] = gemm_f32_skinny_workspace(N, K)
    return _skinny_needs[key]


def _gemm_skinny(op: str, w_dtypes, a, w, bias, out, act, addend, workspace):
    """``gemm_f32_skinny`` and ``gemm_f32_w16_skinny``: one set of checks, the entry point follows ``w.dtype``."""
    for t, nm in ((a, "a"), (w, "w"), (out, "out")) + (((addend, "addend"),) if addend is not None else ()):
        dts = w_dtypes if nm == "w" else (F32,)
        if not isinstance(t, Tensor) or t.ndim != 2 or not t.is_cuda or t.dtype not in dts or (t.stride(1) != 1 and t.shape[1] > 1):
            raise _C.F5EError(f"{op}: {nm} must be a 2-D {'f32' if dts == (F32,) else 'fp16 / bf16'} GPU tensor with unit column "
                              f"stride; there is no CPU path")
    (M, K), N = a.shape, w.shape[0]
    if not 1 <= M <= SKINNY_MAX_M:
        raise _C.F5EError(f"{op}: built for 1 <= M <= {SKINNY_MAX_M} rows (got {M}); gemm_f32 takes the rest")
    if N < 1 or K < 4 or K % 4 or w.shape[1] != K:
        raise _C.F5EError(f"{op}: a [{M}, {K}] against w {tuple(w.shape)}: K must be a positive multiple of 4 and equal")
    if act not in (ACT_NONE, ACT_GELU_ERF):
        raise _C.F5EError(f"{op}: act = {act} is not built (ACT_NONE and ACT_GELU_ERF are)")
    if out.shape[0] != M or out.shape[1] < N or (addend is not None and (addend.shape[0] != M or addend.shape[1] < N)):
        raise _C.F5EError(f"{op}: out and addend must be [{M}, >= {N}]")
    if bias is not None and bias.numel() < N:
        raise _C.F5EError(f"{op}: bias must hold at least {N} elements (got {bias.numel()})")
    ap, lda = _rows(a, (F32,), f"{op}: a", K)
    wp, ldw = _rows(w, w_dtypes, f"{op}: w", K)        # vec = 4: 16-byte (fp32) / 8-byte (16-bit) base, row stride % 4
    op_, ldo = _rows(out, (F32,), f"{op}: out", N, vec=1)
    dp, ldd = (None, 0) if addend is None else _rows(addend, (F32,), f"{op}: addend", N, vec=1)
    require_device()
    need = _skinny_need(N, K, a.device)
    if workspace is None and need:
        key = (a.device, _stream())                      # launches of one stream are ordered: they can share the scratch
        workspace = _skinny_ws.get(key)
        if workspace is None or workspace.numel() * 4 < need:
            workspace = _skinny_ws[key] = torch.empty(max(need, 1 << 20) // 4, dtype=F32, device=a.device)
    if need and (not workspace.is_cuda or not workspace.is_contiguous() or workspace.data_ptr() % 16 or
                 workspace.numel() * workspace.element_size() < need):
        raise _C.F5EError(f"{op}: workspace must be a contiguous 16-byte aligned GPU tensor of at least {need} bytes")
    tail = (_p(bias, F32, "bias"), int(act), dp, ldd, op_, ldo, C.c_void_p(workspace.data_ptr()) if need else None,
            workspace.numel() * workspace.element_size() if need else 0, M, N, K)
    if w.dtype == F32:
        check(lib().f5e_gemm_f32_skinny(_stream(), ap, lda, wp, ldw, *tail), "f5e_gemm_f32_skinny")
    else:
        check(lib().f5e_gemm_f32_w16_skinny(_stream(), ap, lda, wp, ldw, W16_TYPES[w.dtype], *tail), "f5e_gemm_f32_w16_skinny")
    return out


def gemm_f32_skinny(a: Tensor, w: Tensor, bias: Optional[Tensor] = None, *, out: Tensor, act: int = ACT_NONE,
                    addend: Optional[Tensor] = None, workspace: Optional[Tensor] = None):
    """out[m, n] = act(sum_k a[m, k] w[n, k] + bias[n]) + addend[m, n] for 1 <= M <= 16 rows (f5e_gemm_f32_skinny): the weight
    read of a verify pass spread over the whole chip.  a f32 [M, K] and w f32 [N, K] row-strided views (K and the row strides
    multiples of 4, 16-byte aligned), out / addend f32 [M, >= N] views with unit column stride (addend may be out), bias f32
    [>= N].  ``act``: ACT_NONE or ACT_GELU_ERF.  A row's result does not depend on M; two launches give the same bits.
    ``workspace``: a device tensor of ``gemm_f32_skinny_workspace`` bytes (None: one is kept per device and stream, whose
    launches are ordered)."""
    return _gemm_skinny("gemm_f32_skinny", (F32,), a, w, bias, out, act, addend, workspace)


def gemm_f32_w16_skinny(a: Tensor, w: Tensor, bias: Optional[Tensor] = None, *, out: Tensor, act: int = ACT_NONE,
                        addend: Optional[Tensor] = None, workspace: Optional[Tensor] = None):
    """``gemm_f32_skinny`` with a 16-bit weight (f5e_gemm_f32_w16_skinny): ``w`` fp16 or bf16 [N, K], 8-byte aligned, widened to
    fp32 in registers; everything else as there.  Bit-equal to ``gemm_f32_skinny(a, w.float(), ...)`` at half the bytes of
    ``w``, which is all a decode step reads."""
    return _gemm_skinny("gemm_f32_w16_skinny", tuple(W16_TYPES), a, w, bias, out, act, addend, workspace)


def _whisper_embed(op: str, emb_dtypes, ids, emb, pos, out, p0, begin):
    """``whisper_embed`` and ``whisper_embed_w16``: one set of checks, the entry point follows ``emb.dtype``."""
    if ids.ndim != 2 or emb.ndim != 2 or pos.ndim != 2 or out.ndim != 3:
        raise _C.F5EError(f"{op}: ids [R, U], emb [V, D], pos [P, D] and out [R, U, D]; there is no CPU path")
    (R, U), D = ids.shape, emb.shape[1]
    p0 = int(p0)
    if R < 1 or U < 1 or out.shape != (R, U, D) or pos.shape[1] != D or D % 4 or p0 < 0 or p0 + U > pos.shape[0]:
        raise _C.F5EError(f"{op}: ids {tuple(ids.shape)}, emb {tuple(emb.shape)}, pos {tuple(pos.shape)}, out "
                          f"{tuple(out.shape)}: out must be [R, U, D], D a multiple of 4, and positions {p0} .. {p0 + U - 1} "
                          f"inside the {pos.shape[0]} rows of pos")
    for t, nm in ((emb, "emb"), (pos, "pos"), (out, "out")):
        if t.is_cuda and t.data_ptr() % (8 if t.dtype in W16_TYPES else 16):
            raise _C.F5EError(f"{op}: {nm} must be 16-byte aligned (a 16-bit emb: 8-byte)")
    bp = None if begin is None else _vec(begin, I32, f"{op}: begin", (R,))
    if emb.dtype not in emb_dtypes:
        raise _C.F5EError(f"{op}: emb must be {'f32' if emb_dtypes == (F32,) else 'fp16 / bf16'} (got {emb.dtype})")
    front = (_p(ids, I32, f"{op}: ids"), bp, _p(emb, None, f"{op}: emb"))
    back = (_p(pos, F32, f"{op}: pos"), _p(out, F32, f"{op}: out"), R, U, D, p0, pos.shape[0], emb.shape[0])
    require_device()
    if emb.dtype == F32:
        check(lib().f5e_whisper_embed(_stream(), *front, *back), "f5e_whisper_embed")
    else:
        check(lib().f5e_whisper_embed_w16(_stream(), *front, W16_TYPES[emb.dtype], *back), "f5e_whisper_embed_w16")
    return out


def whisper_embed(ids: Tensor, emb: Tensor, pos: Tensor, out: Tensor, p0: int = 0, begin: Optional[Tensor] = None):
    """out[r, u] = emb[ids[r, u]] + pos[max(p0 + u - begin[r], 0)] (f5e_whisper_embed): ids i32 [R, U], emb f32 [V, D], pos f32
    [P, D], begin i32 [R] or None, out f32 [R, U, D], all contiguous on the device.  U = 1 with p0 = p feeds a decode step."""
    return _whisper_embed("whisper_embed", (F32,), ids, emb, pos, out, p0, begin)


def whisper_embed_w16(ids: Tensor, emb: Tensor, pos: Tensor, out: Tensor, p0: int = 0, begin: Optional[Tensor] = None):
    """``whisper_embed`` reading a 16-bit token table (f5e_whisper_embed_w16): emb fp16 or bf16 [V, D], 8-byte aligned; pos and
    out stay f32.  Bit-equal to ``whisper_embed(ids, emb.float(), ...)``."""
    return _whisper_embed("whisper_embed_w16", tuple(W16_TYPES), ids, emb, pos, out, p0, begin)


def beam_step(logits: Tensor, score: Tensor, hyp_in: Tensor, anc_in: Tensor, hyp_out: Tensor, anc_out: Tensor, last: Tensor,
              alive: Tensor, done_at: Tensor, p: int, beam: int, eos: int):
    """One step of the attention decoder's beam search (f5e_beam_step): logits f32 [B * beam, V] (raw; row stride free),
    score f32 [B * beam] (in / out), the hyp / anc table pairs i32 [B * beam, ld] (contiguous, in != out), last i32
    [B * beam], alive / done_at i32 [B]; all on the device.  See include/f5e_abi.h for the semantics."""
    if logits.ndim != 2 or not logits.is_cuda or logits.dtype != F32 or logits.stride(1) != 1:
        raise _C.F5EError("beam_step: logits must be an f32 GPU tensor [rows, V] with unit class stride; there is no CPU path")
    R, V = logits.shape
    beam, p = int(beam), int(p)
    if not 1 <= beam <= min(16, V) or R % beam:
        raise _C.F5EError(f"beam_step: beam must lie in 1..min(16, V = {V}) and divide the {R} rows, got {beam}")
    B = R // beam
    ld = hyp_in.shape[1] if hyp_in.ndim == 2 else 0
    for t, nm in ((hyp_in, "hyp_in"), (anc_in, "anc_in"), (hyp_out, "hyp_out"), (anc_out, "anc_out")):
        if t.shape != (R, ld) or not t.is_contiguous():
            raise _C.F5EError(f"beam_step: {nm} must be a contiguous i32 tensor [{R}, {ld}]")
    if not 0 <= p <= ld - 2:
        raise _C.F5EError(f"beam_step: step {p} needs tables of at least {p + 2} columns (got {ld})")
    if hyp_in.data_ptr() == hyp_out.data_ptr() or anc_in.data_ptr() == anc_out.data_ptr():
        raise _C.F5EError("beam_step: the tables are double-buffered: in and out must differ")
    if score.shape != (R,) or last.shape != (R,) or alive.shape != (B,) or done_at.shape != (B,):
        raise _C.F5EError(f"beam_step: score / last [{R}], alive / done_at [{B}]")
    if not 0 <= int(eos) < V:
        raise _C.F5EError(f"beam_step: eos must lie in [0, {V})")
    require_device()
    check(lib().f5e_beam_step(_stream(), C.c_void_p(logits.data_ptr()), logits.stride(0) if R > 1 else max(V, logits.stride(0)),
                              _p(score, F32, "score"), _p(hyp_in, I32, "hyp_in"), _p(anc_in, I32, "anc_in"),
                              _p(hyp_out, I32, "hyp_out"), _p(anc_out, I32, "anc_out"), ld, _p(last, I32, "last"),
                              _p(alive, I32, "alive"), _p(done_at, I32, "done_at"), B, V, beam, p, int(eos)), "f5e_beam_step")
    return hyp_out, anc_out


_resample_banks = {}
_resample_lock = threading.Lock()


def resample_bank(orig_freq: int, new_freq: int, device) -> Tensor:
    """The filter bank f32 [new, taps] of a conversion on ``device``: computed once per (orig, new) on the host
    (``infer.audio.sinc_resample_kernel``) and kept per device.  The first use uploads, so it must happen outside a graph
    capture."""
    from .infer import audio as A
    orig, new, _w, taps = A.resample_plan(orig_freq, new_freq)
    device = torch.device(device)
    key = (orig, new, device.type, device.index if device.index is not None else torch.cuda.current_device())
    bank = _resample_banks.get(key)
    if bank is None:
        bank = A.sinc_resample_kernel(orig, new)[0].reshape(new, taps).to(device).contiguous()
        with _resample_lock:
            bank = _resample_banks.setdefault(key, bank)
    return bank


def resample(x: Tensor, orig_freq: int, new_freq: int, out: Optional[Tensor] = None) -> Tensor:
    """Sample-rate conversion on the device (f5e_resample): x f32 [n] or [B, n] (row stride free, unit sample stride) at
    ``orig_freq`` -> [.., ceil(n * new / orig)] at ``new_freq``; ``out`` (optional) f32 [B, n_out] view with unit sample
    stride.  The same rate returns ``x`` itself."""
    if int(orig_freq) == int(new_freq):
        return x
    require_device()
    if not x.is_cuda or x.dtype != F32 or x.ndim not in (1, 2) or x.stride(-1) != 1 and x.shape[-1] > 1:
        raise _C.F5EError("resample: x must be an f32 GPU tensor [n] or [B, n] with unit sample stride; there is no CPU path")
    from .infer import audio as A
    orig, new, width, _taps = A.resample_plan(orig_freq, new_freq)
    x2 = x if x.ndim == 2 else x.unsqueeze(0)
    B, n = x2.shape
    n_out = -(-new * n // orig)
    if out is None:
        out = torch.empty(B, n_out, dtype=F32, device=x.device)
    o2 = out if out.ndim == 2 else out.unsqueeze(0)
    if not o2.is_cuda or o2.dtype != F32 or o2.ndim != 2 or o2.shape[0] != B or (o2.stride(1) != 1 and o2.shape[1] > 1):
        raise _C.F5EError(f"resample: out must be an f32 GPU tensor [{B}, n_out] with unit sample stride")
    ld_x = x2.stride(0) if B > 1 else max(n, 1)
    ld_y = o2.stride(0) if B > 1 else max(o2.shape[1], 1)
    bank = resample_bank(orig, new, x.device)
    # the library checks n >= 1 and n_out == ceil(new n / orig) (a mis-sized ``out`` is its BAD_SHAPE)
    check(lib().f5e_resample(_stream(), C.c_void_p(x2.data_ptr()), ld_x, _p(bank, F32, "bank"), orig, new, width,
                             C.c_void_p(o2.data_ptr()), ld_y, B, n, o2.shape[1]), "f5e_resample")
    return out if x.ndim == 2 else o2[0]


def _stft_operands(wav: Tensor, window: Tensor, twiddle: Tensor, out: Tensor, hop: int, n_mels: int, T: Optional[int],
                   name: str):
    """(wav pointer, nw, ldw, window pointer, twiddle pointer, out pointer, B) of the STFT log-mel entry points: wav f32
    [B, nw] with unit sample stride (any row stride), window f32 [1024], twiddle f32 [512, 2], out f32 contiguous and exactly
    [B, T, n_mels] (T = 1 + nw // hop unless given): the kernels write all of it and nothing else."""
    if wav.ndim != 2 or wav.dtype != F32 or not wav.is_cuda or min(wav.shape) < 1 or (wav.stride(1) != 1 and wav.shape[1] > 1):
        _err(f"{name}: wav must be an f32 [B, nw] GPU tensor with unit sample stride (got {wav.dtype}, {wav.device}, shape "
             f"{tuple(wav.shape)}, strides {tuple(wav.stride())})")
    B, nw = wav.shape
    hop = int(hop)
    if hop < 1:
        _err(f"{name}: hop must be positive (got {hop})")
    if B > 1 and wav.stride(0) < nw:
        _err(f"{name}: wav's row stride {wav.stride(0)} is smaller than its {nw} samples")
    T = 1 + nw // hop if T is None else int(T)
    wp, tp = _vec(window, F32, f"{name}: window", (1024,)), _vec(twiddle, F32, f"{name}: twiddle", (512, 2))
    op = _vec(out, F32, f"{name}: out", (B, T, n_mels))
    return C.c_void_p(wav.data_ptr()), nw, wav.stride(0) if B > 1 else nw, wp, tp, op, B


def _band_operands(fb_compact: Tensor, fb_band: Tensor, name: str):
    if fb_band.ndim != 2 or fb_band.shape[1] != 3 or fb_band.shape[0] < 1:
        _err(f"{name}: fb_band must be i32 [n_mels, 3] (got shape {tuple(fb_band.shape)})")
    if fb_compact.ndim != 1:
        _err(f"{name}: fb_compact must be f32 [nnz] (got shape {tuple(fb_compact.shape)})")
    return _p(fb_compact, F32, f"{name}: fb_compact"), _p(fb_band, I32, f"{name}: fb_band"), fb_compact.numel(), fb_band.shape[0]


def stft_logmel(wav: Tensor, window: Tensor, twiddle: Tensor, fb: Tensor, out: Tensor, n_fft: int, hop: int):
    """out f32 [B, 1 + nw // hop, n_mels] = log(clamp(|STFT(wav)| fb, 1e-5)), centred and reflect-padded; fb f32 [513, n_mels]
    contiguous.  Operands as ``_stft_operands``; everything is refused here or by the library, before any launch."""
    if fb.ndim != 2 or fb.shape[0] != 513 or fb.shape[1] < 1:
        _err(f"stft_logmel: fb must be f32 [513, n_mels] (got shape {tuple(fb.shape)})")
    require_device()
    wavp, nw, ldw, wp, tp, op, B = _stft_operands(wav, window, twiddle, out, hop, fb.shape[1], None, "stft_logmel")
    check(lib().f5e_stft_logmel(_stream(), wavp, nw, ldw, wp, tp, _p(fb, F32, "stft_logmel: fb"), op, B, n_fft, hop,
                                fb.shape[1]), "f5e_stft_logmel")
    return out


def band_filterbank(fb: Tensor):
    """Dense [n_freqs, n_mels] filterbank -> (compact weights f32 [nnz], band i32 [n_mels, 3] = lo, cnt, offset) on fb's
    device, or None when a filter has interior zeros / the total exceeds the kernel's LDS table (dense kernel then)."""
    h = fb.detach().to("cpu", F32)
    nz = h != 0
    bands, chunks, off = [], [], 0
    for m in range(h.shape[1]):
        idx = torch.nonzero(nz[:, m]).flatten()
        if idx.numel() == 0:
            bands.append((0, 0, off))
            continue
        lo, hi = int(idx[0]), int(idx[-1])
        bands.append((lo, hi - lo + 1, off))       # interior zeros (if any) stay in the run: they add +0 like the dense loop
        chunks.append(h[lo:hi + 1, m])
        off += hi - lo + 1
    if off == 0 or off > 2048:
        return None
    return torch.cat(chunks).contiguous().to(fb.device), torch.tensor(bands, dtype=I32).contiguous().to(fb.device)


def stft_logmel_banded(wav: Tensor, window: Tensor, twiddle: Tensor, fb_compact: Tensor, fb_band: Tensor, out: Tensor,
                       n_fft: int, hop: int):
    """``stft_logmel`` with the filterbank in ``band_filterbank``'s form (fb_compact f32 [nnz <= 2048], fb_band i32
    [n_mels, 3]): the same result bit for bit."""
    fcp, fbp, nnz, n_mels = _band_operands(fb_compact, fb_band, "stft_logmel_banded")
    require_device()
    wavp, nw, ldw, wp, tp, op, B = _stft_operands(wav, window, twiddle, out, hop, n_mels, None, "stft_logmel_banded")
    check(lib().f5e_stft_logmel_banded(_stream(), wavp, nw, ldw, wp, tp, fcp, fbp, nnz, op, B, n_fft, hop, n_mels),
          "f5e_stft_logmel_banded")
    return out


def stft_logmel_banded_ex(wav: Tensor, window: Tensor, twiddle: Tensor, fb_compact: Tensor, fb_band: Tensor, out: Tensor,
                          n_fft: int, hop: int, pad_left: int, mag_eps: float):
    """out f32 [B, T, n_mels]: frames start pad_left samples before f * hop (reflect-padded); T = out.shape[1]."""
    fcp, fbp, nnz, n_mels = _band_operands(fb_compact, fb_band, "stft_logmel_banded_ex")
    if out.ndim != 3:
        _err(f"stft_logmel_banded_ex: out must be [B, T, n_mels] (got shape {tuple(out.shape)})")
    require_device()
    T = out.shape[1]
    wavp, nw, ldw, wp, tp, op, B = _stft_operands(wav, window, twiddle, out, hop, n_mels, T, "stft_logmel_banded_ex")
    check(lib().f5e_stft_logmel_banded_ex(_stream(), wavp, nw, ldw, wp, tp, fcp, fbp, nnz, op, B, n_fft, hop, n_mels,
                                          int(pad_left), T, mag_eps), "f5e_stft_logmel_banded_ex")
    return out


def istft_head(z: Tensor, window: Tensor, twiddle: Tensor, frames_ws: Tensor, out: Tensor, B: int, T: int, n_fft: int,
               hop: int):
    """Vocos ISTFTHead tail: z f32 [B * T, >= 1026] view (513 log-magnitudes | 513 phases; unit column stride, any row stride
    >= 1026), frames_ws f32 scratch of at least B * T * 1024 elements, out f32 [B, hop (T - 1)] contiguous.  Everything is
    refused here or by the library (hop must divide 1024 and be at most 512), before any launch."""
    B, T, hop = int(B), int(T), int(hop)
    if B < 1 or T < 2 or hop < 1:
        _err(f"istft_head: needs B >= 1, T >= 2 and hop >= 1 (got {B}, {T}, {hop})")
    if z.ndim != 2 or z.shape[0] != B * T:
        _err(f"istft_head: z must have B * T = {B * T} rows (got shape {tuple(z.shape)})")
    require_device()
    zp, ldz = _rows(z, (F32,), "istft_head: z", 1026, vec=1)
    wp, tp = _vec(window, F32, "istft_head: window", (1024,)), _vec(twiddle, F32, "istft_head: twiddle", (512, 2))
    check(lib().f5e_istft_head(_stream(), zp, ldz, wp, tp, _flat(frames_ws, F32, "istft_head: frames_ws", B * T * 1024),
                               _vec(out, F32, "istft_head: out", (B, hop * (T - 1))), B, T, n_fft, hop), "f5e_istft_head")
    return out


def bigvgan_act(x: Tensor, out: Tensor, alpha: Tensor, inv_beta: Tensor, f_up: Tensor, f_dn: Tensor):
    """Activation1d: x f32 [B, L, C] -> out [B, L, C] (bf16 conv operand, or f32)."""
    require_device()
    B, L, C = x.shape
    if out.shape != x.shape or out.dtype not in (BF, F32):
        raise _C.F5EError("bigvgan_act: out must be bf16 or f32 of x's shape")
    if alpha.numel() != C or inv_beta.numel() != C or f_up.numel() != 12 or f_dn.numel() != 12:
        raise _C.F5EError("bigvgan_act: alpha / inv_beta [C], filters [12]")
    check(lib().f5e_bigvgan_act(_stream(), _p(x, F32, "x"), _p(out, None, "out"), 1 if out.dtype == F32 else 0,
                                _p(alpha, F32, "alpha"), _p(inv_beta, F32, "inv_beta"), _p(f_up, F32, "f_up"),
                                _p(f_dn, F32, "f_dn"), B, L, C), "f5e_bigvgan_act")
    return out


def bigvgan_conv(x: Tensor, w_packed: Tensor, bias: Optional[Tensor], N: int, ksz: int, dil: int, pad: int, *,
                 out: Optional[Tensor] = None, resid: Optional[Tensor] = None, sum_: Optional[Tensor] = None,
                 sum_scale: float = 1.0, sum_init: bool = False):
    """Conv1d on bf16 operands, x bf16 [B, L, Cin] -> f32 [B, L, N] (see f5e_bigvgan_conv); w_packed bf16
    [roundup(N, 64), ksz * Cin_pad] from vocoder_bigvgan.pack_conv_weight."""
    require_device()
    B, L, Cin = x.shape
    cin_pad = w_packed.shape[1] // ksz
    if w_packed.dtype != BF or w_packed.shape != ((N + 63) // 64 * 64, ksz * cin_pad) or cin_pad < Cin:
        raise _C.F5EError(f"bigvgan_conv: w_packed must be bf16 [{(N + 63) // 64 * 64}, {ksz} * Cin_pad] "
                          f"(got {w_packed.dtype} {tuple(w_packed.shape)})")
    for name, t in (("out", out), ("resid", resid), ("sum", sum_)):
        if t is not None and t.shape != (B, L, N):
            raise _C.F5EError(f"bigvgan_conv: {name} must be [{B}, {L}, {N}] (got {tuple(t.shape)})")
    if bias is not None and bias.numel() != N:
        raise _C.F5EError("bigvgan_conv: bias must have N elements")
    check(lib().f5e_bigvgan_conv(_stream(), _p(x, BF, "x"), _p(w_packed, BF, "w_packed"), _p(bias, F32, "bias"),
                                 _p(resid, F32, "resid"), _p(out, F32, "out"), _p(sum_, F32, "sum"), sum_scale,
                                 1 if sum_init else 0, B, L, Cin, cin_pad, N, ksz, dil, pad), "f5e_bigvgan_conv")
    return out if out is not None else sum_


def bigvgan_post(a: Tensor, w: Tensor, bias: Optional[Tensor], out: Tensor, use_tanh: bool):
    """conv_post: a f32 [B, L, C], w f32 [ksz, C] -> out f32 [B, L] = clamp(conv + bias, -1, 1) (or tanh)."""
    require_device()
    B, L, C = a.shape
    if w.shape[1] != C or out.shape != (B, L):
        raise _C.F5EError("bigvgan_post: w [ksz, C], out [B, L]")
    check(lib().f5e_bigvgan_post(_stream(), _p(a, F32, "a"), _p(w, F32, "w"), _p(bias, F32, "bias"), _p(out, F32, "out"),
                                 B, L, C, w.shape[0], 1 if use_tanh else 0), "f5e_bigvgan_post")
    return out


def kaldi_fbank(wav: Tensor, window: Tensor, twiddle: Tensor, fb: Tensor, out: Tensor, win: int, shift: int,
                in_scale: float = 32768.0, preemph: float = 0.97, eps: float = 1.1920928955078125e-07):
    require_device()
    B, nw = wav.shape
    check(lib().f5e_kaldi_fbank(_stream(), _p(wav, F32, "wav"), nw, wav.stride(0), _p(window, F32, "window"),
                                _p(twiddle, F32, "twiddle"), _p(fb, F32, "fb"), _p(out, F32, "out"), B, win, shift,
                                fb.shape[1], in_scale, preemph, eps), "f5e_kaldi_fbank")
    return out


def glu(x: Tensor, out: Tensor):
    """out[r, c] = x[r, c] * sigmoid(x[r, C + c]); x f32 [rows, 2C], out f32 [rows, C]: views with unit column stride and any
    row stride that is a multiple of 4, on a 16-byte aligned base (16-byte accesses)."""
    require_device()
    if out.ndim != 2 or x.shape != (out.shape[0], 2 * out.shape[1]):
        raise _C.F5EError(f"glu: x [rows, 2C], out [rows, C] (got {tuple(x.shape)}, {tuple(out.shape)})")
    rows, Cc = out.shape
    (xp, ldx), (op, ldo) = _rows(x, (F32,), "x", 2 * Cc), _rows(out, (F32,), "out", Cc)
    check(lib().f5e_glu(_stream(), xp, ldx, op, ldo, rows, Cc), "f5e_glu")
    return out


def dwconv(x: Tensor, w_t: Tensor, bias: Tensor, out: Tensor, keep: Optional[Tensor] = None):
    """Depthwise conv over time, channels-last f32 [B, T, C]; w_t [K, C]."""
    require_device()
    B, T, Cc = x.shape
    check(lib().f5e_dwconv(_stream(), _p(x, F32, "x"), _p(w_t, F32, "w_t"), _p(bias, F32, "bias"), _p(keep, F32, "keep"),
                           _p(out, F32, "out"), B, T, Cc, w_t.shape[0]), "f5e_dwconv")
    return out


def softmax_rows(x: Tensor, out: Tensor, L: int, scale: float, kv_len: Optional[Tensor] = None, rows_per_seq: int = 1):
    """Row softmax of scale * x[:, :len], len = min(kv_len[row // rows_per_seq], L) (L without kv_len); x, out f32
    [rows, >= L] views with unit column stride and any row stride (scalar accesses: no alignment beyond the element's).
    Every column of ``out`` from len up to its ROW STRIDE is set to zero (the pad columns a following GEMM reads), so
    ``out`` must own whole rows of its stride.  out may be x."""
    require_device()
    if x.ndim != 2 or out.ndim != 2 or out.shape[0] != x.shape[0] or L < 1:
        raise _C.F5EError(f"softmax_rows: x, out [rows, >= L] (got {tuple(x.shape)}, {tuple(out.shape)}, L={L})")
    rows = x.shape[0]
    if kv_len is not None and (rows_per_seq < 1 or kv_len.numel() < -(-rows // rows_per_seq)):
        raise _C.F5EError(f"softmax_rows: kv_len needs one entry per sequence of {rows_per_seq} rows")
    (xp, ldx), (op, ldo) = _rows(x, (F32,), "x", L, vec=1), _rows(out, (F32,), "out", L, vec=1, whole_rows=True)
    check(lib().f5e_softmax_rows(_stream(), xp, ldx, op, ldo,
                                 _p(kv_len, I32, "kv_len"), rows, rows_per_seq if kv_len is not None else max(rows, 1), L,
                                 scale), "f5e_softmax_rows")
    return out


def dwconv_stream(x: Tensor, w_t: Tensor, bias: Tensor, out: Tensor, causal: bool = False, chunk: int = 0,
                  fill: Optional[Tensor] = None):
    """Depthwise conv over time of the streaming conformer, channels-last f32 [B, T, C]; w_t [K, C].  causal False: taps
    that stay inside the frame's chunk (chunk <= 0: the whole sequence); causal True: taps t-(K-1)..t, positions before
    the sequence read the per-channel constant ``fill`` [C] (None: 0)."""
    require_device()
    B, T, Cc = x.shape
    check(lib().f5e_dwconv_stream(_stream(), _p(x, F32, "x"), _p(w_t, F32, "w_t"), _p(bias, F32, "bias"),
                                  _p(fill, F32, "fill"), _p(out, F32, "out"), B, T, Cc, w_t.shape[0], int(bool(causal)),
                                  int(chunk)), "f5e_dwconv_stream")
    return out


def relpos_attn(qu: Tensor, k: Tensor, pos: Tensor, v: Tensor, out: Tensor, heads: int, scale: float, B: int = 1,
                kv_len: Optional[Tensor] = None, chunk: int = 0, left_chunks: int = -1, q_begin: int = 0):
    """Fused relative-position attention with an optional chunk band (f5e_abi.h): qu f32 [B*T, 2D] (q+u | q+v), k / v / out
    f32 [B*T, D], pos f32 [>= T, D] indexed by the key; chunk <= 0: full context, left_chunks < 0: all left chunks."""
    require_device()
    M, D = out.shape
    T = M // B
    if M != B * T or qu.shape != (M, 2 * D) or k.shape != (M, D) or v.shape != (M, D) or pos.shape[0] < T or \
            pos.shape[1] != D or D % heads:
        raise _C.F5EError(f"relpos_attn: inconsistent shapes qu {tuple(qu.shape)} k {tuple(k.shape)} pos {tuple(pos.shape)} "
                          f"v {tuple(v.shape)} out {tuple(out.shape)} B={B} heads={heads}")
    for n_, t_ in (("qu", qu), ("k", k), ("pos", pos), ("v", v), ("out", out)):
        if t_.stride(1) != 1:
            raise _C.F5EError(f"relpos_attn: {n_} must have unit column stride")
    if kv_len is not None and kv_len.numel() != B:
        raise _C.F5EError("relpos_attn: kv_len needs one entry per sequence")
    check(lib().f5e_relpos_attn(_stream(), _p(qu, F32, "qu"), qu.stride(0), _p(k, F32, "k"), k.stride(0),
                                _p(pos, F32, "pos"), pos.stride(0), _p(v, F32, "v"), v.stride(0), _p(out, F32, "out"),
                                out.stride(0), _p(kv_len, I32, "kv_len"), B, T, heads, D // heads, int(q_begin), int(chunk),
                                int(left_chunks), float(scale)), "f5e_relpos_attn")
    return out


def mha_f32(q: Tensor, k: Tensor, v: Tensor, heads: int, scale: float, B: int = 1, kv_len: Optional[Tensor] = None,
            causal: bool = False, out: Optional[Tensor] = None):
    """Plain masked fp32 attention (f5e_mha_f32): q f32 [B*Tq, D], k / v f32 [B*Tk, D] on the device (row strides free, unit
    column stride) -> out f32 [B*Tq, D].  Key j is visible to query i iff j < kv_len[b] (i32 [B] on the device, optional) and,
    when ``causal`` (Tq == Tk), j <= i; a query with no visible key yields zeros."""
    if q.ndim != 2 or k.ndim != 2:
        raise _C.F5EError("mha_f32: q and k must be f32 GPU matrices; there is no CPU path")
    Mq, D = q.shape
    Mk = k.shape[0]
    if B < 1 or Mq % B or Mk % B or Mq == 0 or Mk == 0 or k.shape != (Mk, D) or v.shape != (Mk, D) or D % heads or \
            (out is not None and out.shape != (Mq, D)):
        raise _C.F5EError(f"mha_f32: inconsistent shapes q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)} B={B} "
                          f"heads={heads}")
    Tq, Tk = Mq // B, Mk // B
    if causal and Tq != Tk:
        raise _C.F5EError(f"mha_f32: causal needs Tq == Tk (got {Tq} and {Tk})")
    if kv_len is not None and (kv_len.numel() != B or kv_len.dtype != I32 or not kv_len.is_cuda):
        raise _C.F5EError(f"mha_f32: kv_len must be an i32 GPU tensor [{B}]")
    (qp, ldq), (kp, ldk), (vp, ldv) = _rows(q, (F32,), "mha_f32: q", D), _rows(k, (F32,), "mha_f32: k", D), \
        _rows(v, (F32,), "mha_f32: v", D, vec=1)
    require_device()
    out = torch.empty(Mq, D, dtype=F32, device=q.device) if out is None else out
    op, ldo = _rows(out, (F32,), "mha_f32: out", D)
    check(lib().f5e_mha_f32(_stream(), qp, ldq, kp, ldk, vp, ldv, op, ldo, _p(kv_len, I32, "kv_len"), B, Tq, Tk, heads,
                            D // heads, 1 if causal else 0, float(scale)), "f5e_mha_f32")
    return out


# ---- ECAPA-TDNN speaker encoder (csrc/ecapa.hip) ----

RES2_TILE = 16   # output frames per workgroup of f5e_res2_dconv (RES2_TT of csrc/ecapa.hip)


def _btc(t: Tensor, name: str, vec: int = 4):
    """(pointer, row stride, B, T, C) of a channels-last f32 [B, T, C] view whose frames are evenly spaced over the whole
    batch (stride(0) == T * stride(1)): a contiguous tensor or a column slice of one."""
    if t.ndim != 3 or min(t.shape) < 1:
        raise _C.F5EError(f"{name} must be a non-empty [B, T, C] tensor (got shape {tuple(t.shape)})")
    B, T, Cc = t.shape
    ld = t.stride(1) if T > 1 else (t.stride(0) if B > 1 else Cc)   # the stride of a size-1 dimension is arbitrary
    if (Cc > 1 and t.stride(2) != 1) or (B > 1 and t.stride(0) != T * ld):
        raise _C.F5EError(f"{name}: need unit channel stride and evenly spaced frames (strides {tuple(t.stride())})")
    p, ld = _rows(t.as_strided((B * T, Cc), (ld, 1)), (F32,), name, Cc, vec=vec)
    return p, ld, B, T, Cc


def _len(length: Optional[Tensor], B: int, name: str):
    if length is None:
        return None
    if not length.is_cuda or length.dtype != I32 or length.shape != (B,):
        raise _C.F5EError(f"{name}: lengths must be an i32 GPU tensor [{B}] (got {length.dtype} {tuple(length.shape)} on "
                          f"{length.device})")
    return _p(length, I32, "lengths")


def layer_mix_inorm(hs: Tensor, feature_weight: Tensor, lengths: Optional[Tensor], x: Tensor, mask: Tensor):
    """f5e_layer_mix_inorm: hs f32 [L, B, T, F] -> x f32 [B, T, F] (softmax-weighted layer mix + 1e-6, instance norm over
    t < lengths[b], zero beyond) and mask f32 [B, T] (1 where t < lengths[b])."""
    if hs.ndim != 4:
        raise _C.F5EError(f"layer_mix_inorm: hs must be [L, B, T, F] (got {tuple(hs.shape)})")
    L, B, T, F = hs.shape
    if feature_weight.shape != (L,) or x.shape != (B, T, F) or mask.shape != (B, T):
        raise _C.F5EError(f"layer_mix_inorm: feature_weight [{L}], x [{B}, {T}, {F}], mask [{B}, {T}] (got "
                          f"{tuple(feature_weight.shape)}, {tuple(x.shape)}, {tuple(mask.shape)})")
    require_device()
    check(lib().f5e_layer_mix_inorm(_stream(), _p(hs, F32, "hs"), _p(feature_weight, F32, "feature_weight"),
                                    _len(lengths, B, "layer_mix_inorm"), _p(x, F32, "x"), _p(mask, F32, "mask"),
                                    L, B, T, F), "f5e_layer_mix_inorm")
    return x, mask


def res2_dconv(x: Tensor, y: Tensor, w_packed: Tensor, bias: Tensor, bn_scale: Tensor, bn_shift: Tensor,
               lengths: Optional[Tensor], dilation: int, first: int = 0, count: int = 7):
    """f5e_res2_dconv: steps [first, first + count) of the Res2 chain on x f32 [B, T, 8 w] -> y (same shape, no aliasing);
    w_packed f32 [7, w, 3 w] (k = tap * w + ic), bias / bn_scale / bn_shift f32 [7, w]."""
    xp, ldx, B, T, Cc = _btc(x, "res2_dconv: x", vec=1)
    yp, ldy, By, Ty, Cy = _btc(y, "res2_dconv: y", vec=1)
    w = Cc // 8
    if (By, Ty, Cy) != (B, T, Cc) or w_packed.shape != (7, w, 3 * w) or any(t.shape != (7, w) for t in (bias, bn_scale, bn_shift)):
        raise _C.F5EError(f"res2_dconv: y like x {tuple(x.shape)}, w_packed [7, {w}, {3 * w}], bias / bn_scale / bn_shift "
                          f"[7, {w}]")
    require_device()
    check(lib().f5e_res2_dconv(_stream(), xp, ldx, yp, ldy, _p(w_packed, F32, "w_packed"), _p(bias, F32, "bias"),
                               _p(bn_scale, F32, "bn_scale"), _p(bn_shift, F32, "bn_shift"),
                               _len(lengths, B, "res2_dconv"), B, T, Cc, int(dilation), int(first), int(count)),
          "f5e_res2_dconv")
    return y


def time_stats(x: Tensor, lengths: Optional[Tensor], mean: Tensor, std: Optional[Tensor] = None):
    """f5e_time_stats: mean over t < lengths[b] of x f32 [B, T, C] -> mean f32 [B, C]; std (optional, same row stride as
    mean) = sqrt(unbiased variance + 1e-10).  mean / std may be column slices of one [B, >= C] buffer."""
    xp, ldx, B, T, Cc = _btc(x, "time_stats: x")
    mp, ldm = _rows(mean, (F32,), "time_stats: mean", Cc)
    sp = None
    if std is not None:
        sp, lds = _rows(std, (F32,), "time_stats: std", Cc)
        if lds != ldm or std.shape[0] != B:
            raise _C.F5EError("time_stats: std must share mean's row stride and row count")
    if mean.shape[0] != B:
        raise _C.F5EError(f"time_stats: mean must have {B} rows")
    require_device()
    check(lib().f5e_time_stats(_stream(), xp, ldx, _len(lengths, B, "time_stats"), mp, sp, ldm, B, T, Cc), "f5e_time_stats")
    return mean, std


def se_scale(x: Tensor, gate: Tensor, resid: Tensor, out: Tensor):
    """f5e_se_scale: out = x * sigmoid(gate[b]) + resid; x / resid / out f32 [B, T, C] views, gate f32 [B, C] logits."""
    xp, ldx, B, T, Cc = _btc(x, "se_scale: x")
    rp, ldr, *rs = _btc(resid, "se_scale: resid")
    op, ldo, *os_ = _btc(out, "se_scale: out")
    if rs != [B, T, Cc] or os_ != [B, T, Cc] or gate.shape != (B, Cc):
        raise _C.F5EError(f"se_scale: resid / out like x {tuple(x.shape)}, gate [{B}, {Cc}]")
    require_device()
    check(lib().f5e_se_scale(_stream(), xp, ldx, _p(gate, F32, "gate"), rp, ldr, op, ldo, B, T, Cc), "f5e_se_scale")
    return out


def bias_tanh(x: Tensor, add: Tensor):
    """f5e_bias_tanh: x f32 [B, T, N] <- tanh(x + add[b]) in place; add f32 [1, N] or [B, N]."""
    xp, ldx, B, T, N = _btc(x, "bias_tanh: x", vec=1)
    ap, lda = _rows(add, (F32,), "bias_tanh: add", N, vec=1)
    if add.shape[0] not in (1, B):
        raise _C.F5EError(f"bias_tanh: add must have 1 or {B} rows")
    require_device()
    check(lib().f5e_bias_tanh(_stream(), xp, ldx, ap, lda, add.shape[0], B, T, N), "f5e_bias_tanh")
    return x


def attn_stats_pool(x: Tensor, logits: Tensor, lengths: Optional[Tensor], out: Tensor):
    """f5e_attn_stats_pool: x, logits f32 [B, T, C] -> out f32 [B, 2 C] = [weighted mean | weighted std], the weights being
    the softmax of the logits over t < lengths[b]."""
    xp, ldx, B, T, Cc = _btc(x, "attn_stats_pool: x")
    lp, ldl, *ls = _btc(logits, "attn_stats_pool: logits")
    if ls != [B, T, Cc] or out.shape != (B, 2 * Cc):
        raise _C.F5EError(f"attn_stats_pool: logits like x {tuple(x.shape)}, out [{B}, {2 * Cc}]")
    require_device()
    check(lib().f5e_attn_stats_pool(_stream(), xp, ldx, lp, ldl, _len(lengths, B, "attn_stats_pool"), _p(out, F32, "out"),
                                    B, T, Cc), "f5e_attn_stats_pool")
    return out


# ---- WavLM upstream (csrc/wavlm.hip, f5e_relbias_attn_f32 of csrc/ppg_attention.hip) ----

def wav_norm_partials(B: int, S: int) -> int:
    """Floats of scratch that ``wav_norm`` needs for B rows of S samples (host arithmetic)."""
    n = C.c_ulonglong(0)
    check(lib().f5e_wav_norm_partials(int(B), int(S), C.byref(n)), "f5e_wav_norm_partials")
    return int(n.value)


def wav_norm(wav: Tensor, lengths: Optional[Tensor], out: Tensor, partials: Tensor, frames: Optional[Tensor] = None,
             mask: Optional[Tensor] = None, conv_kernels=(), conv_strides=()):
    """f5e_wav_norm: wav f32 [B, S] -> out f32 [B, S] normalised over each row's first lengths[b] samples, zero beyond;
    frames i32 [B] = frame count after the valid convolutions (conv_kernels, conv_strides); mask f32 [B, Tm] = t < frames[b]."""
    if wav.ndim != 2 or out.shape != wav.shape:
        raise _C.F5EError(f"wav_norm: wav and out must be [B, S] of one shape (got {tuple(wav.shape)}, {tuple(out.shape)})")
    B, S = wav.shape
    wp, ldw = _rows(wav, (F32,), "wav_norm: wav", S, vec=1)
    op, ldo = _rows(out, (F32,), "wav_norm: out", S, vec=1)
    if len(conv_kernels) != len(conv_strides) or len(conv_kernels) > 8:
        raise _C.F5EError("wav_norm: conv_kernels and conv_strides must have one length, at most 8")
    if partials.dtype != F32 or partials.numel() < wav_norm_partials(B, S):
        raise _C.F5EError(f"wav_norm: partials must hold {wav_norm_partials(B, S)} floats (wav_norm_partials)")
    if frames is not None and (frames.dtype != I32 or frames.shape != (B,)):
        raise _C.F5EError(f"wav_norm: frames must be i32 [{B}]")
    t_mask = 0
    if mask is not None:
        if mask.ndim != 2 or mask.shape[0] != B or not 0 < mask.shape[1] <= S:
            raise _C.F5EError(f"wav_norm: mask must be [{B}, 1..{S}] (got {tuple(mask.shape)})")
        t_mask = mask.shape[1]
    n = len(conv_kernels)
    ks, ss = (C.c_int * max(n, 1))(*[int(v) for v in conv_kernels]), (C.c_int * max(n, 1))(*[int(v) for v in conv_strides])
    require_device()
    check(lib().f5e_wav_norm(_stream(), wp, ldw, _len(lengths, B, "wav_norm"), op, ldo, _p(partials, F32, "partials"),
                             _p(frames, I32, "frames"), _p(mask, F32, "mask"), t_mask, ks, ss, n, B, S), "f5e_wav_norm")
    return out


def wavlm_conv0(wav: Tensor, w: Tensor, bias: Optional[Tensor], gamma: Tensor, beta: Tensor, out: Tensor, T0: Optional[int] = None):
    """f5e_wavlm_conv0: wav f32 [B, S], w f32 [C, 10] -> out f32 [B, P >= T0, C] (frames C floats apart, rows any stride >= T0 C):
    Conv1d(1 -> C, k 10, stride 5) + LayerNorm(C) + GELU in one pass; T0 defaults to (S - 10) // 5 + 1."""
    if wav.ndim != 2 or w.ndim != 2 or w.shape[1] != 10 or out.ndim != 3 or out.shape[0] != wav.shape[0] or out.shape[2] != w.shape[0]:
        raise _C.F5EError(f"wavlm_conv0: wav [B, S], w [C, 10], out [B, P, C] (got {tuple(wav.shape)}, {tuple(w.shape)}, {tuple(out.shape)})")
    B, S = wav.shape
    Cc = w.shape[0]
    T0 = (S - 10) // 5 + 1 if T0 is None else int(T0)
    if S < 10 or not 0 < T0 <= min((S - 10) // 5 + 1, out.shape[1]):
        raise _C.F5EError(f"wavlm_conv0: T0 = {T0} frames do not fit S = {S} samples / out {tuple(out.shape)}")
    if not out.is_cuda or out.dtype != F32 or out.stride(2) != 1 or (out.shape[1] > 1 and out.stride(1) != Cc):
        raise _C.F5EError("wavlm_conv0: out must be an f32 GPU tensor whose frames are C floats apart")
    bstride = out.stride(0) if B > 1 else max(out.stride(0), T0 * Cc)
    wp, ldw = _rows(wav, (F32,), "wavlm_conv0: wav", S, vec=1)
    for t, nm in ((bias, "bias"), (gamma, "gamma"), (beta, "beta")):
        if t is not None and t.numel() != Cc:
            raise _C.F5EError(f"wavlm_conv0: {nm} must have C = {Cc} elements")
    require_device()
    check(lib().f5e_wavlm_conv0(_stream(), wp, ldw, _p(w, F32, "w"), _p(bias, F32, "bias"), _p(gamma, F32, "gamma"),
                                _p(beta, F32, "beta"), C.c_void_p(out.data_ptr()), bstride, B, S, T0, Cc), "f5e_wavlm_conv0")
    return out


def layernorm_gelu(x: Tensor, out: Tensor, gamma: Tensor, beta: Tensor, eps: float = 1e-5):
    """f5e_layernorm_gelu: out = GELU(erf)(LayerNorm(x) * gamma + beta); x, out f32 [rows, C] row-strided views, out may be x."""
    if x.ndim != 2 or out.shape != x.shape or gamma.numel() != x.shape[1] or beta.numel() != x.shape[1]:
        raise _C.F5EError(f"layernorm_gelu: x and out [rows, C], gamma / beta [C] (got {tuple(x.shape)}, {tuple(out.shape)})")
    rows, Cc = x.shape
    (xp, ldx), (op, ldo) = _rows(x, (F32,), "layernorm_gelu: x", Cc, vec=1), _rows(out, (F32,), "layernorm_gelu: out", Cc, vec=1)
    require_device()
    check(lib().f5e_layernorm_gelu(_stream(), xp, ldx, op, ldo, _p(gamma, F32, "gamma"), _p(beta, F32, "beta"), rows, Cc,
                                   float(eps)), "f5e_layernorm_gelu")
    return out


def pack_wavlm_posconv_weight(w: Tensor, groups: int) -> Tensor:
    """Conv1d weight [D][D / groups][taps] (weight norm already folded) -> f32 [groups][taps][oc][ic] as f5e_wavlm_posconv reads it."""
    D, cg, taps = w.shape
    if D % groups or D // groups != cg:
        raise _C.F5EError(f"pack_wavlm_posconv_weight: weight {tuple(w.shape)} does not belong to {groups} groups")
    return w.reshape(groups, cg, cg, taps).permute(0, 3, 1, 2).to(F32).contiguous()


def wavlm_posconv(x: Tensor, w_packed: Tensor, bias: Tensor, frames: Optional[Tensor], out: Tensor, pad: Optional[int] = None):
    """f5e_wavlm_posconv: x, out f32 [B, T, D] -> out = x + GELU(conv(x) + bias) below frames[b], zero beyond."""
    xp, ldx, B, T, D = _btc(x, "wavlm_posconv: x")
    op, ldo, *os_ = _btc(out, "wavlm_posconv: out")
    if w_packed.ndim != 4:
        raise _C.F5EError("wavlm_posconv: w_packed must be [groups, taps, cg, cg] (pack_wavlm_posconv_weight)")
    G, taps, cg, cg2 = w_packed.shape
    if os_ != [B, T, D] or cg != cg2 or G * cg != D or bias.numel() != D or x.data_ptr() == out.data_ptr():
        raise _C.F5EError(f"wavlm_posconv: out like x {tuple(x.shape)} (no aliasing), w_packed [G, taps, D / G, D / G], bias [D]")
    pad = taps // 2 if pad is None else int(pad)
    require_device()
    check(lib().f5e_wavlm_posconv(_stream(), xp, ldx, _p(w_packed, F32, "w_packed"), _p(bias, F32, "bias"),
                                  _len(frames, B, "wavlm_posconv"), op, ldo, B, T, D, G, taps, pad), "f5e_wavlm_posconv")
    return out


def wavlm_gate(x: Tensor, w_gate: Tensor, b_gate: Tensor, head_const: Tensor, gate: Tensor):
    """f5e_wavlm_gate: x f32 [B * T, >= H dk] (the layer's normed input) -> gate f32 [B, H, T]."""
    if gate.ndim != 3 or x.ndim != 2 or w_gate.ndim != 2 or w_gate.shape[0] != 8:
        raise _C.F5EError("wavlm_gate: x [B * T, D], w_gate [8, dk], gate [B, H, T]")
    B, H, T = gate.shape
    dk = w_gate.shape[1]
    if x.shape[0] != B * T or b_gate.numel() != 8 or head_const.numel() != H:
        raise _C.F5EError(f"wavlm_gate: x needs {B * T} rows, b_gate 8 and head_const {H} elements")
    xp, ldx = _rows(x, (F32,), "wavlm_gate: x", H * dk)
    require_device()
    check(lib().f5e_wavlm_gate(_stream(), xp, ldx, _p(w_gate, F32, "w_gate"), _p(b_gate, F32, "b_gate"),
                               _p(head_const, F32, "head_const"), _p(gate, F32, "gate"), B, T, H, dk), "f5e_wavlm_gate")
    return gate


def relbias_attn(q: Tensor, k: Tensor, v: Tensor, gate: Tensor, table: Tensor, heads: int, scale: float,
                 kv_len: Optional[Tensor] = None, out: Optional[Tensor] = None):
    """f5e_relbias_attn_f32: q / k / v f32 [B * T, D] row-strided views, gate f32 [B, H, T], table f32 [H, 2 Tt - 1] (Tt >= T)
    -> out f32 [B * T, D]; scores scale q.k + gate[b, h, i] table[h, j - i + Tt - 1] over keys j < kv_len[b]; a query at or
    beyond kv_len[b] yields zeros."""
    if q.ndim != 2 or gate.ndim != 3 or table.ndim != 2:
        raise _C.F5EError("relbias_attn: q [B * T, D], gate [B, H, T], table [H, 2 Tt - 1]")
    M, D = q.shape
    B, H, T = gate.shape
    Tt = (table.shape[1] + 1) // 2
    if H != heads or M != B * T or D % heads or k.shape != (M, D) or v.shape != (M, D) or table.shape != (H, 2 * Tt - 1) or \
            Tt < T or (out is not None and out.shape != (M, D)):
        raise _C.F5EError(f"relbias_attn: inconsistent shapes q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)} gate "
                          f"{tuple(gate.shape)} table {tuple(table.shape)} heads={heads}")
    (qp, ldq), (kp, ldk), (vp, ldv) = _rows(q, (F32,), "relbias_attn: q", D), _rows(k, (F32,), "relbias_attn: k", D), \
        _rows(v, (F32,), "relbias_attn: v", D, vec=1)
    require_device()
    out = torch.empty(M, D, dtype=F32, device=q.device) if out is None else out
    op, ldo = _rows(out, (F32,), "relbias_attn: out", D)
    check(lib().f5e_relbias_attn_f32(_stream(), qp, ldq, kp, ldk, vp, ldv, op, ldo, _p(gate, F32, "gate"),
                                     _p(table, F32, "table"), Tt, _len(kv_len, B, "relbias_attn"), B, T, heads, D // heads,
                                     float(scale)), "f5e_relbias_attn_f32")
    return out


# ---- Whisper (csrc/whisper.hip) ----

WHISPER_N_FFT, WHISPER_HOP = 400, 160


def whisper_logmel_partials(B: int, T: int) -> int:
    """Scratch floats of ``whisper_logmel`` for B rows of T frames (host arithmetic)."""
    n = C.c_ulonglong(0)
    check(lib().f5e_whisper_logmel_partials(int(B), int(T), C.byref(n)), "f5e_whisper_logmel_partials")
    return int(n.value)


def whisper_logmel(wav: Tensor, lengths: Optional[Tensor], window: Tensor, twiddle: Tensor, fb: Tensor, T: int, *,
                   out: Optional[Tensor] = None, partials: Optional[Tensor] = None) -> Tensor:
    """f5e_whisper_logmel: wav f32 [B, S] (row-strided view), lengths i32 [B] on the device or None, window f32 [400], twiddle f32
    [400, 2] = (cos, sin)(2 pi i / 400), fb f32 [201, n_mels] -> out f32 [B, T, n_mels]: the features of
    ``WhisperFeatureExtractor`` for rows zero-padded (or cut) to 160 T samples."""
    if wav.ndim != 2 or fb.ndim != 2:
        raise _C.F5EError("whisper_logmel: wav [B, S] and fb [201, n_mels]; there is no CPU path")
    B, S = wav.shape
    n_mels = fb.shape[1]
    if window.shape != (WHISPER_N_FFT,) or twiddle.shape != (WHISPER_N_FFT, 2) or fb.shape[0] != WHISPER_N_FFT // 2 + 1:
        raise _C.F5EError(f"whisper_logmel: window [400], twiddle [400, 2], fb [201, n_mels] (got {tuple(window.shape)}, "
                          f"{tuple(twiddle.shape)}, {tuple(fb.shape)})")
    wp, ldw = _rows(wav, (F32,), "whisper_logmel: wav", S, vec=1)
    require_device()
    T = int(T)
    out = torch.empty(B, T, n_mels, dtype=F32, device=wav.device) if out is None else out
    if tuple(out.shape) != (B, T, n_mels):
        raise _C.F5EError(f"whisper_logmel: out must be [{B}, {T}, {n_mels}] (got {tuple(out.shape)})")
    need = whisper_logmel_partials(B, T) if T > 0 else 0
    partials = torch.empty(max(need, 1), dtype=F32, device=wav.device) if partials is None else partials
    if partials.numel() < need:
        raise _C.F5EError(f"whisper_logmel: partials needs {need} floats (whisper_logmel_partials)")
    check(lib().f5e_whisper_logmel(_stream(), wp, min(ldw, 0x7fffffff), _len(lengths, B, "whisper_logmel"),
                                   _p(window, F32, "window"), _p(twiddle, F32, "twiddle"), _p(fb, F32, "fb"), _p(out, F32, "out"),
                                   _p(partials, F32, "partials"), B, T, WHISPER_N_FFT, WHISPER_HOP, n_mels), "f5e_whisper_logmel")
    return out


def cross_attn_decode_f32(q: Tensor, k: Tensor, v: Tensor, heads: int, scale: float, rows_per_utt: int = 1,
                          kv_len: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """f5e_cross_attn_decode_f32: q f32 [R, D] (row-strided view), k / v f32 [B, Tk, D] (evenly spaced frames, unit channel
    stride) with B = R / rows_per_utt -> out f32 [R, D]: one query per row and head over the keys of the row's utterance;
    kv_len i32 [B] on the device limits the keys (None: all Tk)."""
    if q.ndim != 2 or k.ndim != 3 or v.ndim != 3 or k.shape != v.shape:
        raise _C.F5EError("cross_attn_decode_f32: q [R, D] and k, v [B, Tk, D] of one shape; there is no CPU path")
    R, D = q.shape
    kp, ldk, B, Tk, Dk = _btc(k, "cross_attn_decode_f32: k")
    vp, ldv, _, _, _ = _btc(v, "cross_attn_decode_f32: v", vec=1)
    if Dk != D or D % heads or rows_per_utt < 1 or R != B * rows_per_utt or (out is not None and out.shape != (R, D)):
        raise _C.F5EError(f"cross_attn_decode_f32: inconsistent shapes q {tuple(q.shape)} k {tuple(k.shape)} heads={heads} "
                          f"rows_per_utt={rows_per_utt}")
    qp, ldq = _rows(q, (F32,), "cross_attn_decode_f32: q", D)
    require_device()
    out = torch.empty(R, D, dtype=F32, device=q.device) if out is None else out
    op, ldo = _rows(out, (F32,), "cross_attn_decode_f32: out", D, vec=1)
    check(lib().f5e_cross_attn_decode_f32(_stream(), qp, ldq, kp, ldk, vp, ldv, op, ldo, _len(kv_len, B, "cross_attn_decode_f32"),
                                          R, rows_per_utt, Tk, heads, D // heads, float(scale)), "f5e_cross_attn_decode_f32")
    return out


def greedy_pick(logits: Tensor, tokens: Tensor, last: Tensor, done: Tensor, alive: Tensor, p: int, eos: int, *,
                V: Optional[int] = None, suppress: Optional[Tensor] = None, begin_suppress: Optional[Tensor] = None,
                first_step: bool = False):
    """f5e_greedy_pick: logits f32 [R, >= V] (row-strided view, only read), tokens i32 [R, >= p + 2], last / done i32 [R], alive
    i32 [1], suppress / begin_suppress i32 lists on the device.  Writes tokens[:, p + 1], last, done (0 -> 1) and alive."""
    if logits.ndim != 2 or tokens.ndim != 2:
        raise _C.F5EError("greedy_pick: logits [R, >= V] and tokens [R, >= p + 2]; there is no CPU path")
    R = logits.shape[0]
    V = logits.shape[1] if V is None else int(V)
    lp, ld = _rows(logits, (F32,), "greedy_pick: logits", V, vec=1)
    tp, ld_tok = _rows(tokens, (I32,), "greedy_pick: tokens", int(p) + 2, vec=1)
    if tokens.shape[0] != R or last.shape != (R,) or done.shape != (R,) or alive.numel() != 1:
        raise _C.F5EError(f"greedy_pick: tokens [{R}, .], last [{R}], done [{R}], alive [1]")
    require_device()
    check(lib().f5e_greedy_pick(_stream(), lp, ld, _p(suppress, I32, "suppress"), suppress.numel() if suppress is not None else 0,
                                _p(begin_suppress, I32, "begin_suppress"),
                                begin_suppress.numel() if begin_suppress is not None else 0, 1 if first_step else 0, tp, ld_tok,
                                _p(last, I32, "last"), _p(done, I32, "done"), _p(alive, I32, "alive"), R, V, int(p), int(eos)),
          "f5e_greedy_pick")
    return last


def whisper_beam_scratch(B: int, beam: int, V: int) -> int:
    """Scratch bytes of ``whisper_beam_step`` for B utterances of ``beam`` rows and V classes (host arithmetic)."""
    n = C.c_ulonglong(0)
    check(lib().f5e_whisper_beam_scratch(int(B), int(beam), int(V), C.byref(n)), "f5e_whisper_beam_scratch")
    return int(n.value)


def whisper_beam_step(logits: Tensor, score: Tensor, hyp_in: Tensor, anc_in: Tensor, hyp_out: Tensor, anc_out: Tensor, last: Tensor,
                      pool_hyp: Tensor, pool_len: Tensor, pool_score: Tensor, pool_n: Tensor, open_: Tensor, alive: Tensor,
                      p: int, n0: int, cap: int, eos: int, beam: int, *, V: Optional[int] = None,
                      suppress: Optional[Tensor] = None, begin_suppress: Optional[Tensor] = None, length_penalty: float = 1.0,
                      scratch: Optional[Tensor] = None, _ts: Optional[tuple] = None):
    """One step of Whisper's pooled beam search (f5e_whisper_beam_step, where the rules are written out): logits f32
    [B * beam, >= V] (row-strided view, only read), score f32 / last i32 [B * beam], hyp / anc tables contiguous i32 [B * beam, ld]
    (double-buffered), pool_hyp i32 [B, beam, ld], pool_len i32 / pool_score f32 [B, beam], pool_n / open_ / alive i32 [B],
    scratch u8 [>= whisper_beam_scratch(B, beam, V)] (allocated when None).  Limits on beam, V, p, n0, cap and eos are the
    library's."""
    if logits.ndim != 2 or hyp_in.ndim != 2:
        raise _C.F5EError("whisper_beam_step: logits [B * beam, >= V] and tables [B * beam, ld]; there is no CPU path")
    R, beam = logits.shape[0], int(beam)
    V = logits.shape[1] if V is None else int(V)
    if beam < 1 or R % beam:
        raise _C.F5EError(f"whisper_beam_step: beam = {beam} must be at least 1 and divide the {R} rows")
    B, ld = R // beam, hyp_in.shape[1]
    if V > logits.shape[1]:
        raise _C.F5EError(f"whisper_beam_step: V = {V} exceeds the {logits.shape[1]} columns of logits")
    lp, ldl = _rows(logits, (F32,), "whisper_beam_step: logits", max(V, 1), vec=1)
    for t, nm in ((hyp_in, "hyp_in"), (anc_in, "anc_in"), (hyp_out, "hyp_out"), (anc_out, "anc_out")):
        if t.dtype != I32 or tuple(t.shape) != (R, ld) or not t.is_contiguous():
            raise _C.F5EError(f"whisper_beam_step: {nm} must be a contiguous i32 tensor [{R}, {ld}]")
    if pool_hyp.dtype != I32 or tuple(pool_hyp.shape) != (B, beam, ld) or not pool_hyp.is_contiguous():
        raise _C.F5EError(f"whisper_beam_step: pool_hyp must be a contiguous i32 tensor [{B}, {beam}, {ld}]")
    if hyp_in.data_ptr() == hyp_out.data_ptr() or anc_in.data_ptr() == anc_out.data_ptr():
        raise _C.F5EError("whisper_beam_step: the tables are double-buffered: in and out must differ")
    if score.shape != (R,) or last.shape != (R,) or tuple(pool_len.shape) != (B, beam) or tuple(pool_score.shape) != (B, beam) \
            or pool_n.shape != (B,) or open_.shape != (B,) or alive.shape != (B,) or not pool_len.is_contiguous() \
            or not pool_score.is_contiguous():
        raise _C.F5EError(f"whisper_beam_step: score / last [{R}], pool_len / pool_score [{B}, {beam}], pool_n / open / alive [{B}]")
    require_device()
    if scratch is None:
        scratch = torch.empty(max(whisper_beam_scratch(B, beam, V), 4), dtype=torch.uint8, device=logits.device)
    if scratch.dtype != torch.uint8 or not scratch.is_contiguous():
        raise _C.F5EError("whisper_beam_step: scratch must be a contiguous uint8 tensor")
    args = (_stream(), lp, ldl, _p(suppress, I32, "suppress"), suppress.numel() if suppress is not None else 0,
            _p(begin_suppress, I32, "begin_suppress"), begin_suppress.numel() if begin_suppress is not None else 0,
            _p(score, F32, "score"), _p(hyp_in, I32, "hyp_in"), _p(anc_in, I32, "anc_in"), _p(hyp_out, I32, "hyp_out"),
            _p(anc_out, I32, "anc_out"), ld, _p(last, I32, "last"), _p(pool_hyp, I32, "pool_hyp"), _p(pool_len, I32, "pool_len"),
            _p(pool_score, F32, "pool_score"), _p(pool_n, I32, "pool_n"), _p(open_, I32, "open"), _p(alive, I32, "alive"),
            C.c_void_p(scratch.data_ptr()), scratch.numel(), B, beam, V, int(p), int(n0), int(cap), int(eos), float(length_penalty))
    if _ts is None:
        check(lib().f5e_whisper_beam_step(*args), "f5e_whisper_beam_step")
    else:
        no_timestamps, max_initial, desc = _ts
        if desc.dtype != I32 or tuple(desc.shape) != (R, 4) or not desc.is_contiguous():
            raise _C.F5EError(f"whisper_beam_step_ts: desc must be a contiguous i32 tensor [{R}, 4]")
        check(lib().f5e_whisper_beam_step_ts(*args, int(no_timestamps), -1 if max_initial is None else int(max_initial),
                                             _p(desc, I32, "desc")), "f5e_whisper_beam_step_ts")
    return last


def whisper_beam_step_ts(logits: Tensor, score: Tensor, hyp_in: Tensor, anc_in: Tensor, hyp_out: Tensor, anc_out: Tensor,
                         last: Tensor, pool_hyp: Tensor, pool_len: Tensor, pool_score: Tensor, pool_n: Tensor, open_: Tensor,
                         alive: Tensor, p: int, n0: int, cap: int, eos: int, beam: int, no_timestamps: int, desc: Tensor, *,
                         max_initial: Optional[int] = None, **kw):
    """``whisper_beam_step`` under Whisper's timestamp rules (f5e_whisper_beam_step_ts): ``desc`` i32 [B * beam, 4] receives the
    rows' rule descriptors (``whisper_ts_rule``), which the chunk launch applies as one more mask."""
    return whisper_beam_step(logits, score, hyp_in, anc_in, hyp_out, anc_out, last, pool_hyp, pool_len, pool_score, pool_n, open_,
                             alive, p, n0, cap, eos, beam, _ts=(no_timestamps, max_initial, desc), **kw)


def _ts_common(name: str, logits: Tensor, tokens: Tensor, V: Optional[int], p: int, suppress, begin_suppress):
    if logits.ndim != 2 or tokens.ndim != 2 or tokens.shape[0] != logits.shape[0]:
        raise _C.F5EError(f"{name}: logits [R, >= V] and tokens [R, >= p + 2]; there is no CPU path")
    V = logits.shape[1] if V is None else int(V)
    if V > logits.shape[1]:
        raise _C.F5EError(f"{name}: V = {V} exceeds the {logits.shape[1]} columns of logits")
    lp, ld = _rows(logits, (F32,), f"{name}: logits", max(V, 1), vec=1)
    tp, ld_tok = _rows(tokens, (I32,), f"{name}: tokens", int(p) + 2, vec=1)
    return (_stream(), lp, ld, _p(suppress, I32, "suppress"), suppress.numel() if suppress is not None else 0,
            _p(begin_suppress, I32, "begin_suppress"), begin_suppress.numel() if begin_suppress is not None else 0, tp, ld_tok), V


def whisper_ts_pick(logits: Tensor, tokens: Tensor, last: Tensor, done: Tensor, alive: Tensor, sum_logp: Tensor, p: int, n0: int,
                    eos: int, no_timestamps: int, *, V: Optional[int] = None, suppress: Optional[Tensor] = None,
                    begin_suppress: Optional[Tensor] = None, max_initial: Optional[int] = None):
    """f5e_whisper_ts_pick: ``greedy_pick`` under Whisper's timestamp rules.  The generated tokens of a row are tokens[r, n0:p + 1];
    begin_suppress counts at the first step (p + 1 == n0); sum_logp f32 [R] gains the log-probability of the pick among the
    allowed classes.  Writes tokens[:, p + 1], last, done (0 -> 1), alive and sum_logp."""
    head, V = _ts_common("whisper_ts_pick", logits, tokens, V, p, suppress, begin_suppress)
    R = logits.shape[0]
    if last.shape != (R,) or done.shape != (R,) or alive.numel() != 1 or sum_logp.shape != (R,):
        raise _C.F5EError(f"whisper_ts_pick: last [{R}], done [{R}], alive [1], sum_logp [{R}]")
    require_device()
    check(lib().f5e_whisper_ts_pick(*head, _p(last, I32, "last"), _p(done, I32, "done"), _p(alive, I32, "alive"),
                                    _p(sum_logp, F32, "sum_logp"), R, V, int(p), int(n0), int(eos), int(no_timestamps),
                                    -1 if max_initial is None else int(max_initial)), "f5e_whisper_ts_pick")
    return last


def whisper_verify(logits: Tensor, hist: Tensor, cand: Tensor, logp: Tensor, p: int, n0: int, eos: int,
                   no_timestamps: Optional[int] = None, *, V: Optional[int] = None, suppress: Optional[Tensor] = None,
                   begin_suppress: Optional[Tensor] = None, max_initial: Optional[int] = None):
    """f5e_whisper_verify: the picks of U + 1 positions per row at once.  logits f32 [R * (U + 1), >= V] (row r * (U + 1) + j =
    position p + j of row r), hist i32 [R, >= p + U + 1] (the final tokens up to column p, the drafts behind), cand i32 [R, U + 1]
    and logp f32 [R, U + 1] (written): what ``greedy_pick`` (``no_timestamps`` None) or ``whisper_ts_pick`` would pick at p + j
    with the history hist[r, n0:p + j + 1], and the ``sum_logp`` increment of the latter (zeros without rules), bit for bit."""
    if logits.ndim != 2 or hist.ndim != 2 or cand.ndim != 2 or cand.shape != logp.shape or cand.shape[0] != hist.shape[0] or \
            logits.shape[0] != cand.numel():
        raise _C.F5EError("whisper_verify: logits [R * (U + 1), >= V], hist [R, >= p + U + 1], cand and logp [R, U + 1]; there is "
                          "no CPU path")
    R, U = cand.shape[0], cand.shape[1] - 1
    V = logits.shape[1] if V is None else int(V)
    if V > logits.shape[1]:
        raise _C.F5EError(f"whisper_verify: V = {V} exceeds the {logits.shape[1]} columns of logits")
    lp, ld = _rows(logits, (F32,), "whisper_verify: logits", max(V, 1), vec=1)
    hp, ld_hist = _rows(hist, (I32,), "whisper_verify: hist", int(p) + U + 1, vec=1)
    require_device()
    check(lib().f5e_whisper_verify(_stream(), lp, ld, _p(suppress, I32, "suppress"), suppress.numel() if suppress is not None else 0,
                                   _p(begin_suppress, I32, "begin_suppress"),
                                   begin_suppress.numel() if begin_suppress is not None else 0, hp, ld_hist, _p(cand, I32, "cand"),
                                   _p(logp, F32, "logp"), R, U, V, int(p), int(n0), int(eos),
                                   -1 if no_timestamps is None else int(no_timestamps),
                                   -1 if max_initial is None else int(max_initial)), "f5e_whisper_verify")
    return cand, logp


def whisper_accept(cand: Tensor, logp: Tensor, hist: Tensor, tokens: Tensor, last: Tensor, done: Tensor, alive: Tensor,
                   sum_logp: Optional[Tensor], adv: Tensor, p: int, eos: int):
    """f5e_whisper_accept: the accept step behind ``whisper_verify``.  cand i32 / logp f32 [R, U + 1]; hist and tokens i32
    [R, >= p + U + 2]; last, done i32 [R]; alive, adv i32 [1]; sum_logp f32 [R] or None.  An open row agrees with its drafts
    hist[r, p + 1:p + 1 + m] = cand[r, :m]; the common advance a = min(m + 1) over the open rows goes to ``adv``; every row gets
    tokens[r, p + 1:p + a + 1] (eos from a row's end on), last, done, sum_logp (the kept picks' logp) and alive as ``a`` single
    steps would have left them, and hist is put right (tokens up to p + a, eos on the rejected drafts)."""
    if cand.ndim != 2 or cand.shape != logp.shape or hist.ndim != 2 or tokens.ndim != 2 or cand.shape[1] < 2:
        raise _C.F5EError("whisper_accept: cand and logp [R, U + 1] with U >= 1, hist and tokens [R, >= p + U + 2]; there is no CPU "
                          "path")
    R, U = cand.shape[0], cand.shape[1] - 1
    if hist.shape[0] != R or tokens.shape[0] != R or last.shape != (R,) or done.shape != (R,) or alive.numel() != 1 or \
            adv.numel() != 1 or (sum_logp is not None and sum_logp.shape != (R,)):
        raise _C.F5EError(f"whisper_accept: hist / tokens [{R}, .], last / done / sum_logp [{R}], alive / adv [1]")
    hp, ld_hist = _rows(hist, (I32,), "whisper_accept: hist", int(p) + U + 2, vec=1)
    tp, ld_tok = _rows(tokens, (I32,), "whisper_accept: tokens", int(p) + U + 2, vec=1)
    require_device()
    check(lib().f5e_whisper_accept(_stream(), _p(cand, I32, "cand"), _p(logp, F32, "logp"), hp, ld_hist, tp, ld_tok,
                                   _p(last, I32, "last"), _p(done, I32, "done"), _p(alive, I32, "alive"),
                                   _p(sum_logp, F32, "sum_logp"), _p(adv, I32, "adv"), R, U, int(p), int(eos)), "f5e_whisper_accept")
    return adv


def whisper_sample_pick(logits: Tensor, tokens: Tensor, last: Tensor, done: Tensor, alive: Tensor, sum_logp: Tensor, p: int, n0: int,
                        eos: int, no_timestamps: Optional[int], temperature: float, seed: int, row_key: Tensor, serial: Tensor, *,
                        V: Optional[int] = None, suppress: Optional[Tensor] = None, begin_suppress: Optional[Tensor] = None,
                        max_initial: Optional[int] = None):
    """f5e_whisper_sample_pick: ``whisper_ts_pick`` with a draw from softmax(x / temperature) over the allowed classes in place of
    the argmax.  The noise is a function of (class, p, serial[r], row_key[r], seed) only (i32 [R] device tensors and a 64-bit
    seed), so a row's draw does not depend on its batch.  ``no_timestamps`` None: without the timestamp rules.  sum_logp gains the
    T = 1 log-probability of the pick among the allowed classes.  Writes tokens[:, p + 1], last, done (0 -> 1), alive, sum_logp."""
    R = logits.shape[0]
    if last.shape != (R,) or done.shape != (R,) or alive.numel() != 1 or sum_logp.shape != (R,) or row_key.shape != (R,) or \
            serial.shape != (R,):
        raise _C.F5EError(f"whisper_sample_pick: last [{R}], done [{R}], alive [1], sum_logp [{R}], row_key [{R}], serial [{R}]")
    if not 0 <= int(seed) < 1 << 64:
        raise _C.F5EError(f"whisper_sample_pick: the seed must lie in 0 .. 2^64 - 1 (got {seed})")
    head, V = _ts_common("whisper_sample_pick", logits, tokens, V, p, suppress, begin_suppress)
    require_device()
    check(lib().f5e_whisper_sample_pick(*head, _p(last, I32, "last"), _p(done, I32, "done"), _p(alive, I32, "alive"),
                                        _p(sum_logp, F32, "sum_logp"), R, V, int(p), int(n0), int(eos),
                                        -1 if no_timestamps is None else int(no_timestamps),
                                        -1 if max_initial is None else int(max_initial), float(temperature), int(seed),
                                        _p(row_key, I32, "row_key"), _p(serial, I32, "serial")), "f5e_whisper_sample_pick")
    return last


# ---- Whisper's decode step with the position on the device (csrc/whisper_step.hip) ----

STEP_REC_WORDS = 8     # the step record: i32 [8] = p, n0, seed_lo, seed_hi, temperature bits, 3 reserved words


def whisper_step_record(p: int, n0: int, seed: int = 0, temperature: float = 0.0) -> Tensor:
    """The step record's words as a HOST i32 [8] tensor, to be copied into the device record: p, n0, the seed's low / high
    word, the fp32 temperature's bits, three zeros."""
    import struct
    if not 0 <= int(seed) < 1 << 64:
        raise _C.F5EError(f"whisper_step_record: the seed must lie in 0 .. 2^64 - 1 (got {seed})")

    def i32(u):
        return u - (1 << 32) if u >= 1 << 31 else u
    seed = int(seed)
    bits = struct.unpack("<I", struct.pack("<f", float(temperature)))[0]
    return torch.tensor([int(p), int(n0), i32(seed & 0xffffffff), i32(seed >> 32), i32(bits), 0, 0, 0], dtype=I32)


def _rec(rec: Tensor, name: str):
    if not isinstance(rec, Tensor) or not rec.is_cuda:
        raise _C.F5EError(f"{name}: the step record must live on the GPU; there is no CPU path")
    return _vec(rec, I32, f"{name}: rec", (STEP_REC_WORDS,), align=16)


def attn_decode_dev_f32(qkv: Tensor, kc: Tensor, vc: Tensor, rec: Tensor, heads: int, scale: float, out: Optional[Tensor] = None,
                        begin: Optional[Tensor] = None):
    """``attn_decode_f32`` without an ancestry table at the position the step record holds (f5e_attn_decode_dev_f32): qkv f32
    [R, >= 3 D], kc / vc f32 [R, P, D] views of the layer's caches (the strides ``attn_decode_f32`` takes), rec i32 [8] on the
    device, begin i32 [R] on the device or None -> out f32 [R, D].  p = rec[0] clamped to [0, P - 1] on the device; slot [r, p]
    of both caches receives the step's k / v.  The launch does not depend on p, so it can be captured once."""
    if not isinstance(qkv, Tensor) or qkv.ndim != 2 or kc.ndim != 3 or kc.shape != vc.shape or kc.stride() != vc.stride():
        raise _C.F5EError("attn_decode_dev_f32: qkv [R, >= 3 D] and kc, vc [R, P, D] with equal strides; there is no CPU path")
    R, P, D = kc.shape
    for t, nm in ((qkv, "qkv"), (kc, "kc"), (vc, "vc")):
        if not t.is_cuda or t.dtype != F32 or t.stride(-1) != 1:
            raise _C.F5EError(f"attn_decode_dev_f32: {nm} must be an f32 GPU tensor with unit channel stride; there is no CPU path")
    if qkv.shape[0] != R or D % heads:
        raise _C.F5EError(f"attn_decode_dev_f32: qkv rows {qkv.shape[0]} != {R}, heads {heads} must divide {D}")
    pos_stride = kc.stride(1) if P > 1 else max(D, kc.stride(1))
    row_stride = kc.stride(0) if R > 1 else max(kc.stride(0), (P - 1) * pos_stride + D)
    for t in (kc, vc):
        have = t.untyped_storage().nbytes() // 4 - t.storage_offset()
        if pos_stride < D or row_stride < (P - 1) * pos_stride + D or have < (R - 1) * row_stride + (P - 1) * pos_stride + D \
                or pos_stride % 4 or row_stride % 4 or t.data_ptr() % 16:
            raise _C.F5EError(f"attn_decode_dev_f32: cache strides ({row_stride}, {pos_stride}) must be multiples of 4 spanning "
                              f"[{R}, {P}, {D}] inside the storage, kc and vc 16-byte aligned")
    qp, ldq = _rows(qkv, (F32,), "attn_decode_dev_f32: qkv", 3 * D)
    rp = _rec(rec, "attn_decode_dev_f32")
    bp = None if begin is None else _vec(begin, I32, "attn_decode_dev_f32: begin", (R,))
    require_device()
    out = torch.empty(R, D, dtype=F32, device=qkv.device) if out is None else out
    if out.shape != (R, D):
        raise _C.F5EError(f"attn_decode_dev_f32: out must be [{R}, {D}]")
    op, ldo = _rows(out, (F32,), "attn_decode_dev_f32: out", D, vec=1)
    check(lib().f5e_attn_decode_dev_f32(_stream(), qp, ldq, C.c_void_p(kc.data_ptr()), C.c_void_p(vc.data_ptr()), row_stride,
                                        pos_stride, bp, op, ldo, R, P, heads, D // heads, rp, float(scale)),
          "f5e_attn_decode_dev_f32")
    return out


def _whisper_embed_dev(op: str, emb_dtypes, last, emb, pos, out, rec, begin):
    """``whisper_embed_dev`` and ``whisper_embed_w16_dev``: one set of checks, the entry point follows ``emb.dtype``."""
    if not isinstance(last, Tensor) or last.ndim != 1 or emb.ndim != 2 or pos.ndim != 2 or out.ndim not in (2, 3):
        raise _C.F5EError(f"{op}: last [R], emb [V, D], pos [P, D] and out [R, D]; there is no CPU path")
    R, D = last.shape[0], emb.shape[1]
    if R < 1 or out.numel() != R * D or out.shape[0] != R or out.shape[-1] != D or pos.shape[1] != D or D % 4:
        raise _C.F5EError(f"{op}: last {tuple(last.shape)}, emb {tuple(emb.shape)}, pos {tuple(pos.shape)}, out "
                          f"{tuple(out.shape)}: out must be [R, D] and D a multiple of 4")
    for t, nm in ((emb, "emb"), (pos, "pos"), (out, "out")):
        if t.is_cuda and t.data_ptr() % (8 if t.dtype in W16_TYPES else 16):
            raise _C.F5EError(f"{op}: {nm} must be 16-byte aligned (a 16-bit emb: 8-byte)")
    bp = None if begin is None else _vec(begin, I32, f"{op}: begin", (R,))
    if emb.dtype not in emb_dtypes:
        raise _C.F5EError(f"{op}: emb must be {'f32' if emb_dtypes == (F32,) else 'fp16 / bf16'} (got {emb.dtype})")
    front = (_p(last, I32, f"{op}: last"), bp, _p(emb, None, f"{op}: emb"))
    back = (_p(pos, F32, f"{op}: pos"), _p(out, F32, f"{op}: out"), R, D, _rec(rec, op), pos.shape[0], emb.shape[0])
    require_device()
    if emb.dtype == F32:
        check(lib().f5e_whisper_embed_dev(_stream(), *front, *back), "f5e_whisper_embed_dev")
    else:
        check(lib().f5e_whisper_embed_w16_dev(_stream(), *front, W16_TYPES[emb.dtype], *back), "f5e_whisper_embed_w16_dev")
    return out


def whisper_embed_dev(last: Tensor, emb: Tensor, pos: Tensor, out: Tensor, rec: Tensor, begin: Optional[Tensor] = None):
    """out[r] = emb[last[r]] + pos[max(p - begin[r], 0)] with p from the step record (f5e_whisper_embed_dev): last i32 [R], emb f32
    [V, D], pos f32 [P, D], begin i32 [R] or None, rec i32 [8], out f32 [R, D] (or [R, 1, D]), all contiguous on the device."""
    return _whisper_embed_dev("whisper_embed_dev", (F32,), last, emb, pos, out, rec, begin)


def whisper_embed_w16_dev(last: Tensor, emb: Tensor, pos: Tensor, out: Tensor, rec: Tensor, begin: Optional[Tensor] = None):
    """``whisper_embed_dev`` reading a 16-bit token table (f5e_whisper_embed_w16_dev): emb fp16 or bf16 [V, D], 8-byte aligned."""
    return _whisper_embed_dev("whisper_embed_w16_dev", tuple(W16_TYPES), last, emb, pos, out, rec, begin)


def _pick_dev_common(name: str, logits: Tensor, tokens: Tensor, last: Tensor, done: Tensor, alive: Tensor, rec: Tensor,
                     V: Optional[int], suppress, begin_suppress):
    if not isinstance(logits, Tensor) or logits.ndim != 2 or tokens.ndim != 2 or tokens.shape[0] != logits.shape[0]:
        raise _C.F5EError(f"{name}: logits [R, >= V] and tokens [R, >= 2]; there is no CPU path")
    R = logits.shape[0]
    V = logits.shape[1] if V is None else int(V)
    if V > logits.shape[1]:
        raise _C.F5EError(f"{name}: V = {V} exceeds the {logits.shape[1]} columns of logits")
    if last.shape != (R,) or done.shape != (R,) or alive.numel() != 1:
        raise _C.F5EError(f"{name}: last [{R}], done [{R}], alive [1]")
    lp, ld = _rows(logits, (F32,), f"{name}: logits", max(V, 1), vec=1)
    tp, ld_tok = _rows(tokens, (I32,), f"{name}: tokens", 2, vec=1)
    head = (_stream(), lp, ld, _p(suppress, I32, "suppress"), suppress.numel() if suppress is not None else 0,
            _p(begin_suppress, I32, "begin_suppress"), begin_suppress.numel() if begin_suppress is not None else 0, tp, ld_tok,
            tokens.shape[1], _p(last, I32, "last"), _p(done, I32, "done"), _p(alive, I32, "alive"))
    return head, R, V, _rec(rec, name)


def greedy_pick_dev(logits: Tensor, tokens: Tensor, last: Tensor, done: Tensor, alive: Tensor, rec: Tensor, eos: int, *,
                    V: Optional[int] = None, suppress: Optional[Tensor] = None, begin_suppress: Optional[Tensor] = None):
    """f5e_greedy_pick_dev: ``greedy_pick`` at the step record's position (p clamped to the token table; ``begin_suppress``
    counts iff p + 1 == n0), then ``alive`` and p += 1 by one thread.  rec i32 [8] on the device."""
    head, R, V, rp = _pick_dev_common("greedy_pick_dev", logits, tokens, last, done, alive, rec, V, suppress, begin_suppress)
    require_device()
    check(lib().f5e_greedy_pick_dev(*head, R, V, rp, int(eos)), "f5e_greedy_pick_dev")
    return last


def whisper_ts_pick_dev(logits: Tensor, tokens: Tensor, last: Tensor, done: Tensor, alive: Tensor, sum_logp: Tensor, rec: Tensor,
                        eos: int, no_timestamps: int, *, V: Optional[int] = None, suppress: Optional[Tensor] = None,
                        begin_suppress: Optional[Tensor] = None, max_initial: Optional[int] = None):
    """f5e_whisper_ts_pick_dev: ``whisper_ts_pick`` with p and n0 from the step record, then ``alive`` and p += 1."""
    head, R, V, rp = _pick_dev_common("whisper_ts_pick_dev", logits, tokens, last, done, alive, rec, V, suppress, begin_suppress)
    if sum_logp.shape != (R,):
        raise _C.F5EError(f"whisper_ts_pick_dev: sum_logp [{R}]")
    require_device()
    check(lib().f5e_whisper_ts_pick_dev(*head, _p(sum_logp, F32, "sum_logp"), R, V, rp, int(eos), int(no_timestamps),
                                        -1 if max_initial is None else int(max_initial)), "f5e_whisper_ts_pick_dev")
    return last


def whisper_sample_pick_dev(logits: Tensor, tokens: Tensor, last: Tensor, done: Tensor, alive: Tensor, sum_logp: Tensor,
                            rec: Tensor, eos: int, no_timestamps: Optional[int], row_key: Tensor, serial: Tensor, *,
                            V: Optional[int] = None, suppress: Optional[Tensor] = None, begin_suppress: Optional[Tensor] = None,
                            max_initial: Optional[int] = None):
    """f5e_whisper_sample_pick_dev: ``whisper_sample_pick`` with p, n0, the seed and the temperature from the step record
    (``whisper_step_record``), then ``alive`` and p += 1."""
    head, R, V, rp = _pick_dev_common("whisper_sample_pick_dev", logits, tokens, last, done, alive, rec, V, suppress,
                                      begin_suppress)
    if sum_logp.shape != (R,) or row_key.shape != (R,) or serial.shape != (R,):
        raise _C.F5EError(f"whisper_sample_pick_dev: sum_logp [{R}], row_key [{R}], serial [{R}]")
    require_device()
    check(lib().f5e_whisper_sample_pick_dev(*head, _p(sum_logp, F32, "sum_logp"), R, V, rp, int(eos),
                                            -1 if no_timestamps is None else int(no_timestamps),
                                            -1 if max_initial is None else int(max_initial), _p(row_key, I32, "row_key"),
                                            _p(serial, I32, "serial")), "f5e_whisper_sample_pick_dev")
    return last


def whisper_ts_rule(logits: Tensor, tokens: Tensor, p: int, n0: int, eos: int, no_timestamps: int, *, V: Optional[int] = None,
                    suppress: Optional[Tensor] = None, begin_suppress: Optional[Tensor] = None, max_initial: Optional[int] = None,
                    out: Optional[Tensor] = None) -> Tensor:
    """f5e_whisper_ts_rule: -> desc i32 [R, 4] = (text ban: 0 none / 1 [0, eos) / 2 all text, lo, hi, 0) per row: what
    Whisper's timestamp rules ban for the histories tokens[r, n0:p + 1] and these logits, besides the suppressed classes and
    <|notimestamps|> itself; the timestamps allowed are [lo, hi]."""
    head, V = _ts_common("whisper_ts_rule", logits, tokens, V, p, suppress, begin_suppress)
    R = logits.shape[0]
    out = torch.empty(R, 4, dtype=I32, device=logits.device) if out is None else out
    if out.dtype != I32 or tuple(out.shape) != (R, 4) or not out.is_contiguous():
        raise _C.F5EError(f"whisper_ts_rule: out must be a contiguous i32 tensor [{R}, 4]")
    require_device()
    check(lib().f5e_whisper_ts_rule(*head, _p(out, I32, "out"), R, V, int(p), int(n0), int(eos), int(no_timestamps),
                                    -1 if max_initial is None else int(max_initial)), "f5e_whisper_ts_rule")
    return out


# ---- Whisper word timestamps (csrc/whisper_align.hip) ----

DTW_MAX_N, DTW_MAX_M = 448, 4096


def cross_attn_probs_f32(q: Tensor, k: Tensor, heads_sel: Tensor, heads: int, scale: float, out: Tensor, rows_per_utt: int = 1,
                         m_len: Optional[Tensor] = None) -> Tensor:
    """f5e_cross_attn_probs_f32: q f32 [R, D] (row-strided view), k f32 [B, Tk, D] with B = R / rows_per_utt, heads_sel i32
    [n_sel] on the device (heads of this layer) -> out f32 [R, n_sel, >= m] (a view with unit column stride; a token position and
    the heads' place among all alignment heads are the caller's slicing): out[r, s, :m] = the softmax over all Tk keys of
    head heads_sel[s], m = min(m_len[u], out.shape[2], Tk) (m_len i32 [B] on the device; None: Tk); columns at or beyond m are not
    written."""
    if q.ndim != 2 or k.ndim != 3 or out.ndim != 3 or heads_sel.ndim != 1:
        raise _C.F5EError("cross_attn_probs_f32: q [R, D], k [B, Tk, D], heads_sel [n_sel], out [R, n_sel, >= m]; there is no CPU "
                          "path")
    R, D = q.shape
    kp, ldk, B, Tk, Dk = _btc(k, "cross_attn_probs_f32: k")
    n_sel = heads_sel.shape[0]
    if Dk != D or D % heads or rows_per_utt < 1 or R != B * rows_per_utt or n_sel < 1 or out.shape[0] != R or out.shape[1] != n_sel:
        raise _C.F5EError(f"cross_attn_probs_f32: inconsistent shapes q {tuple(q.shape)} k {tuple(k.shape)} out {tuple(out.shape)} "
                          f"heads={heads} n_sel={n_sel} rows_per_utt={rows_per_utt}")
    cols = out.shape[2]
    if not out.is_cuda or out.dtype != F32 or cols < 1 or (cols > 1 and out.stride(2) != 1):
        raise _C.F5EError(f"cross_attn_probs_f32: out must be an f32 GPU view with unit column stride "
                          f"(got {out.dtype}, shape {tuple(out.shape)}, strides {tuple(out.stride())})")
    s_row = out.stride(0) if R > 1 else 0
    s_sel = out.stride(1) if n_sel > 1 else 0
    have = out.untyped_storage().nbytes() // 4 - out.storage_offset()
    if s_row < 0 or s_sel < 0 or have < (R - 1) * s_row + (n_sel - 1) * s_sel + min(cols, Tk):
        raise _C.F5EError("cross_attn_probs_f32: out does not fit its storage")
    qp, ldq = _rows(q, (F32,), "cross_attn_probs_f32: q", D)
    require_device()
    check(lib().f5e_cross_attn_probs_f32(_stream(), qp, ldq, kp, ldk, _p(heads_sel, I32, "heads_sel"), n_sel,
                                         _len(m_len, B, "cross_attn_probs_f32"), cols, C.c_void_p(out.data_ptr()), s_row, s_sel, R,
                                         rows_per_utt, Tk, heads, D // heads, float(scale)), "f5e_cross_attn_probs_f32")
    return out


def dtw_cost_f32(probs: Tensor, n_rows: Tensor, m_len: Tensor, width: int = 7, M: Optional[int] = None,
                 out: Optional[Tensor] = None) -> Tensor:
    """f5e_dtw_cost_f32: probs f32 [B, n_sel, N_cap, ld] (contiguous), n_rows / m_len i32 [B] on the device -> C f32
    [B, N_cap, M] (M: the column capacity, ld when None): per-column normalisation over the rows, median of ``width`` along the
    columns, minus the mean over the heads.  Cells outside (n_rows, m_len) are not written."""
    if probs.ndim != 4:
        raise _C.F5EError(f"dtw_cost_f32: probs must be [B, n_sel, N_cap, ld] (got {tuple(probs.shape)}); there is no CPU path")
    B, n_sel, N_cap, ld = probs.shape
    M = ld if M is None else int(M)
    if not 1 <= M <= ld:
        raise _C.F5EError(f"dtw_cost_f32: M = {M} must lie in 1 .. {ld}")
    out = torch.zeros(B, N_cap, M, dtype=F32, device=probs.device) if out is None else out
    if out.shape != (B, N_cap, M):
        raise _C.F5EError(f"dtw_cost_f32: out must be [{B}, {N_cap}, {M}] (got {tuple(out.shape)})")
    require_device()
    check(lib().f5e_dtw_cost_f32(_stream(), _p(probs, F32, "probs"), ld, _len(n_rows, B, "dtw_cost_f32"),
                                 _len(m_len, B, "dtw_cost_f32"), _p(out, F32, "out"), M, B, n_sel, N_cap, M, int(width)),
          "f5e_dtw_cost_f32")
    return out


def dtw_workspace_bytes(B: int, N_cap: int, M_cap: int) -> int:
    """Scratch bytes of ``dtw_path`` for B lattices of up to N_cap x M_cap cells (host arithmetic)."""
    n = C.c_ulonglong(0)
    check(lib().f5e_dtw_workspace_bytes(int(B), int(N_cap), int(M_cap), C.byref(n)), "f5e_dtw_workspace_bytes")
    return int(n.value)


def dtw_path(cost: Tensor, n_rows: Tensor, m_len: Tensor, first: Optional[Tensor] = None,
             workspace: Optional[Tensor] = None) -> Tensor:
    """f5e_dtw_path: cost f32 [B, N_cap, M_cap] (contiguous, only read), n_rows / m_len i32 [B] on the device -> first i32
    [B, N_cap]: the column at which the warping path enters row t, -1 at and beyond n_rows.  workspace: a device tensor of at
    least ``dtw_workspace_bytes`` bytes (allocated here when None)."""
    if cost.ndim != 3:
        raise _C.F5EError(f"dtw_path: cost must be [B, N_cap, M_cap] (got {tuple(cost.shape)}); there is no CPU path")
    B, N_cap, M_cap = cost.shape
    first = torch.empty(B, N_cap, dtype=I32, device=cost.device) if first is None else first
    if first.shape != (B, N_cap):
        raise _C.F5EError(f"dtw_path: first must be [{B}, {N_cap}] (got {tuple(first.shape)})")
    require_device()
    workspace, nbytes = _workspace(workspace, dtw_workspace_bytes(B, N_cap, M_cap), I32, cost.device)
    check(lib().f5e_dtw_path(_stream(), _p(cost, F32, "cost"), M_cap, _len(n_rows, B, "dtw_path"), _len(m_len, B, "dtw_path"),
                             _p(first, I32, "first"), _p(workspace, None, "workspace"), nbytes, B, N_cap, M_cap), "f5e_dtw_path")
    return first


# ---- UTMOS (csrc/utmos.hip) ----

LSTM_MAX_H, LSTM_MAX_B, LSTM_MAX_T = 1024, 16, 4096


def w2v_conv0_gn_partials(B: int, S: int, C_: int) -> int:
    """Floats of scratch that ``w2v_conv0_gn`` needs for B rows of S samples and C channels (host arithmetic)."""
    n = C.c_ulonglong(0)
    check(lib().f5e_w2v_conv0_gn_partials(int(B), int(S), int(C_), C.byref(n)), "f5e_w2v_conv0_gn_partials")
    return int(n.value)


def w2v_conv0_gn(wav: Tensor, w: Tensor, bias: Optional[Tensor], gamma: Tensor, beta: Tensor, lengths: Optional[Tensor],
                 out: Tensor, partials: Tensor, frames: Optional[Tensor] = None, mask: Optional[Tensor] = None,
                 conv_kernels=(), conv_strides=(), eps: float = 1e-5):
    """f5e_w2v_conv0_gn: wav f32 [B, S], w f32 [C, 10] -> out f32 [B, P >= T0, C] (frames C floats apart, rows any stride >=
    T0 C), T0 = (S - 10) // 5 + 1: Conv1d(1 -> C, k 10, stride 5) + GroupNorm(C groups) over each row's own (lengths[b] - 10) //
    5 + 1 frames + GELU, zero from there to T0; frames i32 [B] and mask f32 [B, Tm] as ``wav_norm`` writes them."""
    if wav.ndim != 2 or w.ndim != 2 or w.shape[1] != 10 or out.ndim != 3 or out.shape[0] != wav.shape[0] or out.shape[2] != w.shape[0]:
        raise _C.F5EError(f"w2v_conv0_gn: wav [B, S], w [C, 10], out [B, P, C] (got {tuple(wav.shape)}, {tuple(w.shape)}, {tuple(out.shape)})")
    B, S = wav.shape
    Cc = w.shape[0]
    T0 = (S - 10) // 5 + 1
    if S < 10 or out.shape[1] < T0:
        raise _C.F5EError(f"w2v_conv0_gn: S = {S} samples give {max(T0, 0)} frames; out {tuple(out.shape)} must hold at least one and all of them")
    if not out.is_cuda or out.dtype != F32 or out.stride(2) != 1 or (out.shape[1] > 1 and out.stride(1) != Cc):
        raise _C.F5EError("w2v_conv0_gn: out must be an f32 GPU tensor whose frames are C floats apart")
    bstride = out.stride(0) if B > 1 else max(out.stride(0), T0 * Cc)
    if bstride < T0 * Cc:
        raise _C.F5EError(f"w2v_conv0_gn: the batch stride of out ({bstride}) must cover T0 * C = {T0 * Cc} floats")
    wp, ldw = _rows(wav, (F32,), "w2v_conv0_gn: wav", S, vec=1)
    for t, nm in ((bias, "bias"), (gamma, "gamma"), (beta, "beta")):
        if t is not None and t.numel() != Cc:
            raise _C.F5EError(f"w2v_conv0_gn: {nm} must have C = {Cc} elements")
    if len(conv_kernels) != len(conv_strides) or len(conv_kernels) > 8:
        raise _C.F5EError("w2v_conv0_gn: conv_kernels and conv_strides must have one length, at most 8")
    need = w2v_conv0_gn_partials(B, S, Cc)
    if partials.dtype != F32 or partials.numel() < need:
        raise _C.F5EError(f"w2v_conv0_gn: partials must hold {need} floats (w2v_conv0_gn_partials)")
    if frames is not None and (frames.dtype != I32 or frames.shape != (B,)):
        raise _C.F5EError(f"w2v_conv0_gn: frames must be i32 [{B}]")
    t_mask = 0
    if mask is not None:
        if mask.ndim != 2 or mask.shape[0] != B or not 0 < mask.shape[1] <= S:
            raise _C.F5EError(f"w2v_conv0_gn: mask must be [{B}, 1..{S}] (got {tuple(mask.shape)})")
        t_mask = mask.shape[1]
    n = len(conv_kernels)
    ks, ss = (C.c_int * max(n, 1))(*[int(v) for v in conv_kernels]), (C.c_int * max(n, 1))(*[int(v) for v in conv_strides])
    require_device()
    check(lib().f5e_w2v_conv0_gn(_stream(), wp, ldw, _p(w, F32, "w"), _p(bias, F32, "bias"), _p(gamma, F32, "gamma"),
                                 _p(beta, F32, "beta"), _len(lengths, B, "w2v_conv0_gn"), _p(partials, F32, "partials"),
                                 C.c_void_p(out.data_ptr()), bstride, _p(frames, I32, "frames"), _p(mask, F32, "mask"), t_mask,
                                 ks, ss, n, B, S, Cc, float(eps)), "f5e_w2v_conv0_gn")
    return out


def pack_lstm_weight(w_hh: Tensor) -> Tensor:
    """W_hh f32 [ND, 4 H, H] (PyTorch's ``weight_hh_l0`` and ``weight_hh_l0_reverse`` stacked; gate order i, f, g, o) -> f32
    [ND, H, H / 64, 64, 4] as f5e_lstm_f32 reads it: packed[d, u, j, l, g] = W_hh[d, g H + u, 64 j + l]."""
    if w_hh.ndim != 3 or w_hh.shape[1] != 4 * w_hh.shape[2] or w_hh.shape[0] not in (1, 2) or w_hh.shape[2] % 64 or \
            not 64 <= w_hh.shape[2] <= LSTM_MAX_H:
        raise _C.F5EError(f"pack_lstm_weight: w_hh must be [ND, 4 H, H] with ND 1 or 2 and H a multiple of 64 up to {LSTM_MAX_H} "
                          f"(got {tuple(w_hh.shape)})")
    ND, _, H = w_hh.shape
    return w_hh.detach().to(F32).reshape(ND, 4, H, H // 64, 64).permute(0, 2, 3, 4, 1).contiguous()


def lstm_f32(xg: Tensor, w_hh_packed: Tensor, lengths: Optional[Tensor], out: Tensor, cell: Tensor):
    """f5e_lstm_f32: xg f32 [B * T, >= ND 4 H] (row-strided view; x W_ih^T + b_ih + b_hh of every direction), w_hh_packed from
    ``pack_lstm_weight``, lengths i32 [B] on the device or None, out f32 [B, T, ND H], cell f32 scratch of ND B H elements.
    One launch per time step; packed-sequence semantics, out[b, t >= lengths[b]] = 0."""
    if w_hh_packed.ndim != 5 or w_hh_packed.shape[2:] != (w_hh_packed.shape[1] // 64, 64, 4) or out.ndim != 3 or xg.ndim != 2:
        raise _C.F5EError("lstm_f32: xg [B * T, ND 4 H], w_hh_packed [ND, H, H / 64, 64, 4] (pack_lstm_weight), out [B, T, ND H]; "
                          "there is no CPU path")
    ND, H = w_hh_packed.shape[:2]
    B, T, W = out.shape
    if W != ND * H or xg.shape[0] != B * T or ND not in (1, 2) or H % 64 or not 64 <= H <= LSTM_MAX_H or \
            not 1 <= B <= LSTM_MAX_B or not 1 <= T <= LSTM_MAX_T:
        raise _C.F5EError(f"lstm_f32: out {tuple(out.shape)} / xg {tuple(xg.shape)} do not fit ND = {ND}, H = {H} (H a multiple of "
                          f"64 up to {LSTM_MAX_H}, B <= {LSTM_MAX_B}, 1 <= T <= {LSTM_MAX_T})")
    xp, ldxg = _rows(xg, (F32,), "lstm_f32: xg", ND * 4 * H, vec=1)
    if cell.dtype != F32 or cell.numel() < ND * B * H:
        raise _C.F5EError(f"lstm_f32: cell must hold ND B H = {ND * B * H} floats")
    if w_hh_packed.data_ptr() % 16:
        raise _C.F5EError("lstm_f32: w_hh_packed must be 16-byte aligned")
    require_device()
    check(lib().f5e_lstm_f32(_stream(), xp, ldxg, _p(w_hh_packed, F32, "w_hh_packed"), _len(lengths, B, "lstm_f32"),
                             _p(out, F32, "out"), _p(cell, F32, "cell"), B, T, H, ND), "f5e_lstm_f32")
    return out


def score_mean(hid: Tensor, w2: Tensor, b2: Optional[Tensor], frames: Optional[Tensor], out: Tensor, B: int,
               scale: float = 1.0, offset: float = 0.0, frame_scores: Optional[Tensor] = None):
    """f5e_score_mean: hid f32 [B * T, >= F] (row-strided view), w2 f32 [F], b2 f32 [1] or None, frames i32 [B] on the device or
    None -> out f32 [B] = scale * mean over t < frames[b] of (hid[b T + t] . w2 + b2) + offset; frame_scores f32 [B, T]
    (optional) receives the per-frame values, zero beyond frames[b]."""
    if hid.ndim != 2 or w2.ndim != 1 or B < 1 or hid.shape[0] % B or hid.shape[0] == 0:
        raise _C.F5EError(f"score_mean: hid [B * T, >= F], w2 [F] (got {tuple(hid.shape)}, {tuple(w2.shape)}, B = {B}); there is no "
                          f"CPU path")
    T, F = hid.shape[0] // B, w2.shape[0]
    hp, ldh = _rows(hid, (F32,), "score_mean: hid", F, vec=1)
    if out.shape != (B,) or (b2 is not None and b2.numel() != 1) or (frame_scores is not None and frame_scores.shape != (B, T)):
        raise _C.F5EError(f"score_mean: out [{B}], b2 [1], frame_scores [{B}, {T}]")
    require_device()
    check(lib().f5e_score_mean(_stream(), hp, ldh, _p(w2, F32, "w2"), _p(b2, F32, "b2"), _len(frames, B, "score_mean"),
                               _p(frame_scores, F32, "frame_scores"), _p(out, F32, "out"), B, T, F, float(scale), float(offset)),
          "f5e_score_mean")
    return out


# ---- Paraformer (csrc/paraformer.hip) ----

def _i32(t: Optional[Tensor], n: int, name: str):
    """Pointer of a contiguous i32 GPU tensor with at least ``n`` elements (None stays None)."""
    return _flat(t, I32, name, n)


def lfr_cmvn(fbank: Tensor, count: Optional[Tensor], shift: Tensor, scale: Tensor, pos: Optional[Tensor], out: Tensor,
             frames_out: Optional[Tensor], m: int, n: int, xscale: float = 1.0, win: int = 0, hop: int = 0):
    """f5e_lfr_cmvn_f32: fbank f32 [B, T, n_mels] -> out f32 [B, T', m n_mels] = LFR (m frames stacked every n, (m - 1) // 2 copies
    of frame 0 in front, the last frame repeated behind), (x + shift) * scale, * xscale, + pos[i] (f32 [>= T', m n_mels] or None),
    each step rounded on its own; rows at or beyond ceil(T_b / n) are zero.  ``count`` i32 [B]: frames per row, or with ``hop``
    > 0 SAMPLES per row (T_b = 1 + (count - win) // hop, 0 below ``win``); ``frames_out`` i32 [B] receives ceil(T_b / n)."""
    B, T, n_mels = _shape3(fbank, "lfr_cmvn: fbank")
    W = int(m) * n_mels
    if out.ndim != 3 or out.shape[0] != B or out.shape[2] != W or shift.numel() != W or scale.numel() != W or \
            (pos is not None and (pos.ndim != 2 or pos.shape[1] != W)):
        raise _C.F5EError(f"lfr_cmvn: out [{B}, T', {W}], shift / scale [{W}], pos [>= T', {W}] (got {tuple(out.shape)}, "
                          f"{tuple(shift.shape)}, {tuple(scale.shape)}, {None if pos is None else tuple(pos.shape)})")
    require_device()
    check(lib().f5e_lfr_cmvn_f32(_stream(), _p(fbank, F32, "fbank"), _i32(count, B, "lfr_cmvn: count"), int(win), int(hop),
                                 _p(shift, F32, "shift"), _p(scale, F32, "scale"), _p(pos, F32, "pos"),
                                 0 if pos is None else pos.shape[0], _p(out, F32, "out"), _i32(frames_out, B, "lfr_cmvn: frames_out"),
                                 B, T, out.shape[1], n_mels, int(m), int(n), float(xscale)), "f5e_lfr_cmvn_f32")
    return out


def fsmn(x: Tensor, w_t: Tensor, lengths: Optional[Tensor], out: Tensor, B: int, left: int, addend: Optional[Tensor] = None):
    """f5e_fsmn_f32: the masked depthwise memory block.  x f32 [B * T, C] (a row-strided view, e.g. the v third of q | k | v),
    w_t f32 [K, C], out / addend f32 [B * T, C] views (out may be addend, not x): out = conv_K(x masked) + x (+ addend) at
    t < lengths[b]; addend (or zero) beyond."""
    if x.ndim != 2 or w_t.ndim != 2 or B < 1 or x.shape[0] % B or x.shape[0] == 0 or w_t.shape[1] != x.shape[1] or \
            out.shape != x.shape or (addend is not None and addend.shape != x.shape):
        raise _C.F5EError(f"fsmn: x / out / addend [B * T, C], w_t [K, C] (got {tuple(x.shape)}, {tuple(out.shape)}, "
                          f"{tuple(w_t.shape)}, B = {B}); there is no CPU path")
    M, Cc = x.shape
    xp, ldx = _rows(x, (F32,), "fsmn: x", Cc)
    op, ldo = _rows(out, (F32,), "fsmn: out", Cc)
    ap, lda = (None, 0) if addend is None else _rows(addend, (F32,), "fsmn: addend", Cc)
    require_device()
    check(lib().f5e_fsmn_f32(_stream(), xp, ldx, _p(w_t, F32, "w_t"), _len(lengths, B, "fsmn"), ap, lda, op, ldo, B, M // B, Cc,
                             w_t.shape[0], int(left)), "f5e_fsmn_f32")
    return out


def mask_rows(x: Tensor, lengths: Tensor, B: int):
    """f5e_mask_rows_f32: rows t >= lengths[b] of x f32 [B * T, C] (row-strided view) become zero, in place."""
    if x.ndim != 2 or B < 1 or x.shape[0] % B or x.shape[0] == 0:
        raise _C.F5EError(f"mask_rows: x [B * T, C] (got {tuple(x.shape)}, B = {B})")
    xp, ldx = _rows(x, (F32,), "mask_rows: x", x.shape[1], vec=1)
    require_device()
    check(lib().f5e_mask_rows_f32(_stream(), xp, ldx, _len(lengths, B, "mask_rows"), B, x.shape[0] // B, x.shape[1]),
          "f5e_mask_rows_f32")
    return x


def cif_alpha(logits: Tensor, lengths: Optional[Tensor], alpha: Tensor, n_out: Tensor, smooth: float = 1.0, noise: float = 0.0,
              tail: float = 0.45):
    """f5e_cif_alpha_f32: logits f32 [B, T] (contiguous) -> alpha f32 [B, T + 1] = relu(sigmoid * smooth - noise) at t < lengths[b],
    ``tail`` at t = lengths[b], zero beyond; n_out i32 [B] = floor(sum alpha)."""
    if logits.ndim != 2 or alpha.shape != (logits.shape[0], logits.shape[1] + 1):
        raise _C.F5EError(f"cif_alpha: logits [B, T], alpha [B, T + 1] (got {tuple(logits.shape)}, {tuple(alpha.shape)})")
    B, T = logits.shape
    require_device()
    check(lib().f5e_cif_alpha_f32(_stream(), _p(logits, F32, "logits"), 1, _len(lengths, B, "cif_alpha"), _p(alpha, F32, "alpha"),
                                  T + 1, _i32(n_out, B, "cif_alpha: n_out"), B, T, float(smooth), float(noise), float(tail)),
          "f5e_cif_alpha_f32")
    return alpha, n_out


def cif_fire_scratch(B: int, T: int, L_cap: int) -> int:
    """Floats of scratch ``cif_fire`` needs: cur [B, T + 1] | pos [B, L_cap] (i32) | rem [B, L_cap]."""
    return B * (T + 1) + 2 * B * L_cap


def cif_fire(alpha: Tensor, h: Tensor, lengths: Optional[Tensor], out: Tensor, count: Tensor, scratch: Tensor,
             n_limit: Optional[Tensor] = None, threshold: float = 1.0):
    """f5e_cif_fire_f32: alpha f32 [B, T + 1] (``cif_alpha``), h f32 [B * T, D] (row-strided view) -> out f32 [B, L_cap, D]: the
    emitted frames of the sequential integrate-and-fire loop, bit for bit; token k >= min(count[b], L_cap, n_limit[b]) is zero.
    count i32 [B] = all fires of the row.  scratch f32 [>= cif_fire_scratch(B, T, L_cap)]; afterwards it holds cur | pos | rem."""
    if alpha.ndim != 2 or h.ndim != 2 or out.ndim != 3 or out.shape[0] != alpha.shape[0] or out.shape[2] != h.shape[1] or \
            h.shape[0] != alpha.shape[0] * (alpha.shape[1] - 1) or h.shape[0] == 0:
        raise _C.F5EError(f"cif_fire: alpha [B, T + 1], h [B * T, D], out [B, L_cap, D] (got {tuple(alpha.shape)}, {tuple(h.shape)}, "
                          f"{tuple(out.shape)}); there is no CPU path")
    B, T, Lc, D = alpha.shape[0], alpha.shape[1] - 1, out.shape[1], h.shape[1]
    hp, ldh = _rows(h, (F32,), "cif_fire: h", D, vec=1)
    _flat(scratch, F32, "cif_fire: scratch", cif_fire_scratch(B, T, Lc))
    _p(scratch, F32, "cif_fire: scratch")
    base, fb = scratch.data_ptr(), 4
    cur, pos, rem = base, base + fb * B * (T + 1), base + fb * (B * (T + 1) + B * Lc)
    require_device()
    check(lib().f5e_cif_fire_f32(_stream(), _p(alpha, F32, "alpha"), T + 1, hp, ldh, _len(lengths, B, "cif_fire"),
                                 _len(n_limit, B, "cif_fire"), C.c_void_p(cur), C.c_void_p(pos), C.c_void_p(rem),
                                 _i32(count, B, "cif_fire: count"), _p(out, F32, "out"), D, B, T, D, Lc, float(threshold)),
          "f5e_cif_fire_f32")
    return out, count


def nar_pick(logits: Tensor, n: Optional[Tensor], B: int, arg: Tensor, logp: Tensor, ids: Tensor, length: Tensor, score: Tensor,
             sos: int = 1, eos: int = 2, blank: int = 0, pad: int = -1):
    """f5e_nar_pick: logits f32 [B * L, V] (row-strided view) -> arg i32 [B * L] (argmax, lowest index on ties; -1 at k >= n[b]),
    logp f32 [B * L] (its log-softmax value), ids i32 [B, L] (the args of k < n[b] other than sos / eos / blank, compacted,
    padded with ``pad``), length i32 [B], score f32 [B] = sum of logp over k < n[b]."""
    if logits.ndim != 2 or B < 1 or logits.shape[0] % B or logits.shape[0] == 0:
        raise _C.F5EError(f"nar_pick: logits [B * L, V] (got {tuple(logits.shape)}, B = {B}); there is no CPU path")
    R, V = logits.shape
    L = R // B
    lp_, ld = _rows(logits, (F32,), "nar_pick: logits", V, vec=1)
    if ids.shape != (B, L):
        raise _C.F5EError(f"nar_pick: ids must be [{B}, {L}]")
    require_device()
    check(lib().f5e_nar_pick(_stream(), lp_, ld, _len(n, B, "nar_pick"), _i32(arg, R, "nar_pick: arg"),
                             _flat(logp, F32, "nar_pick: logp", R), _p(ids, I32, "ids"), _i32(length, B, "nar_pick: length"),
                             _flat(score, F32, "nar_pick: score", B), B, L, V, int(sos), int(eos), int(blank), int(pad)),
          "f5e_nar_pick")
    return ids, length, score


def dit_forward(plan: "_C.DitPlan"):
    require_device()
    check(lib().f5e_dit_forward(_stream(), C.byref(plan)), "f5e_dit_forward")


class Graph:
    """hipGraph captured through the C ABI on the current (non-default) torch stream.

    An executable graph owns the kernel-argument storage of its nodes, so it must outlive the launches that are still
    queued: ``retire()`` parks it behind an event recorded on the launch stream and ``reap()`` destroys the parked
    graphs whose event has completed (callers never block on the GPU for this)."""

    _parked = []
    _parked_lock = threading.Lock()

    def __init__(self):
        self.handle = C.c_void_p()

    def retire(self):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        with Graph._parked_lock:
            Graph._parked.append((self, ev))

    @staticmethod
    def reap():
        with Graph._parked_lock:
            state = [(x, x[1].query()) for x in Graph._parked]    # ONE query per event: it may complete in between
            done = [x for x, finished in state if finished]
            Graph._parked[:] = [x for x, finished in state if not finished]
        for g, _ in done:
            g.destroy()

    def destroy(self):
        if self.handle:
            lib().f5e_graph_destroy(self.handle)
            self.handle = C.c_void_p()

    def begin(self):
        require_device()
        check(lib().f5e_graph_begin(_stream()), "f5e_graph_begin")

    def end(self):
        check(lib().f5e_graph_end(_stream(), C.byref(self.handle)), "f5e_graph_end")

    def launch(self):
        check(lib().f5e_graph_launch(self.handle, _stream()), "f5e_graph_launch")

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# ---- the Qwen2 chat model's kernels (csrc/llm.hip) ----

LLM_MAX_TOP_K = 64
LLM_MAX_POS = 4096


def rmsnorm_f32(x: Tensor, w: Tensor, eps: float, out: Optional[Tensor] = None) -> Tensor:
    """out[m] = (x[m] * rsqrt(mean(x[m]^2) + eps)) * w (f5e_rmsnorm_f32): x, out f32 [M, >= D] row-strided views (row strides
    multiples of 4, 16-byte aligned; out may be x), w f32 [D], D a multiple of 4, at most 8192.  One wave per row."""
    if not isinstance(x, Tensor) or x.ndim != 2 or w.ndim != 1:
        raise _C.F5EError("rmsnorm_f32: x [M, D] and w [D]; there is no CPU path")
    M, D = x.shape[0], w.shape[0]
    xp, ldx = _rows(x, (F32,), "rmsnorm_f32: x", D)
    out = torch.empty(M, D, dtype=F32, device=x.device) if out is None else out
    if out.ndim != 2 or out.shape[0] != M:
        raise _C.F5EError(f"rmsnorm_f32: out must be [{M}, >= {D}]")
    op, ldo = _rows(out, (F32,), "rmsnorm_f32: out", D)
    require_device()
    check(lib().f5e_rmsnorm_f32(_stream(), xp, ldx, _vec(w, F32, "rmsnorm_f32: w", (D,), align=16), op, ldo, M, D, float(eps)),
          "f5e_rmsnorm_f32")
    return out


def swiglu_f32(gu: Tensor, out: Optional[Tensor] = None, I: Optional[int] = None) -> Tensor:
    """out[m, i] = silu(gu[m, i]) * gu[m, I + i] (f5e_swiglu_f32): gu f32 [M, >= 2 I] (gate | up), out f32 [M, >= I]."""
    if not isinstance(gu, Tensor) or gu.ndim != 2:
        raise _C.F5EError("swiglu_f32: gu [M, 2 I]; there is no CPU path")
    M = gu.shape[0]
    I = gu.shape[1] // 2 if I is None else int(I)
    gp, ld = _rows(gu, (F32,), "swiglu_f32: gu", 2 * I)
    out = torch.empty(M, I, dtype=F32, device=gu.device) if out is None else out
    if out.ndim != 2 or out.shape[0] != M:
        raise _C.F5EError(f"swiglu_f32: out must be [{M}, >= {I}]")
    op, ldo = _rows(out, (F32,), "swiglu_f32: out", I)
    require_device()
    check(lib().f5e_swiglu_f32(_stream(), gp, ld, op, ldo, M, I), "f5e_swiglu_f32")
    return out


def llm_embed(ids: Tensor, emb: Tensor, out: Tensor) -> Tensor:
    """out[i] = emb[ids[i]], widened exactly (f5e_llm_embed_f32 / f5e_llm_embed_w16 by ``emb.dtype``): ids i32 [n] on the device
    (clamped to the table; the decode step passes ``last``), emb f32 / fp16 / bf16 [V, D], out f32 [n, D], contiguous."""
    if not isinstance(ids, Tensor) or ids.ndim != 1 or emb.ndim != 2 or out.ndim != 2:
        raise _C.F5EError("llm_embed: ids [n], emb [V, D] and out [n, D]; there is no CPU path")
    n, (V, D) = ids.shape[0], emb.shape
    if n < 1 or tuple(out.shape) != (n, D) or D % 4:
        raise _C.F5EError(f"llm_embed: ids {tuple(ids.shape)}, emb {tuple(emb.shape)}, out {tuple(out.shape)}: out must be [n, D] "
                          f"and D a multiple of 4")
    if emb.dtype != F32 and emb.dtype not in W16_TYPES:
        raise _C.F5EError(f"llm_embed: emb must be f32, fp16 or bf16 (got {emb.dtype})")
    for t, nm in ((emb, "emb"), (out, "out")):
        if t.is_cuda and t.data_ptr() % (8 if t.dtype in W16_TYPES else 16):
            raise _C.F5EError(f"llm_embed: {nm} must be 16-byte aligned (a 16-bit emb: 8-byte)")
    ip, ep, op = _p(ids, I32, "llm_embed: ids"), _p(emb, None, "llm_embed: emb"), _p(out, F32, "llm_embed: out")
    require_device()
    if emb.dtype == F32:
        check(lib().f5e_llm_embed_f32(_stream(), ip, ep, op, n, D, V), "f5e_llm_embed_f32")
    else:
        check(lib().f5e_llm_embed_w16(_stream(), ip, ep, W16_TYPES[emb.dtype], op, n, D, V), "f5e_llm_embed_w16")
    return out


def _gqa_common(name: str, qkv: Tensor, kc: Tensor, vc: Tensor, cos: Tensor, sin: Tensor, heads: int, kv_heads: int, rows: int,
                begin: Optional[Tensor], out: Optional[Tensor]):
    if not isinstance(qkv, Tensor) or qkv.ndim != 2 or kc.ndim != 3 or kc.shape != vc.shape or kc.stride() != vc.stride():
        raise _C.F5EError(f"{name}: qkv [rows, >= (H + 2 Hkv) dk] and kc, vc [R, P, Hkv dk] with equal strides; there is no CPU path")
    R, P, Dkv = kc.shape
    for t, nm in ((kc, "kc"), (vc, "vc")):
        if not t.is_cuda or t.dtype != F32 or t.stride(2) != 1:
            raise _C.F5EError(f"{name}: {nm} must be an f32 GPU tensor with unit channel stride")
    heads, kv_heads = int(heads), int(kv_heads)
    if kv_heads < 1 or heads % kv_heads or Dkv % kv_heads:
        raise _C.F5EError(f"{name}: kv_heads = {kv_heads} must divide heads = {heads} and the caches' {Dkv} channels")
    dk = Dkv // kv_heads
    D = heads * dk
    if cos.ndim != 2 or cos.shape != sin.shape or cos.shape[1] != dk // 2 or cos.shape[0] < P:
        raise _C.F5EError(f"{name}: cos, sin must be f32 [>= {P}, {dk // 2}] (got {tuple(cos.shape)}, {tuple(sin.shape)})")
    pos_stride = kc.stride(1) if P > 1 else max(Dkv, kc.stride(1))
    row_stride = kc.stride(0) if R > 1 else max(kc.stride(0), (P - 1) * pos_stride + Dkv)
    for t in (kc, vc):
        have = t.untyped_storage().nbytes() // 4 - t.storage_offset()
        if pos_stride < Dkv or row_stride < (P - 1) * pos_stride + Dkv or have < (R - 1) * row_stride + (P - 1) * pos_stride + Dkv \
                or pos_stride % 4 or row_stride % 4 or t.data_ptr() % 16:
            raise _C.F5EError(f"{name}: cache strides ({row_stride}, {pos_stride}) must be multiples of 4 spanning "
                              f"[{R}, {P}, {Dkv}] inside the storage, kc and vc 16-byte aligned")
    if qkv.shape[0] != rows * R:
        raise _C.F5EError(f"{name}: qkv has {qkv.shape[0]} rows, {R} * {rows} are needed")
    qp, ldq = _rows(qkv, (F32,), f"{name}: qkv", D + 2 * Dkv)
    bp = None if begin is None else _vec(begin, I32, f"{name}: begin", (R,))
    cp = _vec(cos, F32, f"{name}: cos", cos.shape, align=16)
    sp = _vec(sin, F32, f"{name}: sin", sin.shape, align=16)
    out = torch.empty(R * rows, D, dtype=F32, device=qkv.device) if out is None else out
    if out.ndim != 2 or tuple(out.shape) != (R * rows, D):
        raise _C.F5EError(f"{name}: out must be [{R * rows}, {D}]")
    op, ldo = _rows(out, (F32,), f"{name}: out", D)
    require_device()
    front = (_stream(), qp, ldq, C.c_void_p(kc.data_ptr()), C.c_void_p(vc.data_ptr()), row_stride, pos_stride, bp, cp, sp,
             cos.shape[0], op, ldo, R)
    return front, out, P, dk


def gqa_rope_append_f32(qkv: Tensor, kc: Tensor, vc: Tensor, cos: Tensor, sin: Tensor, U: int, p0: int, heads: int, kv_heads: int,
                        scale: float, begin: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """Causal attention of U new positions behind p0 cached ones with rotary positions and grouped heads
    (f5e_gqa_rope_append_f32): qkv f32 [R * U, >= (H + 2 Hkv) dk] packed q | k | v, kc / vc f32 [R, Umax, Hkv dk] views of the
    layer's caches, cos / sin f32 [>= Umax, dk / 2], begin i32 [R] on the device or None -> out f32 [R * U, H dk].  Slots
    [r, p0:p0 + U] receive the rotated keys and the values; nothing else is written, nothing at or beyond p0 is read."""
    U, p0 = int(U), int(p0)
    if U < 1 or p0 < 0 or kc.ndim != 3 or p0 + U > kc.shape[1]:
        raise _C.F5EError(f"gqa_rope_append_f32: need U = {U} >= 1 new positions from p0 = {p0} >= 0 inside the cached ones")
    front, out, P, dk = _gqa_common("gqa_rope_append_f32", qkv, kc, vc, cos, sin, heads, kv_heads, U, begin, out)
    check(lib().f5e_gqa_rope_append_f32(*front, U, P, int(heads), int(kv_heads), dk, p0, float(scale)), "f5e_gqa_rope_append_f32")
    return out


def gqa_rope_decode_dev_f32(qkv: Tensor, kc: Tensor, vc: Tensor, cos: Tensor, sin: Tensor, rec: Tensor, heads: int, kv_heads: int,
                            scale: float, begin: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """One position from the step record (f5e_gqa_rope_decode_dev_f32): qkv f32 [R, >= (H + 2 Hkv) dk], kc / vc f32
    [R, P, Hkv dk], rec i32 [8] on the device -> out f32 [R, H dk].  p = rec[0] clamped to [0, P - 1]; slot [r, p] receives the
    step's rotated key and its value.  The launch does not depend on p."""
    front, out, P, dk = _gqa_common("gqa_rope_decode_dev_f32", qkv, kc, vc, cos, sin, heads, kv_heads, 1, begin, out)
    check(lib().f5e_gqa_rope_decode_dev_f32(*front, P, int(heads), int(kv_heads), dk, _rec(rec, "gqa_rope_decode_dev_f32"),
                                            float(scale)), "f5e_gqa_rope_decode_dev_f32")
    return out


def llm_pick_dev(logits: Tensor, tokens: Tensor, last: Tensor, done: Tensor, alive: Tensor, rec: Tensor, *, eos, pad: int,
                 do_sample: bool = False, penalty: float = 1.0, temperature: float = 1.0, top_k: int = 1, top_p: float = 1.0,
                 begin: Optional[Tensor] = None, row_key: Optional[Tensor] = None, serial: Optional[Tensor] = None,
                 keep_id: Optional[Tensor] = None, keep_p: Optional[Tensor] = None, keep_n: Optional[Tensor] = None,
                 V: Optional[int] = None) -> Tensor:
    """f5e_llm_pick_dev: repetition penalty over tokens[r, begin[r]:p + 1], then the arg max (``do_sample`` False) or
    temperature, top-k, top-p and an inverse-CDF draw keyed by (seed, row_key[r], serial[r], p), at the step record's position;
    then ``alive`` and p += 1.  ``eos``: up to 4 ids; a done row writes ``pad``.  keep_id i32 / keep_p f32 [R, 64], keep_n i32
    [R]: the survivors, for the parity tests."""
    if not isinstance(logits, Tensor) or logits.ndim != 2 or tokens.ndim != 2 or tokens.shape[0] != logits.shape[0]:
        raise _C.F5EError("llm_pick_dev: logits [R, >= V] and tokens [R, >= 2]; there is no CPU path")
    R = logits.shape[0]
    V = logits.shape[1] if V is None else int(V)
    if V > logits.shape[1]:
        raise _C.F5EError(f"llm_pick_dev: V = {V} exceeds the {logits.shape[1]} columns of logits")
    if last.shape != (R,) or done.shape != (R,) or alive.numel() != 1:
        raise _C.F5EError(f"llm_pick_dev: last [{R}], done [{R}], alive [1]")
    eos = [int(e) for e in ([eos] if isinstance(eos, int) else eos)]
    if len(eos) > 4:
        raise _C.F5EError(f"llm_pick_dev: at most 4 eos ids (got {len(eos)})")
    lp, ld = _rows(logits, (F32,), "llm_pick_dev: logits", max(V, 1), vec=1)
    tp, ld_tok = _rows(tokens, (I32,), "llm_pick_dev: tokens", 2, vec=1)
    bp = None if begin is None else _vec(begin, I32, "llm_pick_dev: begin", (R,))
    if do_sample and (row_key is None or serial is None or row_key.shape != (R,) or serial.shape != (R,)):
        raise _C.F5EError(f"llm_pick_dev: sampling needs row_key [{R}] and serial [{R}]")
    kid = None if keep_id is None else _vec(keep_id, I32, "llm_pick_dev: keep_id", (R, LLM_MAX_TOP_K))
    kp = None if keep_p is None else _vec(keep_p, F32, "llm_pick_dev: keep_p", (R, LLM_MAX_TOP_K))
    kn = None if keep_n is None else _vec(keep_n, I32, "llm_pick_dev: keep_n", (R,))
    eos_arr = (C.c_int * max(len(eos), 1))(*eos)
    require_device()
    check(lib().f5e_llm_pick_dev(_stream(), lp, ld, tp, ld_tok, tokens.shape[1], bp, _p(last, I32, "last"), _p(done, I32, "done"),
                                 _p(alive, I32, "alive"), R, V, _rec(rec, "llm_pick_dev"), 1 if do_sample else 0, float(penalty),
                                 float(temperature), int(top_k), float(top_p), C.cast(eos_arr, C.c_void_p), len(eos), int(pad),
                                 _p(row_key, I32, "row_key"), _p(serial, I32, "serial"), kid, kp, kn), "f5e_llm_pick_dev")
    return last
