"""The fp32 transformer layer of the speech models (WavLM, wav2vec2, Whisper, the wenet attention decoder), written once, and
the scratch plan their ``extract`` / ``predict`` calls share.

``layer`` issues   LayerNorm -> q|k|v GEMM -> self_attn -> out-projection + residual
                   [-> LayerNorm -> q GEMM -> cross_attn -> out-projection + residual]
                   -> LayerNorm -> FF1 + activation -> FF2 + residual
(``pre_norm``) or the same GEMMs with each LayerNorm in place BEHIND its residual (post-norm: x = LN(x + f(x))).  The attention
launches are the caller's: two callables, built once per ``extract`` call or decode state."""
from __future__ import annotations

import math
from typing import Any, Dict, NamedTuple, Optional, Tuple

import torch

from . import _C, ops

Tensor = torch.Tensor
F32 = torch.float32
Pair = Tuple[Tensor, Optional[Tensor]]


class LayerWeights(NamedTuple):
    """One layer as the kernels take it; every pair is (weight, bias).  ``ln_x`` .. ``xout`` are None without source attention:
    ``xq`` projects the layer's queries, ``xkv`` = k | v of the memory, which the CALLER projects (once per utterance or, in
    ``cross_attn``, per layer).  ``extra`` is the model's own (WavLM: w_gate, b_gate, const)."""
    ln1: Pair
    qkv: Pair
    out: Pair
    ln_x: Optional[Pair]
    xq: Optional[Pair]
    xkv: Optional[Pair]
    xout: Optional[Pair]
    ln_ff: Pair
    ff: Tuple[Tensor, Tensor, Tensor, Tensor]
    extra: Any = None


def _pair(m) -> Pair:
    """(weight, bias) of an ``nn.Linear`` / ``nn.LayerNorm`` holder, or the pair itself."""
    return m if isinstance(m, tuple) else (m.weight, m.bias)


def stack(dev, *ms, wdtype=None) -> Pair:
    """Row-wise q | k | v (or k | v) of holders or (weight, bias) pairs on ``dev``: ONE weight tensor (f32, or ``wdtype``) and
    one f32 bias; a missing bias (None) is zeros."""
    ws, bs = zip(*(_pair(m) for m in ms))
    have = next(b for b in bs if b is not None)
    return fold(dev, (torch.cat(ws, 0), torch.cat([have.new_zeros(w.shape[0]) if b is None else b for w, b in zip(ws, bs)], 0)),
                wdtype=wdtype)


def fold(dev, m, wdtype=None) -> Pair:
    """(weight, bias) on ``dev``: f32, or with ``wdtype`` (torch.float16 / torch.bfloat16) the weight in that type, rounded to
    nearest-even where it does not hold the value, for a ``gemm`` hook that reads 16-bit weights (``layer``).  The bias is f32
    either way; LayerNorm pairs are folded without ``wdtype``."""
    w, b = _pair(m)
    return w.detach().to(dev, F32 if wdtype is None else wdtype).contiguous(), b.detach().to(dev, F32).contiguous()


def fold_layer(dev, ln1, q, k, v, out, ln_ff, fc1, fc2, *, ln_x=None, xq=None, xk=None, xv=None, xout=None,
               extra=None, wdtype=None) -> LayerWeights:
    """The record from ``nn.Linear`` / ``nn.LayerNorm`` holders or (weight, bias) pairs.  ``wdtype``: the matrices' type (None:
    f32); biases and LayerNorm pairs stay f32."""
    cross, wd = ln_x is not None, wdtype
    return LayerWeights(ln1=fold(dev, ln1), qkv=stack(dev, q, k, v, wdtype=wd), out=fold(dev, out, wd),
                        ln_x=fold(dev, ln_x) if cross else None, xq=fold(dev, xq, wd) if cross else None,
                        xkv=stack(dev, xk, xv, wdtype=wd) if cross else None, xout=fold(dev, xout, wd) if cross else None,
                        ln_ff=fold(dev, ln_ff), ff=fold(dev, fc1, wd) + fold(dev, fc2, wd), extra=extra)


def layer(src: Tensor, dst: Tensor, W: LayerWeights, bufs: tuple, *, pre_norm: bool, act: int, eps: float, self_attn,
          cross_attn=None, gemm=None) -> None:
    """One layer from ``src`` [M, D] into ``dst`` (may be ``src``) on the scratch ``bufs`` = (xn [M, D], qkv [M, 3 D], ao [M, D],
    q [M, D], ff [M, FF]); xn is unused post-norm, q without source attention.  ``self_attn(W, h, qkv, ao)``: the attention
    launch(es) on q | k | v = ``qkv`` into ``ao``; h is the projection's input (WavLM's gate reads it, with ``W.extra``).
    ``cross_attn(W, q, ao)``: the source attention of the queries ``q`` (``W.xkv`` for a caller that projects the memory per
    layer).  ``gemm``: a replacement for ``ops.gemm_f32`` with its keywords ``out``, ``act`` and ``addend`` (a pass of a handful
    of rows hands in ``ops.gemm_f32_skinny``; a record folded with ``wdtype`` needs one that reads 16-bit weights); None takes
    the path it always took.  Allocates nothing."""
    xn, qkv, ao, q, ff = bufs
    gemm, ln = ops.gemm_f32 if gemm is None else gemm, ops.layernorm
    h = src
    if pre_norm:
        h = ln(src, xn, W.ln1[0], W.ln1[1], eps=eps)
    gemm(h, W.qkv[0], W.qkv[1], out=qkv)
    self_attn(W, h, qkv, ao)
    gemm(ao, W.out[0], W.out[1], out=dst, addend=src)
    h = dst
    if not pre_norm:
        ln(dst, dst, W.ln1[0], W.ln1[1], eps=eps)
    if cross_attn is not None:
        if pre_norm:
            h = ln(dst, xn, W.ln_x[0], W.ln_x[1], eps=eps)
        gemm(h, W.xq[0], W.xq[1], out=q)
        cross_attn(W, q, ao)
        gemm(ao, W.xout[0], W.xout[1], out=dst, addend=dst)
        h = dst
        if not pre_norm:
            ln(dst, dst, W.ln_x[0], W.ln_x[1], eps=eps)
    if pre_norm:
        h = ln(dst, xn, W.ln_ff[0], W.ln_ff[1], eps=eps)
    gemm(h, W.ff[0], W.ff[1], out=ff, act=act)
    gemm(ff, W.ff[2], W.ff[3], out=dst, addend=dst)
    if not pre_norm:
        ln(dst, dst, W.ln_ff[0], W.ln_ff[1], eps=eps)


# ---- the scratch plan ---------------------------------------------------------------------------------------------------------
def plan(shapes: Dict[str, tuple]) -> Dict[str, tuple]:
    """name -> (offset in floats, shape) in the order of ``shapes``, offsets multiples of 64 floats; "_total" -> (floats, ())."""
    out, off = {}, 0
    for name, shape in shapes.items():
        out[name] = (off, shape)
        off += (math.prod(shape) + 63) // 64 * 64
    out["_total"] = (off, ())
    return out


def take(workspace: Optional[Tensor], total: int, dev, who: str) -> Tensor:
    """``total`` floats of scratch: the caller's ``workspace`` as f32 (refused unless it fits), or a new tensor."""
    if workspace is None:
        return torch.empty(total, dtype=F32, device=dev)
    if not workspace.is_cuda or workspace.dtype not in (F32, torch.uint8) or not workspace.is_contiguous() or \
            workspace.data_ptr() % 16 or workspace.numel() * workspace.element_size() < total * 4:
        raise _C.F5EError(f"{who}: workspace must be a contiguous 16-byte aligned f32 / uint8 GPU tensor of at least "
                          f"{total * 4} bytes (workspace_bytes)")
    ws = workspace.view(-1)
    return ws[: ws.numel() // 4 * 4].view(F32) if ws.dtype == torch.uint8 else ws


def view(ws: Tensor, plan_: Dict[str, tuple], name: str) -> Tensor:
    off, shape = plan_[name]
    return ws[off:off + math.prod(shape)].view(shape)
