"""Monotonic alignment search mirror (reference durpred/monotonic_align/__init__.py): ``maximum_path`` with the reference's
signature and return value, and ``maximum_path_index``, the compact form it is expanded from.  The search is
``ops.mas_path`` (csrc/mas.hip) on the device: no copy of the matrix to the host, no loop over utterances."""
from __future__ import annotations

from typing import Tuple, Union

import torch

from .. import _C, ops

Tensor = torch.Tensor
I32 = torch.int32
Lengths = Union[Tensor, list, tuple]


def check_lengths(t_y: Lengths, t_x: Lengths, B: int, Ty: int, Tx: int) -> Tuple[Tensor, Tensor]:
    """[B] tensors where they were.  Lengths that start on the host are validated there (no sync), each against everything
    that is known on the host: a sequence without a monotonic path is a caller bug there, not a row of -1.  Device lengths
    are used as they are (the kernel defines the degenerate rows)."""
    out = []
    for name, t in (("t_y", t_y), ("t_x", t_x)):
        if not isinstance(t, Tensor):
            t = torch.as_tensor(t)
        if t.numel() != B:
            raise _C.F5EError(f"maximum_path: {name} needs one entry per sequence ({B}), got {t.numel()}")
        out.append(t.reshape(B))
    ty, tx = out
    # every check that needs host values only: a device length takes no part (no sync), the other one is still checked
    host_y, host_x = ty.device.type == "cpu", tx.device.type == "cpu"
    ok = torch.ones(B, dtype=torch.bool)
    if host_x:
        ok &= (tx >= 1) & (tx <= Tx) & (tx <= Ty)
    if host_y:
        ok &= (ty >= 1) & (ty <= Ty)
    if host_x and host_y:
        ok &= tx <= ty
    if not bool(ok.all()):
        i = int((~ok).nonzero()[0])
        shown = [str(int(t[i])) if h else "(on the device)" for t, h in ((ty, host_y), (tx, host_x))]
        raise _C.F5EError(f"maximum_path: sequence {i} has t_y = {shown[0]}, t_x = {shown[1]}; need "
                          f"1 <= t_x <= t_y <= {Ty} and t_x <= {Tx}")
    return ty, tx


def maximum_path_index(neg_cent: Tensor, t_y: Lengths, t_x: Lengths) -> Tuple[Tensor, Tensor]:
    """neg_cent f32 [B, Ty, Tx] (frame x token) on the GPU; t_y / t_x: frames / tokens per sequence (device or host) ->
    (token_of_frame i32 [B, Ty], -1 past t_y;  durations i32 [B, Tx], 0 past t_x).  neg_cent is not modified."""
    if not isinstance(neg_cent, Tensor) or neg_cent.ndim != 3:
        raise _C.F5EError("maximum_path: neg_cent must be a [B, Ty, Tx] tensor")
    B, Ty, Tx = neg_cent.shape
    ty, tx = check_lengths(t_y, t_x, B, Ty, Tx)
    if not neg_cent.is_cuda:
        raise _C.F5EError(f"maximum_path: neg_cent must live on the GPU (got {neg_cent.device}); there is no CPU path")
    ty, tx = (t.to(device=neg_cent.device, dtype=I32).contiguous() for t in (ty, tx))
    logp = neg_cent.detach()
    if logp.dtype != torch.float32:
        logp = logp.float()      # the reference searches in float32 whatever the input (astype(float32))
    if logp.stride(2) != 1:
        logp = logp.contiguous()
    tok = torch.empty(B, Ty, dtype=I32, device=logp.device)
    dur = torch.empty(B, Tx, dtype=I32, device=logp.device)
    ops.mas_path(logp, ty, tx, tok, dur)
    return tok, dur


def dense_path(token_of_frame: Tensor, Tx: int, dtype=torch.float32) -> Tensor:
    """token_of_frame [B, Ty] (-1 = no token) -> path [B, Ty, Tx] of 0 / 1 (index work with torch on the device)."""
    cols = torch.arange(Tx, device=token_of_frame.device, dtype=token_of_frame.dtype)
    return (token_of_frame.unsqueeze(-1) == cols).to(dtype)


def maximum_path(neg_cent: Tensor, mask: Tensor) -> Tensor:
    """Reference signature: neg_cent [B, Ty, Tx], mask [B, Ty, Tx] (outer product of the two padding masks) -> dense path
    of neg_cent's shape and dtype.  The lengths are taken from the mask as the reference takes them (column 0 summed over
    frames, row 0 summed over tokens), on the device."""
    if not isinstance(neg_cent, Tensor) or not neg_cent.is_cuda:
        raise _C.F5EError("maximum_path: neg_cent must live on the GPU; there is no CPU path")
    mask = mask.to(neg_cent.device)
    t_y = mask.sum(1)[:, 0].to(I32)
    t_x = mask.sum(2)[:, 0].to(I32)
    tok, _ = maximum_path_index(neg_cent, t_y, t_x)
    return dense_path(tok, neg_cent.shape[2], neg_cent.dtype)
