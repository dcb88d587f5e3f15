"""ECAPA-TDNN speaker encoder of the SIM metric (mirror of reference eval/ecapa_tdnn.py), the half the reference owns: from the
stack of WavLM hidden states to the embedding.  The WavLM-large upstream (s3prl through ``torch.hub`` in the reference) is
``eval/wavlm.py``; ``forward`` takes its hidden states, ``embed_wavs`` takes an upstream callable (a ``WavLM`` instance is one).

Same parameter and buffer names as the reference head (``feature_weight``, ``layer1.conv.weight``,
``layer2.Res2Conv1dReluBn.convs.0.weight``, ``...bns.0.running_var``, ``layer2.SE_Connect.linear1.weight``,
``pooling.linear1.weight``, ``bn.*``, ``linear.*``), so ``load_state_dict(ckpt["model"], strict=False)`` works on a reference
checkpoint (its ``feature_extract.*`` keys are reported as unexpected and ignored).  The sub-modules only HOLD the weights:
the computation is csrc/ecapa.hip + f5e_gemm_f32, eval mode only (BatchNorm on its running statistics, folded
into the GEMM epilogues once per load), fp32, channels-last.  Ragged batches go beyond the reference (which runs B = 1):
row b of a padded batch equals the B = 1 result on its first ``lengths[b]`` frames, whatever the padding holds."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Union

import torch
import torch.nn as nn

from .. import _C, ops

Tensor = torch.Tensor
F32, I32 = torch.float32, torch.int32
POOL_DIM, ATT_DIM, SE_DIM, SCALE = 1536, 128, 128, 8


class _Conv1dReluBn(nn.Module):
    def __init__(self, cin: int, cout: int, k: int = 1):
        super().__init__()
        self.conv = nn.Conv1d(cin, cout, k)
        self.bn = nn.BatchNorm1d(cout)


class _Res2Conv1dReluBn(nn.Module):
    def __init__(self, channels: int, dilation: int):
        super().__init__()
        w = channels // SCALE
        self.convs = nn.ModuleList([nn.Conv1d(w, w, 3, dilation=dilation, padding=dilation) for _ in range(SCALE - 1)])
        self.bns = nn.ModuleList([nn.BatchNorm1d(w) for _ in range(SCALE - 1)])


class _SEConnect(nn.Module):
    def __init__(self, channels: int):
        super().__init__()
        self.linear1 = nn.Linear(channels, SE_DIM)
        self.linear2 = nn.Linear(SE_DIM, channels)


class _SERes2Block(nn.Module):
    def __init__(self, cin: int, cout: int, dilation: int):
        super().__init__()
        self.Conv1dReluBn1 = _Conv1dReluBn(cin, cout)
        self.Res2Conv1dReluBn = _Res2Conv1dReluBn(cout, dilation)
        self.Conv1dReluBn2 = _Conv1dReluBn(cout, cout)
        self.SE_Connect = _SEConnect(cout)
        self.shortcut = nn.Conv1d(cin, cout, 1) if cin != cout else None
        self.dilation = dilation


class _AttentiveStatsPool(nn.Module):
    def __init__(self, dim: int, global_context_att: bool):
        super().__init__()
        self.linear1 = nn.Conv1d(dim * 3 if global_context_att else dim, ATT_DIM, 1)
        self.linear2 = nn.Conv1d(ATT_DIM, dim, 1)


def _fold_bn(bn: nn.BatchNorm1d, dev):
    """BatchNorm(eval) as y = x * scale + shift, computed in float64: (scale [C], shift [1, C]) f32 on ``dev``."""
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    sh = bn.bias.detach().double() - bn.running_mean.detach().double() * s
    return s.to(dev, F32).contiguous(), sh.to(dev, F32).reshape(1, -1).contiguous()


def _f(t: Tensor, dev) -> Tensor:
    return t.detach().to(dev, F32).contiguous()


class ECAPA_TDNN(nn.Module):
    def __init__(self, feat_dim: int, channels: int = 512, emb_dim: int = 192, global_context_att: bool = False,
                 feat_num: int = 25):
        super().__init__()
        if channels % SCALE or feat_dim % 4:
            raise _C.F5EError(f"ECAPA_TDNN: channels must be a multiple of {SCALE} and feat_dim of 4 (got {channels}, {feat_dim})")
        self.feat_dim, self.channels, self.emb_dim, self.feat_num = feat_dim, channels, emb_dim, feat_num
        self.global_context_att = bool(global_context_att)
        self.feature_weight = nn.Parameter(torch.zeros(feat_num))
        self.layer1 = _Conv1dReluBn(feat_dim, channels, 5)
        self.layer2 = _SERes2Block(channels, channels, 2)
        self.layer3 = _SERes2Block(channels, channels, 3)
        self.layer4 = _SERes2Block(channels, channels, 4)
        self.conv = nn.Conv1d(channels * 3, POOL_DIM, 1)
        self.pooling = _AttentiveStatsPool(POOL_DIM, self.global_context_att)
        self.bn = nn.BatchNorm1d(POOL_DIM * 2)
        self.linear = nn.Linear(POOL_DIM * 2, emb_dim)
        self._folded = None
        super().train(False)
        for p in self.parameters():
            p.requires_grad_(False)

    # ---- eval mode only --------------------------------------------------------------------------------------------
    def train(self, mode: bool = True):
        if mode:
            raise _C.F5EError("ECAPA_TDNN: training is out of scope (eval mode only: BatchNorm runs on its running statistics)")
        return super().train(False)

    def _apply(self, fn, *a, **kw):
        self._folded = None
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, *a, **kw):
        self._folded = None
        return super().load_state_dict(*a, **kw)

    # ---- weights as the kernels take them, once per load -------------------------------------------------------------
    def _fold(self) -> dict:
        dev = self.feature_weight.device
        if self._folded is not None and self._folded["device"] == dev:
            return self._folded
        if dev.type != "cuda":
            raise _C.F5EError(f"ECAPA_TDNN lives on {dev}: move it to the GPU (there is no CPU path)")

        def crb(m: _Conv1dReluBn):
            w = m.conv.weight.detach()
            s, sh = _fold_bn(m.bn, dev)                    # k taps: [C][k * Cin], tap-major as f5e_im2col lays the patches
            return dict(w=_f(w.permute(0, 2, 1).reshape(w.shape[0], -1), dev), b=_f(m.conv.bias, dev), s=s, sh=sh)

        fd = dict(device=dev, fw=_f(self.feature_weight, dev), layer1=crb(self.layer1), blocks=[])
        for blk in (self.layer2, self.layer3, self.layer4):
            r = blk.Res2Conv1dReluBn
            bns = [_fold_bn(bn, dev) for bn in r.bns]
            fd["blocks"].append(dict(
                c1=crb(blk.Conv1dReluBn1), c2=crb(blk.Conv1dReluBn2), dilation=blk.dilation,
                rw=torch.stack([_f(c.weight.permute(0, 2, 1).reshape(c.weight.shape[0], -1), dev) for c in r.convs]).contiguous(),
                rb=torch.stack([_f(c.bias, dev) for c in r.convs]).contiguous(),
                rs=torch.stack([s for s, _ in bns]).contiguous(), rsh=torch.stack([sh[0] for _, sh in bns]).contiguous(),
                se_w1=_f(blk.SE_Connect.linear1.weight, dev), se_b1=_f(blk.SE_Connect.linear1.bias, dev),
                se_w2=_f(blk.SE_Connect.linear2.weight, dev), se_b2=_f(blk.SE_Connect.linear2.bias, dev),
                sc_w=_f(blk.shortcut.weight[:, :, 0], dev) if blk.shortcut is not None else None,
                sc_b=_f(blk.shortcut.bias, dev) if blk.shortcut is not None else None))
        fd["conv_w"], fd["conv_b"] = _f(self.conv.weight[:, :, 0], dev), _f(self.conv.bias, dev)
        fd["att_w1"] = _f(self.pooling.linear1.weight[:, :, 0], dev)
        fd["att_b1"] = _f(self.pooling.linear1.bias, dev).reshape(1, -1)
        fd["att_w2"], fd["att_b2"] = _f(self.pooling.linear2.weight[:, :, 0], dev), _f(self.pooling.linear2.bias, dev)
        # tail: linear(bn(p)) = (W * scale) p + (W shift + b), folded in float64
        s = self.bn.weight.detach().double() / torch.sqrt(self.bn.running_var.detach().double() + self.bn.eps)
        sh = self.bn.bias.detach().double() - self.bn.running_mean.detach().double() * s
        w = self.linear.weight.detach().double()
        fd["tail_w"] = (w * s[None, :]).to(dev, F32).contiguous()
        fd["tail_b"] = (w @ sh + self.linear.bias.detach().double()).to(dev, F32).contiguous()
        self._folded = fd
        return fd

    # ---- workspace ---------------------------------------------------------------------------------------------------
    def _plan(self, B: int, T: int) -> Dict[str, tuple]:
        """name -> (offset in floats, shape) of every intermediate; offsets are multiples of 64 floats."""
        M, C, Fd = B * T, self.channels, self.feat_dim
        shapes = dict(x0=(B, T, Fd), mask=(M,), col=(B, T, 5 * Fd), out1=(M, C), cat=(M, 3 * C), ta=(M, C), tb=(M, C),
                      se_mean=(B, C), se_z1=(B, SE_DIM), se_z2=(B, C), h=(M, POOL_DIM), pre=(M, ATT_DIM),
                      logits=(M, POOL_DIM), ctx=(B, 2 * POOL_DIM), cadd=(B, ATT_DIM), pooled=(B, 2 * POOL_DIM))
        plan, off = {}, 0
        for name, shape in shapes.items():
            n = 1
            for d in shape:
                n *= d
            plan[name] = (off, shape)
            off += (n + 63) // 64 * 64
        plan["_total"] = (off, ())
        return plan

    def workspace_bytes(self, B: int, T: int) -> int:
        """Scratch bytes of ``forward`` for B rows of up to T frames (host arithmetic)."""
        return self._plan(int(B), int(T))["_total"][0] * 4

    # ---- forward -----------------------------------------------------------------------------------------------------
    def _check_lengths(self, lengths, B: int, T: int, dev) -> Optional[Tensor]:
        floor = 2 if self.global_context_att else 1
        if T < floor:
            raise _C.F5EError(f"ECAPA_TDNN: global_context_att needs at least 2 frames per row (unbiased variance); got T = {T}")
        if lengths is None:
            return None
        if isinstance(lengths, Tensor) and lengths.is_cuda:
            if lengths.dtype != I32 or lengths.shape != (B,):
                raise _C.F5EError(f"ECAPA_TDNN: lengths must be i32 [{B}] (got {lengths.dtype} {tuple(lengths.shape)})")
            return lengths          # device lengths are not read back: rows shorter than the floor are the caller's to avoid
        host = [int(v) for v in (lengths.tolist() if isinstance(lengths, Tensor) else lengths)]
        if len(host) != B or min(host) < floor or max(host) > T:
            raise _C.F5EError(f"ECAPA_TDNN: lengths must be {B} values in [{floor}, {T}]"
                              + (" (global_context_att takes an unbiased variance over time)" if floor == 2 else "")
                              + f"; got {host}")
        return torch.tensor(host, dtype=I32).to(dev, non_blocking=True)

    @torch.no_grad()
    def forward(self, hidden_states: Union[Tensor, Sequence[Tensor]], lengths=None, *, workspace: Optional[Tensor] = None,
                out: Optional[Tensor] = None, intermediates: Optional[dict] = None) -> Tensor:
        """hidden_states f32 [L, B, T, feat_dim] on the GPU (or a list of L tensors [B, T, feat_dim]); lengths i32 [B] on the
        device (None: every row has T frames; a host sequence / CPU tensor is validated and uploaded) -> f32 [B, emb_dim].
        No device-to-host copy, no synchronisation; with ``workspace`` (``workspace_bytes(B, T)`` bytes, f32 or uint8) and
        ``out`` it allocates nothing, so it can be captured into a graph.  ``intermediates``: a dict that receives views of
        the workspace (feat, out1..out4 [B, T, C], pooled) -- valid until the next call on that workspace."""
        hs = hidden_states
        if not isinstance(hs, Tensor):
            hs = list(hs)
            if len(hs) != self.feat_num:
                raise _C.F5EError(f"ECAPA_TDNN: {len(hs)} hidden states given, feat_num is {self.feat_num}")
            hs = torch.stack(hs, 0)
        if hs.ndim != 4 or hs.shape[0] != self.feat_num or hs.shape[3] != self.feat_dim:
            raise _C.F5EError(f"ECAPA_TDNN: hidden_states must be [L = {self.feat_num}, B, T, feat_dim = {self.feat_dim}] "
                              f"(got {tuple(hs.shape)})")
        if hs.dtype != F32:
            raise _C.F5EError(f"ECAPA_TDNN: hidden_states must be float32 (got {hs.dtype})")
        L, B, T, Fd = hs.shape
        if B < 1 or T < 1:
            raise _C.F5EError(f"ECAPA_TDNN: empty batch {tuple(hs.shape)}")
        if not hs.is_cuda:
            self._check_lengths(lengths, B, T, hs.device)
            raise _C.F5EError(f"ECAPA_TDNN: hidden_states live on {hs.device}; there is no CPU path")
        dev = hs.device
        lengths = self._check_lengths(lengths, B, T, dev)
        fd = self._fold()
        hs = hs.contiguous()
        plan = self._plan(B, T)
        need = plan["_total"][0]
        if workspace is None:
            ws = torch.empty(need, dtype=F32, device=dev)
        else:
            if not workspace.is_cuda or workspace.dtype not in (F32, torch.uint8) or not workspace.is_contiguous() or \
                    workspace.data_ptr() % 16 or workspace.numel() * workspace.element_size() < need * 4:
                raise _C.F5EError(f"ECAPA_TDNN: workspace must be a contiguous 16-byte aligned f32 / uint8 GPU tensor of at "
                                  f"least {need * 4} bytes (workspace_bytes)")
            ws = workspace.view(-1)
            ws = ws[: ws.numel() // 4 * 4].view(F32) if ws.dtype == torch.uint8 else ws
        if out is None:
            out = torch.empty(B, self.emb_dim, dtype=F32, device=dev)
        elif out.shape != (B, self.emb_dim) or out.dtype != F32 or not out.is_cuda or not out.is_contiguous():
            raise _C.F5EError(f"ECAPA_TDNN: out must be a contiguous f32 GPU tensor [{B}, {self.emb_dim}]")

        def buf(name):
            off, shape = plan[name]
            n = 1
            for d in shape:
                n *= d
            return ws[off:off + n].view(shape)

        M, C, RELU = B * T, self.channels, ops.ACT_RELU
        x0, mask, col = buf("x0"), buf("mask"), buf("col")
        ops.layer_mix_inorm(hs, fd["fw"], lengths, x0, mask.view(B, T))
        ops.im2col(x0, col, 5, 2)

        def crb(a, p, o):     # conv -> ReLU -> BN, zero beyond each row's length
            return ops.gemm_f32(a, p["w"], p["b"], out=o, act=RELU, ch_scale=p["s"], addend=p["sh"], row_scale=mask)

        out1, cat, ta, tb = buf("out1"), buf("cat"), buf("ta"), buf("tb")
        se_mean, se_z1, se_z2 = buf("se_mean"), buf("se_z1"), buf("se_z2")
        crb(col.view(M, 5 * Fd), fd["layer1"], out1)
        prev = out1
        for k, blk in enumerate(fd["blocks"]):
            crb(prev, blk["c1"], ta)
            ops.res2_dconv(ta.view(B, T, C), tb.view(B, T, C), blk["rw"], blk["rb"], blk["rs"], blk["rsh"], lengths,
                           blk["dilation"])
            crb(tb, blk["c2"], ta)
            ops.time_stats(ta.view(B, T, C), lengths, se_mean)
            ops.gemm_f32(se_mean, blk["se_w1"], blk["se_b1"], out=se_z1, act=RELU)
            ops.gemm_f32(se_z1, blk["se_w2"], blk["se_b2"], out=se_z2)
            resid = prev
            if blk["sc_w"] is not None:
                resid = ops.gemm_f32(prev, blk["sc_w"], blk["sc_b"], out=tb, row_scale=mask)
            nxt = cat[:, k * C:(k + 1) * C]
            ops.se_scale(ta.view(B, T, C), se_z2, resid.unflatten(0, (B, T)), nxt.unflatten(0, (B, T)))
            prev = nxt
        h, pre, logits, pooled = buf("h"), buf("pre"), buf("logits"), buf("pooled")
        ops.gemm_f32(cat, fd["conv_w"], fd["conv_b"], out=h, act=RELU, row_scale=mask)
        add = fd["att_b1"]
        if self.global_context_att:      # the two context terms are constant over time: they enter as a per-row addend
            ctx, add = buf("ctx"), buf("cadd")
            ops.time_stats(h.view(B, T, POOL_DIM), lengths, ctx[:, :POOL_DIM], ctx[:, POOL_DIM:])
            ops.gemm_f32(ctx, fd["att_w1"][:, POOL_DIM:], fd["att_b1"][0], out=add)
        ops.gemm_f32(h, fd["att_w1"][:, :POOL_DIM], None, out=pre)
        ops.bias_tanh(pre.view(B, T, ATT_DIM), add)
        ops.gemm_f32(pre, fd["att_w2"], fd["att_b2"], out=logits)
        ops.attn_stats_pool(h.view(B, T, POOL_DIM), logits.view(B, T, POOL_DIM), lengths, pooled)
        ops.gemm_f32(pooled, fd["tail_w"], fd["tail_b"], out=out)
        if intermediates is not None:
            c3 = cat.view(B, T, 3 * C)
            intermediates.update(feat=x0, out1=out1.view(B, T, C), out2=c3[:, :, :C], out3=c3[:, :, C:2 * C],
                                 out4=c3[:, :, 2 * C:], pooled=pooled)
        return out

    # ---- convenience -------------------------------------------------------------------------------------------------
    def embed_wavs(self, wavs: List[Tensor], feature_extract: Optional[Callable] = None, lengths=None) -> Tensor:
        """The reference's ``model(wavs)``: ``feature_extract(wavs)`` must return the s3prl-style dict
        ``{"hidden_states": [L tensors [B, T, feat_dim]]}`` (16 kHz audio in, as the reference resamples before the call).
        ``lengths``: frames per row when the upstream padded its batch."""
        if feature_extract is None:
            raise _C.F5EError("ECAPA_TDNN.embed_wavs: the WavLM upstream is not built in this project; pass a "
                              "feature_extract callable that returns {'hidden_states': [...]}, or call forward() on "
                              "precomputed hidden states")
        feats = feature_extract(list(wavs))["hidden_states"]
        return self.forward(list(feats) if isinstance(feats, (list, tuple)) else [feats], lengths)

    def similarity(self, hs_a, len_a, hs_b, len_b) -> Tensor:
        """Cosine of the embeddings of two batches of recordings -> f32 [B] on the device (``run_sim``'s score)."""
        ea = self.forward(hs_a, len_a)
        eb = self.forward(hs_b, len_b)
        return torch.nn.functional.cosine_similarity(ea, eb, dim=1)


def ECAPA_TDNN_SMALL(feat_dim: int, emb_dim: int = 256, feat_num: int = 25) -> ECAPA_TDNN:
    return ECAPA_TDNN(feat_dim=feat_dim, channels=512, emb_dim=emb_dim, feat_num=feat_num)
