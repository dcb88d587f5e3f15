"""WavLM-large, the upstream of the SIM metric (the reference fetches it through ``torch.hub`` / s3prl, eval/ecapa_tdnn.py:171-199):
from 16 kHz audio to the stack of hidden states that ``ECAPA_TDNN.forward`` takes -- the input of every encoder layer plus the
encoder output, s3prl's ``hidden_states`` list.  fp32, eval mode, on the device: csrc/wavlm.hip, f5e_relbias_attn_f32,
f5e_gemm_f32 and f5e_layernorm; the encoder layer is ``xfmr_f32.layer``, pre-norm, each layer writing the
next entry of the stack.  The sub-modules only HOLD the weights.  ``WaveEncoder``: what is shared with ``eval/wav2vec2.py``.

Only the large family's structure is built (layer-norm feature extractor, ``layer_norm_first``, ``normalize=True``); anything
else is refused by field name.  Parameter names are fairseq's / s3prl's, so ``load_state_dict`` works on the
``feature_extract.model.`` slice of a reference SIM checkpoint (``WavLM.from_sim_checkpoint``):

    feature_extractor.conv_layers.{i}.0.weight, feature_extractor.conv_layers.{i}.2.1.{weight,bias}, layer_norm.*,
    post_extract_proj.*, mask_emb (held, unused), encoder.pos_conv.0.{weight_g,weight_v,bias},
    encoder.layers.{i}.self_attn.{q,k,v,out}_proj.*, .self_attn.grep_linear.*, .self_attn.grep_a,
    encoder.layers.0.self_attn.relative_attention_bias.weight, encoder.layers.{i}.self_attn_layer_norm.*, .fc1.*, .fc2.*,
    .final_layer_norm.*, encoder.layer_norm.*

This list is RESTATED from the published WavLM module; no upstream source or checkpoint was at hand to verify it against
(two of the names are pinned by tests/test_ecapa_cpu.py).  ``convert_hf_state_dict`` maps a ``transformers`` ``WavLMModel``
state dict onto it.

Ragged batches: row b of a padded batch equals the B = 1 run on its own ``lengths[b]`` samples for every frame below
``frames[b]``; frames at or beyond it hold finite values that mean nothing."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from .. import _C, ops
from ..xfmr_f32 import fold, fold_layer, layer, plan, take, view

Tensor = torch.Tensor
F32, I32 = torch.float32, torch.int32
SIM_PREFIX = "feature_extract.model."


@dataclass
class WavLMConfig:
    """Defaults = WavLM-large."""
    conv_dim: Tuple[int, ...] = (512,) * 7
    conv_kernel: Tuple[int, ...] = (10, 3, 3, 3, 3, 2, 2)
    conv_stride: Tuple[int, ...] = (5, 2, 2, 2, 2, 2, 2)
    conv_bias: bool = False
    extractor_mode: str = "layer_norm"
    layer_norm_first: bool = True
    normalize: bool = True
    encoder_embed_dim: int = 1024
    encoder_layers: int = 24
    encoder_attention_heads: int = 16
    encoder_ffn_embed_dim: int = 4096
    conv_pos: int = 128
    conv_pos_groups: int = 16
    num_buckets: int = 320
    max_distance: int = 800
    layer_norm_eps: float = 1e-5

    def check(self) -> None:
        def refuse(field, why):
            raise _C.F5EError(f"WavLM: {field} = {getattr(self, field)!r} is not built: {why}")
        if self.extractor_mode != "layer_norm":
            refuse("extractor_mode", "only the layer-norm feature extractor of the large family is (group-norm extractors are not)")
        if not self.layer_norm_first:
            refuse("layer_norm_first", "only the pre-LayerNorm encoder of the large family is (post-LN encoders are not)")
        if not self.normalize:
            refuse("normalize", "the large family normalises the waveform")
        n = len(self.conv_dim)
        if not (1 <= n <= 8 and len(self.conv_kernel) == n and len(self.conv_stride) == n):
            refuse("conv_kernel", f"conv_dim, conv_kernel and conv_stride need one length in 1..8 (got {n}, "
                                  f"{len(self.conv_kernel)}, {len(self.conv_stride)})")
        if len(set(self.conv_dim)) != 1 or self.conv_dim[0] % 4 or self.conv_dim[0] > 512:
            refuse("conv_dim", "one width for all layers, a multiple of 4, at most 512")
        if self.conv_kernel[0] != 10 or self.conv_stride[0] != 5:
            refuse("conv_kernel", "layer 0 is built for kernel 10, stride 5")
        if any(k < s or s < 1 for k, s in zip(self.conv_kernel, self.conv_stride)):
            refuse("conv_stride", "every layer needs 1 <= stride <= kernel")
        D, H = self.encoder_embed_dim, self.encoder_attention_heads
        if D % H or D // H not in (16, 32, 64):
            refuse("encoder_attention_heads", f"head dim {D / H:g} (16, 32 and 64 are)")
        if D % self.conv_pos_groups or (D // self.conv_pos_groups) % 4:
            refuse("conv_pos_groups", "encoder_embed_dim / conv_pos_groups must be a multiple of 4")
        if self.encoder_ffn_embed_dim % 4 or self.num_buckets % 4 or self.num_buckets < 4:
            refuse("encoder_ffn_embed_dim", "multiples of 4 (also num_buckets)")


def frame_counts(n_samples: int, cfg: WavLMConfig) -> List[int]:
    """Frames after every conv layer: n <- (n - k) // s + 1, 0 once n < k (what f5e_wav_norm computes on the device)."""
    out, n = [], int(n_samples)
    for k, s in zip(cfg.conv_kernel, cfg.conv_stride):
        n = (n - k) // s + 1 if n >= k else 0
        out.append(n)
    return out


def relative_bucket(rel: Tensor, num_buckets: int = 320, max_distance: int = 800) -> Tensor:
    """Bucket of relative position j - i (int64 tensor), with the float32 torch expression of the published module: exact below
    |rel| = num_buckets / 4, log-spaced above, sign in the upper half."""
    nb = num_buckets // 2
    ret = (rel > 0).to(torch.long) * nb
    n = torch.abs(rel)
    max_exact = nb // 2
    is_small = n < max_exact
    large = torch.log(n.float() / max_exact)
    large = large / math.log(max_distance / max_exact)
    large = large * (nb - max_exact)
    large = (max_exact + large).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return ret + torch.where(is_small, n, large)


def bias_table(rel_embed: Tensor, Tt: int, num_buckets: int = 320, max_distance: int = 800) -> Tensor:
    """rel_embed [num_buckets][H] -> table [H][2 Tt - 1] with table[h][j - i + Tt - 1] = rel_embed[bucket(j - i)][h]."""
    rel = torch.arange(-(Tt - 1), Tt, dtype=torch.long)
    return rel_embed.detach().cpu()[relative_bucket(rel, num_buckets, max_distance)].t().contiguous()


def fold_weight_norm(weight_g: Tensor, weight_v: Tensor) -> Tensor:
    """weight_norm(dim=2): w[:, :, k] = g[k] v[:, :, k] / ||v[:, :, k]||, in float64."""
    v = weight_v.detach().double()
    return v * (weight_g.detach().double() / v.norm(dim=(0, 1), keepdim=True))


_HF_LAYER = {"attention.q_proj": "self_attn.q_proj", "attention.k_proj": "self_attn.k_proj", "attention.v_proj": "self_attn.v_proj",
             "attention.out_proj": "self_attn.out_proj", "attention.gru_rel_pos_linear": "self_attn.grep_linear",
             "attention.rel_attn_embed": "self_attn.relative_attention_bias", "layer_norm": "self_attn_layer_norm",
             "feed_forward.intermediate_dense": "fc1", "feed_forward.output_dense": "fc2", "final_layer_norm": "final_layer_norm"}


def convert_hf_state_dict(sd: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """``transformers`` ``WavLMModel`` names -> the fairseq / s3prl names of this module (a leading ``wavlm.`` is dropped).  Keys
    that belong to nothing built here (adapters, quantizers) raise."""
    out = {}
    for key, val in sd.items():
        k = key[len("wavlm."):] if key.startswith("wavlm.") else key
        p = k.split(".")
        if k == "masked_spec_embed":
            new = "mask_emb"
        elif p[0] == "feature_extractor" and p[1] == "conv_layers" and p[3] == "conv":
            new = f"feature_extractor.conv_layers.{p[2]}.0.{p[4]}"
        elif p[0] == "feature_extractor" and p[1] == "conv_layers" and p[3] == "layer_norm":
            new = f"feature_extractor.conv_layers.{p[2]}.2.1.{p[4]}"
        elif k.startswith("feature_projection.layer_norm."):
            new = "layer_norm." + p[-1]
        elif k.startswith("feature_projection.projection."):
            new = "post_extract_proj." + p[-1]
        elif k.startswith("encoder.pos_conv_embed.conv."):
            tail = ".".join(p[3:])
            new = "encoder.pos_conv.0." + {"parametrizations.weight.original0": "weight_g", "parametrizations.weight.original1": "weight_v",
                                           "weight_g": "weight_g", "weight_v": "weight_v", "bias": "bias"}[tail]
        elif k.startswith("encoder.layer_norm."):
            new = k
        elif p[0] == "encoder" and p[1] == "layers":
            tail = ".".join(p[3:])
            if tail == "attention.gru_rel_pos_const":
                new = f"encoder.layers.{p[2]}.self_attn.grep_a"
            else:
                mod, leaf = tail.rsplit(".", 1)
                if mod not in _HF_LAYER:
                    raise KeyError(f"convert_hf_state_dict: {key} has no counterpart")
                new = f"encoder.layers.{p[2]}.{_HF_LAYER[mod]}.{leaf}"
        else:
            raise KeyError(f"convert_hf_state_dict: {key} has no counterpart")
        out[new] = val
    return out


class _Holder(nn.Module):
    """A child without parameters that only keeps the numbering of the published ``nn.Sequential`` layouts."""


class _WeightNormConv(nn.Module):
    def __init__(self, D: int, k: int, groups: int):
        super().__init__()
        conv = nn.Conv1d(D, D, k, padding=k // 2, groups=groups)
        self.weight_v = nn.Parameter(conv.weight.detach().clone())
        self.weight_g = nn.Parameter(conv.weight.detach().norm(dim=(0, 1), keepdim=True))
        self.bias = nn.Parameter(conv.bias.detach().clone())


class _SelfAttn(nn.Module):
    def __init__(self, D: int, H: int, num_buckets: int, has_bias: bool):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj, self.out_proj = (nn.Linear(D, D) for _ in range(4))
        self.grep_linear = nn.Linear(D // H, 8)
        self.grep_a = nn.Parameter(torch.ones(1, H, 1, 1))
        if has_bias:
            self.relative_attention_bias = nn.Embedding(num_buckets, H)


class _Layer(nn.Module):
    def __init__(self, cfg: WavLMConfig, first: bool):
        super().__init__()
        D = cfg.encoder_embed_dim
        self.self_attn = _SelfAttn(D, cfg.encoder_attention_heads, cfg.num_buckets, first)
        self.self_attn_layer_norm = nn.LayerNorm(D, eps=cfg.layer_norm_eps)
        self.fc1, self.fc2 = nn.Linear(D, cfg.encoder_ffn_embed_dim), nn.Linear(cfg.encoder_ffn_embed_dim, D)
        self.final_layer_norm = nn.LayerNorm(D, eps=cfg.layer_norm_eps)


class _Encoder(nn.Module):
    def __init__(self, cfg: WavLMConfig):
        super().__init__()
        D = cfg.encoder_embed_dim
        self.pos_conv = nn.Sequential(_WeightNormConv(D, cfg.conv_pos, cfg.conv_pos_groups))
        self.layers = nn.ModuleList([_Layer(cfg, i == 0) for i in range(cfg.encoder_layers)])
        self.layer_norm = nn.LayerNorm(D, eps=cfg.layer_norm_eps)


class _FeatureExtractor(nn.Module):
    def __init__(self, cfg: WavLMConfig):
        super().__init__()
        layers, cin = [], 1
        for c, k, s in zip(cfg.conv_dim, cfg.conv_kernel, cfg.conv_stride):   # conv, dropout, (transpose, LayerNorm, transpose), GELU
            layers.append(nn.Sequential(nn.Conv1d(cin, c, k, stride=s, bias=cfg.conv_bias), _Holder(),
                                        nn.Sequential(_Holder(), nn.LayerNorm(c, eps=cfg.layer_norm_eps), _Holder()), _Holder()))
            cin = c
        self.conv_layers = nn.ModuleList(layers)


def _f(t: Tensor, dev) -> Tensor:
    return t.detach().to(dev, F32).contiguous()


class WaveEncoder(nn.Module):
    """What WavLM and Wav2Vec2 share: eval mode only, the weights folded once per load, the conv front-end's geometry, the
    scratch plan, the checks of ``extract`` and its launches up to the masked projection.  A model adds its parameter holders
    (``feature_extractor``, ``layer_norm``, ``post_extract_proj``, ``encoder``), ``_shapes``, ``_fold_more`` and ``extract``."""
    _conv_act = ops.ACT_NONE                    # the activation fused into the GEMMs of conv layers 1..

    def _freeze(self) -> None:
        self._folded, self._tables = None, {}
        nn.Module.train(self, False)
        for p in self.parameters():
            p.requires_grad_(False)

    # ---- eval mode only; weights as the kernels take them, once per load ------------------------------------------------
    def train(self, mode: bool = True):
        if mode:
            raise _C.F5EError(f"{type(self).__name__}: training is out of scope (eval mode only)")
        return super().train(False)

    def _apply(self, fn, *a, **kw):
        self._folded, self._tables = None, {}
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, *a, **kw):
        self._folded, self._tables = None, {}
        return super().load_state_dict(*a, **kw)

    def _fold(self) -> dict:
        dev = self.layer_norm.weight.device
        if self._folded is not None and self._folded["device"] == dev:
            return self._folded
        if dev.type != "cuda":
            raise _C.F5EError(f"{type(self).__name__} lives on {dev}: move it to the GPU (there is no CPU path)")
        cfg, enc = self.cfg, self.encoder
        fd = dict(device=dev, conv=[], layers=[])
        for i, seq in enumerate(self.feature_extractor.conv_layers):
            w = seq[0].weight.detach()
            w = w[:, 0] if i == 0 else w.permute(0, 2, 1).reshape(w.shape[0], -1)     # tap-major: k = tap * C + ic
            fd["conv"].append(dict(w=_f(w, dev), b=_f(seq[0].bias, dev) if seq[0].bias is not None else None))
        fd["ln_g"], fd["ln_b"] = fold(dev, self.layer_norm)
        fd["proj_w"], fd["proj_b"] = fold(dev, self.post_extract_proj)
        pc = enc.pos_conv[0]
        fd["pos_w"] = ops.pack_wavlm_posconv_weight(fold_weight_norm(pc.weight_g, pc.weight_v), cfg.conv_pos_groups).to(dev)
        fd["pos_b"] = _f(pc.bias, dev)
        for lyr in enc.layers:
            sa = lyr.self_attn
            fd["layers"].append(fold_layer(dev, lyr.self_attn_layer_norm, sa.q_proj, sa.k_proj, sa.v_proj, sa.out_proj,
                                           lyr.final_layer_norm, lyr.fc1, lyr.fc2))
        fd["enc_g"], fd["enc_b"] = fold(dev, enc.layer_norm)
        self._fold_more(fd, dev)
        self._folded = fd
        return fd

    # ---- geometry and workspace ---------------------------------------------------------------------------------------------
    def frame_count(self, n_samples: int) -> int:
        return frame_counts(n_samples, self.cfg)[-1]

    def min_samples(self) -> int:
        """The shortest row that yields one frame."""
        n = 1
        for k, s in zip(reversed(self.cfg.conv_kernel), reversed(self.cfg.conv_stride)):
            n = (n - 1) * s + k
        return n

    def _geometry(self, S: int) -> Tuple[int, List[int], List[int]]:
        """(T, need, pitch): frames of the longest row, the frames of layer l that layer l + 1 .. reads (need[l]) and the frame
        pitch of a batch row in layer l.  pitch[l - 1] = stride[l] * pitch[l], so row m = b * pitch[l] + t of layer l starts
        at frame stride[l] * m of layer l - 1 for EVERY batch row: each strided conv is one GEMM on an overlapping view."""
        cfg = self.cfg
        T = frame_counts(S, cfg)[-1]
        n = len(cfg.conv_dim)
        need, pitch = [0] * n, [0] * n
        need[-1], pitch[-1] = T, T + 1
        for l in range(n - 1, 0, -1):
            need[l - 1] = (need[l] - 1) * cfg.conv_stride[l] + cfg.conv_kernel[l]
            pitch[l - 1] = cfg.conv_stride[l] * pitch[l]
        while any(nd > p for nd, p in zip(need, pitch)):        # never with the large family's kernels (need <= pitch above)
            pitch = [p + math.prod(cfg.conv_stride[l + 1:]) for l, p in enumerate(pitch)]
        return T, need, pitch

    def _plan(self, B: int, S: int) -> Dict[str, tuple]:
        """name -> (offset in floats, shape) of every intermediate; offsets are multiples of 64 floats."""
        cfg = self.cfg
        T, _need, pitch = self._geometry(S)
        C, slack = cfg.conv_dim[-1], max(cfg.conv_kernel) * cfg.conv_dim[-1]
        return plan(self._shapes(B, S, max(T, 1), ca=(B * pitch[0] * C + slack,),
                                 cb=(B * (pitch[1] if len(pitch) > 1 else 1) * C + slack,)))

    def workspace_bytes(self, B: int, S: int) -> int:
        """Scratch bytes of ``extract`` for B rows of S samples (host arithmetic)."""
        return self._plan(int(B), int(S))["_total"][0] * 4

    # ---- forward: the part of ``extract`` that both models run -----------------------------------------------------------
    def _enter(self, wav: Tensor, lengths, workspace: Optional[Tensor]):
        """The checks of ``extract`` -> (wav, lengths on the device, the folded weights, buf(name): a view of the scratch)."""
        who = f"{type(self).__name__}.extract"
        if not isinstance(wav, Tensor) or wav.ndim != 2 or wav.dtype != F32:
            raise _C.F5EError(f"{who}: wav must be a float32 tensor [B, S]")
        if not wav.is_cuda:
            raise _C.F5EError(f"{who}: wav lives on {wav.device}; there is no CPU path")
        B, S = wav.shape
        if B < 1 or self._geometry(S)[0] < 1:
            raise _C.F5EError(f"{who}: {S} samples give no frame (a row needs {self.min_samples()})")
        if lengths is not None and not (isinstance(lengths, Tensor) and lengths.is_cuda):
            host = [int(v) for v in (lengths.tolist() if isinstance(lengths, Tensor) else lengths)]
            if len(host) != B or min(host) < self.min_samples() or max(host) > S:
                raise _C.F5EError(f"{who}: lengths must be {B} values in [{self.min_samples()}, {S}]; got {host}")
            lengths = torch.tensor(host, dtype=I32).to(wav.device, non_blocking=True)
        elif lengths is not None and (lengths.dtype != I32 or lengths.shape != (B,)):
            raise _C.F5EError(f"{who}: lengths must be i32 [{B}] (got {lengths.dtype} {tuple(lengths.shape)})")
        fd, pl = self._fold(), self._plan(B, S)
        ws = take(workspace, pl["_total"][0], wav.device, who)
        return wav.contiguous(), lengths, fd, lambda name: view(ws, pl, name)

    def _after_conv(self, y: Tensor, p: dict, eps: float) -> None:
        """What follows the GEMM of a conv layer 1.. (nothing when ``_conv_act`` is all)."""

    def _project(self, fd: dict, buf, cur: Tensor, nxt: Tensor, B: int, T: int, pitch: List[int]) -> Tensor:
        """Conv layers 1.. (one GEMM each on an overlapping strided view of the layer below, ``cur``, ping-pong with ``nxt``),
        the LayerNorm of every row's own T frames and the masked projection -> proj [B * T, D]."""
        cfg = self.cfg
        C, eps = cfg.conv_dim[-1], cfg.layer_norm_eps
        for l in range(1, len(cfg.conv_dim)):
            k, s, p = cfg.conv_kernel[l], cfg.conv_stride[l], fd["conv"][l]
            rows = B * pitch[l]
            y = nxt[:rows * C].view(rows, C)
            ops.gemm_f32(torch.as_strided(cur, (rows, k * C), (s * C, 1)), p["w"], p["b"], out=y, act=self._conv_act)
            self._after_conv(y, p, eps)
            cur, nxt = nxt, cur
        feat, xnc = cur[:B * pitch[-1] * C].view(B, pitch[-1], C), buf("xnc")
        for b in range(B):
            ops.layernorm(feat[b, :T], xnc[b * T:(b + 1) * T], fd["ln_g"], fd["ln_b"], eps=eps)
        return ops.gemm_f32(xnc, fd["proj_w"], fd["proj_b"], out=buf("proj"), row_scale=buf("mask"))     # x[padding_mask] = 0


class WavLM(WaveEncoder):
    def __init__(self, cfg: Optional[WavLMConfig] = None):
        super().__init__()
        self.cfg = cfg = cfg or WavLMConfig()
        cfg.check()
        C, D = cfg.conv_dim[-1], cfg.encoder_embed_dim
        self.feature_extractor = _FeatureExtractor(cfg)
        self.layer_norm = nn.LayerNorm(C, eps=cfg.layer_norm_eps)
        self.post_extract_proj = nn.Linear(C, D)
        self.mask_emb = nn.Parameter(torch.zeros(D))
        self.encoder = _Encoder(cfg)
        self._freeze()

    @classmethod
    def from_sim_checkpoint(cls, state: Dict[str, Tensor], cfg: Optional[WavLMConfig] = None) -> "WavLM":
        """``state``: the ``"model"`` entry of a reference SIM checkpoint; its ``feature_extract.model.*`` slice is loaded."""
        sd = {k[len(SIM_PREFIX):]: v for k, v in state.items() if k.startswith(SIM_PREFIX)}
        if not sd:
            raise _C.F5EError(f"WavLM.from_sim_checkpoint: the state dict has no {SIM_PREFIX}* keys")
        model = cls(cfg)
        missing, unexpected = model.load_state_dict(sd, strict=False)
        if missing:
            raise _C.F5EError(f"WavLM.from_sim_checkpoint: the checkpoint lacks {len(missing)} keys, e.g. {missing[:3]}")
        return model

    def _fold_more(self, fd: dict, dev) -> None:
        for p, seq in zip(fd["conv"], self.feature_extractor.conv_layers):
            p["g"], p["beta"] = fold(dev, seq[2][1])
        gates = [(lyr.self_attn.grep_linear, lyr.self_attn.grep_a) for lyr in self.encoder.layers]
        fd["layers"] = [W._replace(extra=(*fold(dev, lin), _f(a.reshape(-1), dev)))                 # w_gate, b_gate, const
                        for W, (lin, a) in zip(fd["layers"], gates)]

    def _table(self, T: int) -> Tensor:
        """The bias table for Tt = T, built on the host once per (load, T)."""
        dev = self.mask_emb.device
        t = self._tables.get(T)
        if t is None or t.device != dev:
            cfg = self.cfg
            emb = self.encoder.layers[0].self_attn.relative_attention_bias.weight
            t = self._tables[T] = bias_table(emb, T, cfg.num_buckets, cfg.max_distance).to(dev, F32).contiguous()
        return t

    def _shapes(self, B: int, S: int, T: int, **conv) -> Dict[str, tuple]:
        cfg = self.cfg
        C, D, H, M = cfg.conv_dim[-1], cfg.encoder_embed_dim, cfg.encoder_attention_heads, B * T
        return dict(frames=(B,), wn=(B, S), partials=(ops.wav_norm_partials(B, S),), mask=(M,), **conv, xnc=(M, C), proj=(M, D),
                    xn=(M, D), qkv=(M, 3 * D), gate=(B, H, T), ao=(M, D), ff=(M, cfg.encoder_ffn_embed_dim))

    def _after_conv(self, y: Tensor, p: dict, eps: float) -> None:
        ops.layernorm_gelu(y, y, p["g"], p["beta"], eps)

    # ---- forward -------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def extract(self, wav: Tensor, lengths=None, *, out: Optional[Tensor] = None, workspace: Optional[Tensor] = None):
        """wav f32 [B, S] on the GPU, 16 kHz; lengths: samples per row, i32 [B] on the device (None: S; a host sequence is
        validated and uploaded, which allocates) -> (hs f32 [L + 1, B, T, D], frames i32 [B]); ``frames`` is a view of the
        workspace, valid until the next call on it.  No device-to-host copy, no synchronisation; with ``out``, ``workspace``
        (``workspace_bytes(B, S)`` bytes, f32 or uint8) and device lengths it allocates nothing once the weights are folded and
        the bias table of this T exists (a first call does both), so it can be captured into a graph."""
        cfg = self.cfg
        wav, lengths, fd, buf = self._enter(wav, lengths, workspace)
        (B, S), (T, need, pitch) = wav.shape, self._geometry(wav.shape[1])
        table = self._table(T)
        C, D, H, L = cfg.conv_dim[-1], cfg.encoder_embed_dim, cfg.encoder_attention_heads, cfg.encoder_layers
        if out is None:
            out = torch.empty(L + 1, B, T, D, dtype=F32, device=wav.device)
        elif out.shape != (L + 1, B, T, D) or out.dtype != F32 or not out.is_cuda or not out.is_contiguous():
            raise _C.F5EError(f"WavLM.extract: out must be a contiguous f32 GPU tensor [{L + 1}, {B}, {T}, {D}]")
        M, eps = B * T, cfg.layer_norm_eps
        frames, wn = buf("frames").view(I32), buf("wn")
        ops.wav_norm(wav, lengths, wn, buf("partials"), frames, buf("mask").view(B, T), cfg.conv_kernel, cfg.conv_stride)
        cur, c0 = buf("ca"), fd["conv"][0]                      # the conv front-end: layer 0 fused
        ops.wavlm_conv0(wn, c0["w"], c0["b"], c0["g"], c0["beta"], cur[:B * pitch[0] * C].view(B, pitch[0], C), T0=need[0])
        proj = self._project(fd, buf, cur, buf("cb"), B, T, pitch)
        ops.wavlm_posconv(proj.view(B, T, D), fd["pos_w"], fd["pos_b"], frames, out[0])
        bufs, gate, scale = (buf("xn"), buf("qkv"), buf("ao"), None, buf("ff")), buf("gate"), (D // H) ** -0.5

        def self_attn(W, xn, qkv, ao):                          # the gated relative-position bias: two launches
            ops.wavlm_gate(xn, *W.extra, gate)
            ops.relbias_attn(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], gate, table, H, scale, kv_len=frames, out=ao)

        for l, W in enumerate(fd["layers"]):                    # pre-LN; layer l reads out[l] and writes out[l + 1]
            layer(out[l].view(M, D), out[l + 1].view(M, D), W, bufs, pre_norm=True, act=ops.ACT_GELU_ERF, eps=eps,
                  self_attn=self_attn)
        last = out[L].view(M, D)
        ops.layernorm(last, last, fd["enc_g"], fd["enc_b"], eps=eps)
        return out, frames

    def forward(self, wavs: Sequence[Tensor]) -> dict:
        """s3prl's call: a list of 1-D 16 kHz waveforms on the GPU -> {"hidden_states": [L + 1 tensors [B, T, D]], "lengths":
        frames i32 [B]}, so an instance is a ``feature_extract`` for ``ECAPA_TDNN.embed_wavs`` (whose ``lengths`` are the
        host-side ``frame_count`` of every wav)."""
        wavs = list(wavs)
        if not wavs or any(w.ndim != 1 or not w.is_cuda for w in wavs):
            raise _C.F5EError("WavLM: forward takes a non-empty list of 1-D GPU tensors; there is no CPU path")
        n = [int(w.numel()) for w in wavs]
        batch = torch.zeros(len(wavs), max(n), dtype=F32, device=wavs[0].device)
        for b, w in enumerate(wavs):
            batch[b, :n[b]] = w.to(F32)
        hs, frames = self.extract(batch, n)
        return {"hidden_states": list(hs.unbind(0)), "lengths": frames}
