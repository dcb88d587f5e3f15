"""wav2vec2-base, the upstream of the UTMOS predictor (``eval/utmos.py``; the reference fetches ``utmos22_strong`` through
``torch.hub``, eval/eval_utmos.py:18): from 16 kHz audio to the last hidden state of the encoder.  fp32, eval mode, on the device:
f5e_w2v_conv0_gn (csrc/utmos.hip), f5e_gemm_f32, f5e_layernorm, f5e_wavlm_posconv and f5e_mha_f32; the encoder layer
is ``xfmr_f32.layer``, post-norm, and everything shared with WavLM is ``eval/wavlm.py::WaveEncoder``.  The sub-modules
only HOLD the weights.

Only the base family's structure is built -- the fairseq "default" feature extractor (GroupNorm over time after conv 0, no norm
after convs 1..), the post-LayerNorm encoder, ``normalize = False`` (the raw waveform goes in) -- and anything else is refused by
field name; the large family's structure is ``eval/wavlm.py``.  Parameter names are those of the fairseq module:

    feature_extractor.conv_layers.{i}.0.weight, feature_extractor.conv_layers.0.2.{weight,bias} (the group norm), layer_norm.*,
    post_extract_proj.*, encoder.pos_conv.0.{weight_g,weight_v,bias}, encoder.layers.{i}.self_attn.{q,k,v,out}_proj.*,
    encoder.layers.{i}.self_attn_layer_norm.*, .fc1.*, .fc2.*, .final_layer_norm.*, encoder.layer_norm.*

This list is RESTATED from the published fairseq module; no upstream source or checkpoint was at hand to verify it against.
``convert_hf_state_dict`` maps a ``transformers`` ``Wav2Vec2Model`` state dict onto it.

Ragged batches: a channel of conv 0 is normalised over the frames of its own row, so row b of a padded batch equals the B = 1 run
on its own ``lengths[b]`` samples for every frame below ``frames[b]`` (the reference only ever calls with B = 1: this choice
DEFINES the ragged case); frames at or beyond it hold finite values that mean nothing."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from .. import _C, ops
from ..xfmr_f32 import fold, layer
from .wavlm import WaveEncoder, _Holder, _WeightNormConv, frame_counts

Tensor = torch.Tensor
F32, I32 = torch.float32, torch.int32


@dataclass
class Wav2Vec2Config:
    """Defaults = wav2vec2-base."""
    conv_dim: Tuple[int, ...] = (512,) * 7
    conv_kernel: Tuple[int, ...] = (10, 3, 3, 3, 3, 2, 2)
    conv_stride: Tuple[int, ...] = (5, 2, 2, 2, 2, 2, 2)
    conv_bias: bool = False
    extractor_mode: str = "default"
    layer_norm_first: bool = False
    normalize: bool = False
    encoder_embed_dim: int = 768
    encoder_layers: int = 12
    encoder_attention_heads: int = 12
    encoder_ffn_embed_dim: int = 3072
    conv_pos: int = 128
    conv_pos_groups: int = 16
    layer_norm_eps: float = 1e-5

    def check(self) -> None:
        def refuse(field, why):
            raise _C.F5EError(f"Wav2Vec2: {field} = {getattr(self, field)!r} is not built: {why}")
        if self.extractor_mode != "default":
            refuse("extractor_mode", "only the group-norm (\"default\") feature extractor of the base family is (the layer-norm "
                                     "extractor is eval/wavlm.py's)")
        if self.layer_norm_first:
            refuse("layer_norm_first", "only the post-LayerNorm encoder of the base family is")
        if self.normalize:
            refuse("normalize", "the base family takes the raw waveform")
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
        if D % H or D // H not in (16, 32, 64, 128):
            refuse("encoder_attention_heads", f"head dim {D / H:g} (16, 32, 64 and 128 are)")
        if D % self.conv_pos_groups or (D // self.conv_pos_groups) % 4:
            refuse("conv_pos_groups", "encoder_embed_dim / conv_pos_groups must be a multiple of 4")
        if self.encoder_ffn_embed_dim % 4:
            refuse("encoder_ffn_embed_dim", "a multiple of 4")


_HF_LAYER = {"attention.q_proj": "self_attn.q_proj", "attention.k_proj": "self_attn.k_proj", "attention.v_proj": "self_attn.v_proj",
             "attention.out_proj": "self_attn.out_proj", "layer_norm": "self_attn_layer_norm",
             "feed_forward.intermediate_dense": "fc1", "feed_forward.output_dense": "fc2", "final_layer_norm": "final_layer_norm"}
_HF_POS = {"parametrizations.weight.original0": "weight_g", "parametrizations.weight.original1": "weight_v", "weight_g": "weight_g",
           "weight_v": "weight_v", "bias": "bias"}


def convert_hf_state_dict(sd: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """``transformers`` ``Wav2Vec2Model`` names -> the fairseq names of this module (a leading ``wav2vec2.`` is dropped;
    ``masked_spec_embed``, which inference never reads, is dropped too).  Keys that belong to nothing built here (adapters,
    quantizers, the layer norms of a layer-norm extractor) raise."""
    out = {}
    for key, val in sd.items():
        k = key[len("wav2vec2."):] if key.startswith("wav2vec2.") else key
        p = k.split(".")
        new = None
        if k == "masked_spec_embed":
            continue
        if p[0] == "feature_extractor" and p[1] == "conv_layers" and len(p) == 5:
            if p[3] == "conv":
                new = f"feature_extractor.conv_layers.{p[2]}.0.{p[4]}"
            elif p[3] == "layer_norm" and p[2] == "0":                  # the GroupNorm of layer 0 is called layer_norm there
                new = f"feature_extractor.conv_layers.0.2.{p[4]}"
        elif k.startswith("feature_projection.layer_norm."):
            new = "layer_norm." + p[-1]
        elif k.startswith("feature_projection.projection."):
            new = "post_extract_proj." + p[-1]
        elif k.startswith("encoder.pos_conv_embed.conv."):
            new = "encoder.pos_conv.0." + _HF_POS[".".join(p[3:])] if ".".join(p[3:]) in _HF_POS else None
        elif k.startswith("encoder.layer_norm."):
            new = k
        elif p[0] == "encoder" and p[1] == "layers" and len(p) >= 5:
            mod, leaf = ".".join(p[3:]).rsplit(".", 1)
            if mod in _HF_LAYER:
                new = f"encoder.layers.{p[2]}.{_HF_LAYER[mod]}.{leaf}"
        if new is None:
            raise KeyError(f"convert_hf_state_dict: {key} has no counterpart")
        out[new] = val
    return out


class _SelfAttn(nn.Module):
    def __init__(self, D: int):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj, self.out_proj = (nn.Linear(D, D) for _ in range(4))


class _Layer(nn.Module):
    def __init__(self, cfg: Wav2Vec2Config):
        super().__init__()
        D = cfg.encoder_embed_dim
        self.self_attn = _SelfAttn(D)
        self.self_attn_layer_norm = nn.LayerNorm(D, eps=cfg.layer_norm_eps)
        self.fc1, self.fc2 = nn.Linear(D, cfg.encoder_ffn_embed_dim), nn.Linear(cfg.encoder_ffn_embed_dim, D)
        self.final_layer_norm = nn.LayerNorm(D, eps=cfg.layer_norm_eps)


class _Encoder(nn.Module):
    def __init__(self, cfg: Wav2Vec2Config):
        super().__init__()
        D = cfg.encoder_embed_dim
        self.pos_conv = nn.Sequential(_WeightNormConv(D, cfg.conv_pos, cfg.conv_pos_groups))
        self.layers = nn.ModuleList([_Layer(cfg) for _ in range(cfg.encoder_layers)])
        self.layer_norm = nn.LayerNorm(D, eps=cfg.layer_norm_eps)


class _FeatureExtractor(nn.Module):
    def __init__(self, cfg: Wav2Vec2Config):
        super().__init__()
        layers, cin = [], 1
        for i, (c, k, s) in enumerate(zip(cfg.conv_dim, cfg.conv_kernel, cfg.conv_stride)):   # conv, dropout, [GroupNorm,] GELU
            conv = nn.Conv1d(cin, c, k, stride=s, bias=cfg.conv_bias)
            layers.append(nn.Sequential(conv, _Holder(), nn.GroupNorm(c, c, eps=cfg.layer_norm_eps), _Holder()) if i == 0
                          else nn.Sequential(conv, _Holder(), _Holder()))
            cin = c
        self.conv_layers = nn.ModuleList(layers)


class Wav2Vec2(WaveEncoder):
    _conv_act = ops.ACT_GELU_ERF                # no norm after convs 1..: the GELU rides on the GEMM

    def __init__(self, cfg: Optional[Wav2Vec2Config] = None):
        super().__init__()
        self.cfg = cfg = cfg or Wav2Vec2Config()
        cfg.check()
        C, D = cfg.conv_dim[-1], cfg.encoder_embed_dim
        self.feature_extractor = _FeatureExtractor(cfg)
        self.layer_norm = nn.LayerNorm(C, eps=cfg.layer_norm_eps)
        self.post_extract_proj = nn.Linear(C, D)
        self.encoder = _Encoder(cfg)
        self._freeze()

    def _fold_more(self, fd: dict, dev) -> None:
        fd["gn_g"], fd["gn_b"] = fold(dev, self.feature_extractor.conv_layers[0][2])

    # ---- geometry and workspace ---------------------------------------------------------------------------------------------
    def _geometry(self, S: int) -> Tuple[int, List[int], List[int]]:
        """``WaveEncoder._geometry`` (T, need, pitch), with the batch pitch of layer 0 raised to hold ALL (S - 10) // 5 + 1 frames
        of conv 0: the group norm runs over every one of them, also over those that no later layer reads."""
        cfg = self.cfg
        T, need, pitch = super()._geometry(S)
        T0 = frame_counts(S, cfg)[0]
        while pitch[0] < T0:
            pitch = [p + math.prod(cfg.conv_stride[l + 1:]) for l, p in enumerate(pitch)]
        return T, need, pitch

    def _shapes(self, B: int, S: int, T: int, **conv) -> Dict[str, tuple]:
        cfg = self.cfg
        C, D, M = cfg.conv_dim[-1], cfg.encoder_embed_dim, B * T
        return dict(frames=(B,), partials=(ops.w2v_conv0_gn_partials(B, max(S, 10), C),), mask=(M,), **conv, xnc=(M, C),
                    proj=(M, D), qkv=(M, 3 * D), ao=(M, D), ff=(M, cfg.encoder_ffn_embed_dim))

    # ---- forward -------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def extract(self, wav: Tensor, lengths=None, *, out: Optional[Tensor] = None, workspace: Optional[Tensor] = None):
        """wav f32 [B, S] on the GPU, 16 kHz, raw; lengths: samples per row, i32 [B] on the device (None: S; a host sequence is
        validated and uploaded, which allocates) -> (last hidden state f32 [B, T, D], frames i32 [B]); ``frames`` is a view of the
        workspace, valid until the next call on it.  No device-to-host copy, no synchronisation; with ``out``, ``workspace``
        (``workspace_bytes(B, S)`` bytes, f32 or uint8) and device lengths it allocates nothing once the weights are folded (a
        first call does that), so it can be captured into a graph."""
        cfg = self.cfg
        wav, lengths, fd, buf = self._enter(wav, lengths, workspace)
        (B, S), (T, _need, pitch) = wav.shape, self._geometry(wav.shape[1])
        C, D, H = cfg.conv_dim[-1], cfg.encoder_embed_dim, cfg.encoder_attention_heads
        if out is None:
            out = torch.empty(B, T, D, dtype=F32, device=wav.device)
        elif out.shape != (B, T, D) or out.dtype != F32 or not out.is_cuda or not out.is_contiguous() or out.data_ptr() % 16:
            raise _C.F5EError(f"Wav2Vec2.extract: out must be a contiguous 16-byte aligned f32 GPU tensor [{B}, {T}, {D}]")
        M, eps = B * T, cfg.layer_norm_eps
        frames = buf("frames").view(I32)
        cur, c0 = buf("ca"), fd["conv"][0]      # the conv front-end: layer 0 in two launches (statistics over time, apply)
        ops.w2v_conv0_gn(wav, c0["w"], c0["b"], fd["gn_g"], fd["gn_b"], lengths, cur[:B * pitch[0] * C].view(B, pitch[0], C),
                         buf("partials"), frames, buf("mask").view(B, T), cfg.conv_kernel, cfg.conv_stride, eps)
        proj = self._project(fd, buf, cur, buf("cb"), B, T, pitch)
        ops.wavlm_posconv(proj.view(B, T, D), fd["pos_w"], fd["pos_b"], frames, out)
        x = out.view(M, D)
        ops.layernorm(x, x, fd["enc_g"], fd["enc_b"], eps=eps)
        bufs, scale = (None, buf("qkv"), buf("ao"), None, buf("ff")), (D // H) ** -0.5

        def self_attn(_W, _x, qkv, ao):
            ops.mha_f32(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], H, scale, B=B, kv_len=frames, out=ao)

        for W in fd["layers"]:                                                          # post-LN: x = LN(x + f(x))
            layer(x, x, W, bufs, pre_norm=False, act=ops.ACT_GELU_ERF, eps=eps, self_attn=self_attn)
        return out, frames
