"""CPU fp32 restatement of the chunk-by-chunk (streaming) mode of the PPG extractor, caches and all.

TEST INFRASTRUCTURE ONLY (same rule as oracle/f5e_ppg_oracle.py, whose row-wise pieces it reuses): written from a reading of
``ASRModel.extract(stream=True)`` (ppg/asr_model.py:222-244), ``BaseEncoder.forward_chunk`` / ``forward_chunk_by_chunk``
(ppg/wenet/transformer/encoder.py:210-355), ``ConformerEncoderLayer.forward`` with an output cache (encoder_layer.py:179-268)
and ``ConvolutionModule.forward`` with a cache (convolution.py:81-134); pinned by ``tests/golden/ppg_stream_*.npz``
(``tests/golden/make_ppg_stream_golden.py``, the reference's own classes).  It is what the GPU tests compare against at
sizes the fixtures do not cover.  State dicts are flat, with the reference's key names."""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import f5e_ppg_oracle as P

Tensor = torch.Tensor
State = Dict[str, Tensor]
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_stream_fixture(causal: bool) -> Tuple[State, Dict[str, Tensor]]:
    """(state dict, everything else) of ppg_stream_common.npz + ppg_stream_causal{0,1}.npz, fp16 storage widened to fp32."""
    sd, g = {}, {}
    for name in ("ppg_stream_common.npz", f"ppg_stream_causal{int(causal)}.npz"):
        z = np.load(os.path.join(GOLD, name), allow_pickle=False)
        for k in z.files:
            t = torch.from_numpy(z[k])
            t = t.float() if t.dtype == torch.float16 else t
            if k.startswith("w/"):
                sd[k[2:]] = t
            else:
                g[k] = t
    return sd, g


def rel_mha_cached(sd: State, p: str, xq: Tensor, x: Tensor, pos_emb: Tensor, heads: int) -> Tensor:
    """RelPositionMultiHeadedAttention.forward(x_q, x, x, all-ones mask, pos_emb) (attention.py:172-222): queries are the
    new rows, keys / values the cached rows plus the new rows, the position term indexed by the key."""
    b, tq, d = xq.shape
    t, dk = x.shape[1], d // heads
    lin = lambda n, v: F.linear(v, sd[p + n + ".weight"], sd.get(p + n + ".bias"))   # noqa: E731
    q = lin("linear_q", xq).view(b, tq, heads, dk)
    k = lin("linear_k", x).view(b, t, heads, dk).transpose(1, 2)
    v = lin("linear_v", x).view(b, t, heads, dk).transpose(1, 2)
    pp = lin("linear_pos", pos_emb).view(pos_emb.shape[0], -1, heads, dk).transpose(1, 2)
    qu = (q + sd[p + "pos_bias_u"]).transpose(1, 2)
    qv = (q + sd[p + "pos_bias_v"]).transpose(1, 2)
    scores = (qu @ k.transpose(-2, -1) + qv @ pp.transpose(-2, -1)) / math.sqrt(dk)
    ctx = (torch.softmax(scores, dim=-1) @ v).transpose(1, 2).contiguous().view(b, tq, d)
    return lin("linear_out", ctx)


def conv_module_cached(sd: State, p: str, x: Tensor, cache: Optional[Tensor], causal: bool) -> Tuple[Tensor, Tensor]:
    """ConvolutionModule.forward(x, None, cache) (convolution.py:81-134).  causal: ``kernel - 1`` frames of left context
    BEFORE pointwise_conv1 (zeros at the start of an utterance, the cache [B, C, kernel - 1] afterwards); otherwise the
    chunk is convolved on its own with zero padding on both sides and the cache is a dummy."""
    h = x.transpose(1, 2)
    w = sd[p + "depthwise_conv.weight"]
    lorder = w.shape[-1] - 1
    if causal:
        h = F.pad(h, (lorder, 0)) if cache is None else torch.cat((cache, h), dim=2)
        new_cache = h[:, :, -lorder:]
    else:
        new_cache = torch.tensor([0.0])
    h = F.glu(F.conv1d(h, sd[p + "pointwise_conv1.weight"], sd[p + "pointwise_conv1.bias"]), dim=1)
    h = F.conv1d(h, w, sd[p + "depthwise_conv.bias"], padding=0 if causal else lorder // 2, groups=w.shape[0])
    h = F.batch_norm(h, sd[p + "norm.running_mean"], sd[p + "norm.running_var"], sd[p + "norm.weight"], sd[p + "norm.bias"],
                     training=False, eps=1e-5)
    h = F.conv1d(F.silu(h), sd[p + "pointwise_conv2.weight"], sd[p + "pointwise_conv2.bias"])
    return h.transpose(1, 2), new_cache


def conformer_layer_cached(sd: State, p: str, x: Tensor, pos_emb: Tensor, output_cache: Optional[Tensor],
                           cnn_cache: Optional[Tensor], heads: int, causal: bool) -> Tuple[Tensor, Tensor]:
    """ConformerEncoderLayer.forward with output_cache / cnn_cache (encoder_layer.py:179-268): x holds the cached rows of the
    PREVIOUS layer's output followed by the new rows; only the new rows are computed past the key / value projection."""
    ln = lambda n, v: F.layer_norm(v, (v.shape[-1],), sd[p + n + ".weight"], sd[p + n + ".bias"], eps=1e-5)   # noqa: E731
    ff = lambda n, v: F.linear(F.silu(F.linear(v, sd[p + n + ".w_1.weight"], sd[p + n + ".w_1.bias"])),           # noqa: E731
                               sd[p + n + ".w_2.weight"], sd[p + n + ".w_2.bias"])
    x = x + 0.5 * ff("feed_forward_macaron", ln("norm_ff_macaron", x))
    h = ln("norm_mha", x)
    chunk = x.shape[1] - (0 if output_cache is None else output_cache.shape[1])
    x = x[:, -chunk:] + rel_mha_cached(sd, p + "self_attn.", h[:, -chunk:], h, pos_emb, heads)
    c, new_cnn_cache = conv_module_cached(sd, p + "conv_module.", ln("norm_conv", x), cnn_cache, causal)
    x = x + c
    x = x + 0.5 * ff("feed_forward", ln("norm_ff", x))
    x = ln("norm_final", x)
    if output_cache is not None:
        x = torch.cat([output_cache, x], dim=1)
    return x, new_cnn_cache


def forward_chunk(sd: State, xs: Tensor, offset: int, required_cache_size: int, subsampling_cache: Optional[Tensor] = None,
                  elayers_output_cache: Optional[List[Tensor]] = None, conformer_cnn_cache: Optional[List[Tensor]] = None,
                  heads: int = 4, causal: bool = False) -> Tuple[Tensor, Tensor, List[Tensor], List[Tensor]]:
    """BaseEncoder.forward_chunk (encoder.py:210-291)."""
    assert xs.shape[0] == 1
    if "encoder.global_cmvn.mean" in sd:
        xs = (xs - sd["encoder.global_cmvn.mean"]) * sd["encoder.global_cmvn.istd"]
    ones = torch.ones(1, 1, xs.shape[1], dtype=torch.bool)
    x, _, _ = P.conv2d_subsampling2(sd, "encoder.embed.", xs, ones)
    cache_size = 0
    if subsampling_cache is not None:
        cache_size = subsampling_cache.shape[1]
        x = torch.cat((subsampling_cache, x), dim=1)
    n = x.shape[1]
    pos_emb = P.rel_pos_table(offset + n, x.shape[2])[:, offset - cache_size:offset - cache_size + n]
    if required_cache_size < 0:
        start = 0
    elif required_cache_size == 0:
        start = n
    else:
        start = max(n - required_cache_size, 0)
    r_sub, r_att, r_cnn = x[:, start:], [], []
    for i in range(P.encoder_depth(sd)):
        x, cnn = conformer_layer_cached(sd, f"encoder.encoders.{i}.", x, pos_emb,
                                        None if elayers_output_cache is None else elayers_output_cache[i],
                                        None if conformer_cnn_cache is None else conformer_cnn_cache[i], heads, causal)
        r_att.append(x[:, start:])
        r_cnn.append(cnn)
    x = F.layer_norm(x, (x.shape[-1],), sd["encoder.after_norm.weight"], sd["encoder.after_norm.bias"], eps=1e-5)
    return x[:, cache_size:], r_sub, r_att, r_cnn


def stream_windows(num_frames: int, chunk: int, subsampling: int = 2, right_context: int = 2):
    """The (start, end) feature windows of forward_chunk_by_chunk (encoder.py:328-343): overlapping windows of
    ``(chunk - 1) * subsampling + right_context + 1`` frames at stride ``subsampling * chunk``; the loop bound
    ``num_frames - context + 1`` decides how many there are."""
    context = right_context + 1
    window = (chunk - 1) * subsampling + context
    return [(cur, min(cur + window, num_frames)) for cur in range(0, num_frames - context + 1, subsampling * chunk)]


def forward_chunk_by_chunk(sd: State, xs: Tensor, decoding_chunk_size: int, num_decoding_left_chunks: int = -1,
                           heads: int = 4, causal: bool = False) -> Tensor:
    """BaseEncoder.forward_chunk_by_chunk (encoder.py:293-355) -> encoder output [1, T', D]."""
    assert decoding_chunk_size > 0
    sub = att = cnn = None
    outs, offset = [], 0
    for cur, end in stream_windows(xs.shape[1], decoding_chunk_size):
        y, sub, att, cnn = forward_chunk(sd, xs[:, cur:end], offset, decoding_chunk_size * num_decoding_left_chunks, sub, att,
                                         cnn, heads, causal)
        outs.append(y)
        offset += y.shape[1]
    return torch.cat(outs, 1)


def asr_extract_stream(sd: State, feats: Tensor, heads: int = 4, causal: bool = False, chunk: int = 16,
                       left_chunks: int = 17) -> Tuple[Tensor, Tensor]:
    """ASRModel.extract(stream=True) (asr_model.py:222-244) -> (ppg [1, T', D], logits [T', vocab + 1])."""
    enc = forward_chunk_by_chunk(sd, feats, chunk, left_chunks, heads, causal)
    out = F.linear(enc, sd["linear.weight"], sd["linear.bias"])
    return out, F.linear(out.flatten(0, 1), sd["ce.fc.weight"], sd["ce.fc.bias"])


def seeded_state(model: torch.nn.Module, seed: int) -> State:
    """Seeded values for every entry of a ConformerPPG state dict (norm weights near 1, biases near 0, BatchNorm buffers
    and CMVN away from their defaults, matrices uniform at 1 / sqrt(fan_in)); the recipe of tests/test_ppg_gpu.py."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = v.clone()
        elif k.endswith("running_var"):
            sd[k] = 1.0 + 0.2 * torch.rand(v.shape, generator=g)
        elif k.endswith("running_mean") or k.endswith("global_cmvn.mean"):
            sd[k] = 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith("global_cmvn.istd"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        elif v.ndim == 1:
            base = 1.0 if ("norm" in k and k.endswith("weight")) else 0.0
            sd[k] = base + 0.1 * torch.randn(v.shape, generator=g)
        else:
            sd[k] = (torch.rand(v.shape, generator=g) * 2 - 1) / math.sqrt(v[0].numel())
    return sd
