"""CPU fp32 restatement of the recogniser's encoder on the reference's 4x / 6x / 8x subsampling fronts and with
``cnn_module_norm: layer_norm``: full context, ``forward_chunk`` with its caches, the chunk-by-chunk loop, the CTC head.

TEST INFRASTRUCTURE ONLY (same rule as tests/ppg_stream_ref.py, whose attention it reuses): written from a reading of
``Conv2dSubsampling2 / 4 / 6 / 8`` (ppg/wenet/transformer/subsampling.py:68-280), ``ConvolutionModule.forward``
(convolution.py:81-134, both norms), ``BaseEncoder.forward`` / ``forward_chunk`` / ``forward_chunk_by_chunk``
(encoder.py:141-355) and ``CTC.log_softmax`` (ctc.py:52-60); pinned by ``tests/golden/asr_subsample_{4,6,8}.npz``
(``tests/golden/make_asr_subsample_golden.py``, the reference's own ``init_asr_model``).  State dicts are flat, with the
reference's key names.  The decode helpers restate ``ctc_greedy_search`` / ``ctc_prefix_beam_search`` on log-probabilities
through tests/ctc_ref.py and tests/ctc_beam_ref.py."""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import ctc_beam_ref
import ctc_ref
from oracle import f5e_ppg_oracle as P
from ppg_stream_ref import rel_mha_cached

Tensor = torch.Tensor
State = Dict[str, Tensor]
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RATES = (4, 6, 8)
# (kernel, stride) of every convolution of the stack, the mask slice each one applies, the name of the Linear
CONVS = {2: ((3, 2),), 4: ((3, 2), (3, 2)), 6: ((3, 2), (5, 3)), 8: ((3, 2), (3, 2), (3, 2))}
RIGHT_CONTEXT = {2: 2, 4: 6, 6: 10, 8: 14}          # subsampling.py:92, 147, 200, 254
INPUT_LAYER = {2: "conv2d", 4: "conv2d4", 6: "conv2d6", 8: "conv2d8"}
CNN_NORM = {4: "layer_norm", 6: "batch_norm", 8: "batch_norm"}      # what the fixtures use


def fixture_config(rate: int) -> dict:
    """The config ``make_asr_subsample_golden.py`` hands to ``init_asr_model`` for this rate."""
    return dict(cmvn_file=None, is_json_cmvn=True, input_dim=80, output_dim=30, encoder="conformer", decoder="transformer",
                encoder_conf=dict(output_size=64, attention_heads=4, linear_units=64, num_blocks=2,
                                  cnn_module_kernel=7, use_dynamic_chunk=True, causal=rate == 8,
                                  input_layer=INPUT_LAYER[rate], cnn_module_norm=CNN_NORM[rate]),
                decoder_conf=dict(attention_heads=4, linear_units=32, num_blocks=1),
                model_conf=dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False, sv_conf=dict(use_sv=False)))


_cache: Dict[int, Tuple[State, Dict[str, Tensor]]] = {}


def load_fixture(rate: int) -> Tuple[State, Dict[str, Tensor]]:
    """(state dict, everything else) of asr_subsample_<rate>.npz, fp16 storage widened to fp32; loaded once, shared."""
    if rate not in _cache:
        sd, g = {}, {}
        z = np.load(os.path.join(GOLD, f"asr_subsample_{rate}.npz"), allow_pickle=False)
        for k in z.files:
            t = torch.from_numpy(z[k])
            t = t.float() if t.dtype == torch.float16 else t
            if k.startswith("w/"):
                sd[k[2:]] = t
            else:
                g[k] = t
        _cache[rate] = (sd, g)
    return _cache[rate]


def rate_of(sd: State) -> int:
    if "encoder.embed.conv.2.weight" not in sd:
        return 2
    if "encoder.embed.conv.4.weight" in sd:
        return 8
    return 6 if sd["encoder.embed.conv.2.weight"].shape[-1] == 5 else 4


def out_frames(n: int, rate: int) -> int:
    for k, s in CONVS[rate]:
        n = (n - k) // s + 1 if n >= k else 0
    return n


def sub_mask(mask: Tensor, rate: int) -> Tensor:
    """``x_mask[:, :, :-2:2]``, then ``[:, :, :-2:2]`` or ``[:, :, :-4:3]`` ... as the forward of each class slices it."""
    for k, s in CONVS[rate]:
        mask = mask[:, :, :-(k - 1):s]
    return mask


def subsampling(sd: State, p: str, x: Tensor, mask: Tensor) -> Tuple[Tensor, Tensor]:
    """Conv2dSubsamplingN.forward + the xscale of RelPositionalEncoding -> (x sqrt(d) [B, T', D], mask [B, 1, T']).
    Padded frames are convolved as they are."""
    rate = rate_of(sd)
    h = x.unsqueeze(1)
    for i, (_, s) in enumerate(CONVS[rate]):
        h = F.relu(F.conv2d(h, sd[f"{p}conv.{2 * i}.weight"], sd[f"{p}conv.{2 * i}.bias"], stride=s))
    b, c, t, f = h.shape
    lin = "out.0." if rate in (2, 4) else "linear."
    h = F.linear(h.transpose(1, 2).contiguous().view(b, t, c * f), sd[p + lin + "weight"], sd[p + lin + "bias"])
    return h * math.sqrt(h.shape[-1]), sub_mask(mask, rate)


def conv_module(sd: State, p: str, x: Tensor, mask_pad: Optional[Tensor], cache: Optional[Tensor],
                causal: bool) -> Tuple[Tensor, Tensor]:
    """ConvolutionModule.forward(x, mask_pad, cache) (convolution.py:81-134), either norm."""
    h = x.transpose(1, 2)
    if mask_pad is not None:
        h = h.masked_fill(~mask_pad, 0.0)
    w = sd[p + "depthwise_conv.weight"]
    lorder = w.shape[-1] - 1
    if causal:
        h = F.pad(h, (lorder, 0)) if cache is None else torch.cat((cache, h), dim=2)
        new_cache = h[:, :, -lorder:]
    else:
        new_cache = torch.tensor([0.0])
    h = F.glu(F.conv1d(h, sd[p + "pointwise_conv1.weight"], sd[p + "pointwise_conv1.bias"]), dim=1)
    h = F.conv1d(h, w, sd[p + "depthwise_conv.bias"], padding=0 if causal else lorder // 2, groups=w.shape[0])
    if p + "norm.running_mean" in sd:
        h = F.batch_norm(h, sd[p + "norm.running_mean"], sd[p + "norm.running_var"], sd[p + "norm.weight"],
                         sd[p + "norm.bias"], training=False, eps=1e-5)
    else:
        h = F.layer_norm(h.transpose(1, 2), (h.shape[1],), sd[p + "norm.weight"], sd[p + "norm.bias"], eps=1e-5).transpose(1, 2)
    h = F.conv1d(F.silu(h), sd[p + "pointwise_conv2.weight"], sd[p + "pointwise_conv2.bias"])
    if mask_pad is not None:
        h = h.masked_fill(~mask_pad, 0.0)
    return h.transpose(1, 2), new_cache


def layer(sd: State, p: str, x: Tensor, pos_emb: Tensor, heads: int, causal: bool, mask: Optional[Tensor] = None,
          output_cache: Optional[Tensor] = None, cnn_cache: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """ConformerEncoderLayer.forward (encoder_layer.py:179-268): ``mask`` [B, 1, T] for a full-context ragged batch (pad mask
    and attention mask are the same there), or the caches of ``forward_chunk``."""
    ln = lambda n, v: F.layer_norm(v, (v.shape[-1],), sd[p + n + ".weight"], sd[p + n + ".bias"], eps=1e-5)   # noqa: E731
    ff = lambda n, v: F.linear(F.silu(F.linear(v, sd[p + n + ".w_1.weight"], sd[p + n + ".w_1.bias"])),           # noqa: E731
                               sd[p + n + ".w_2.weight"], sd[p + n + ".w_2.bias"])
    x = x + 0.5 * ff("feed_forward_macaron", ln("norm_ff_macaron", x))
    h = ln("norm_mha", x)
    if mask is not None:
        x = x + P.rel_mha(sd, p + "self_attn.", h, mask, pos_emb, heads)
    else:
        chunk = x.shape[1] - (0 if output_cache is None else output_cache.shape[1])
        x = x[:, -chunk:] + rel_mha_cached(sd, p + "self_attn.", h[:, -chunk:], h, pos_emb, heads)
    c, new_cnn = conv_module(sd, p + "conv_module.", ln("norm_conv", x), mask, cnn_cache, causal)
    x = x + c
    x = x + 0.5 * ff("feed_forward", ln("norm_ff", x))
    x = ln("norm_final", x)
    if output_cache is not None:
        x = torch.cat([output_cache, x], dim=1)
    return x, new_cnn


def _cmvn(sd: State, x: Tensor) -> Tensor:
    if "encoder.global_cmvn.mean" in sd:
        return (x - sd["encoder.global_cmvn.mean"]) * sd["encoder.global_cmvn.istd"]
    return x


def _after(sd: State, x: Tensor) -> Tensor:
    return F.layer_norm(x, (x.shape[-1],), sd["encoder.after_norm.weight"], sd["encoder.after_norm.bias"], eps=1e-5)


def embed(sd: State, feats: Tensor, lens: Tensor) -> Tuple[Tensor, Tensor]:
    masks = (torch.arange(feats.shape[1])[None, :] < lens[:, None]).unsqueeze(1)
    return subsampling(sd, "encoder.embed.", _cmvn(sd, feats), masks)


def encoder(sd: State, feats: Tensor, lens: Tensor, heads: int = 4, causal: bool = False) -> Tuple[Tensor, Tensor]:
    """BaseEncoder.forward with the full context (decoding_chunk_size < 0) -> (xs [B, T', D], masks [B, 1, T'])."""
    x, masks = embed(sd, feats, lens)
    pos_emb = P.rel_pos_table(x.shape[1], x.shape[2])
    for i in range(P.encoder_depth(sd)):
        x, _ = layer(sd, f"encoder.encoders.{i}.", x, pos_emb, heads, causal, mask=masks)
    return _after(sd, x), masks


def forward_chunk(sd: State, xs: Tensor, offset: int, required_cache_size: int, subsampling_cache: Optional[Tensor] = None,
                  elayers_output_cache: Optional[List[Tensor]] = None, conformer_cnn_cache: Optional[List[Tensor]] = None,
                  heads: int = 4, causal: bool = False):
    """BaseEncoder.forward_chunk (encoder.py:210-291)."""
    assert xs.shape[0] == 1
    x, _ = subsampling(sd, "encoder.embed.", _cmvn(sd, xs), torch.ones(1, 1, xs.shape[1], dtype=torch.bool))
    cache_size = 0
    if subsampling_cache is not None:
        cache_size = subsampling_cache.shape[1]
        x = torch.cat((subsampling_cache, x), dim=1)
    n = x.shape[1]
    pos_emb = P.rel_pos_table(offset + n, x.shape[2])[:, offset - cache_size:offset - cache_size + n]
    start = 0 if required_cache_size < 0 else (n if required_cache_size == 0 else max(n - required_cache_size, 0))
    r_sub, r_att, r_cnn = x[:, start:], [], []
    for i in range(P.encoder_depth(sd)):
        x, cnn = layer(sd, f"encoder.encoders.{i}.", x, pos_emb, heads, causal,
                       output_cache=None if elayers_output_cache is None else elayers_output_cache[i],
                       cnn_cache=None if conformer_cnn_cache is None else conformer_cnn_cache[i])
        r_att.append(x[:, start:])
        r_cnn.append(cnn)
    return _after(sd, x)[:, cache_size:], r_sub, r_att, r_cnn


def loop_bounds(num_frames: int, chunk: int, rate: int) -> List[Tuple[int, int]]:
    """The loop of forward_chunk_by_chunk transcribed (encoder.py:328-343), for the tests of the window arithmetic."""
    subsampling_rate = rate
    context = RIGHT_CONTEXT[rate] + 1
    stride = subsampling_rate * chunk
    decoding_window = (chunk - 1) * subsampling_rate + context
    out = []
    for cur in range(0, num_frames - context + 1, stride):
        end = min(cur + decoding_window, num_frames)
        out.append((cur, end))
    return out


def forward_chunk_by_chunk(sd: State, xs: Tensor, chunk: int, left_chunks: int = -1, heads: int = 4,
                           causal: bool = False) -> Tensor:
    sub = att = cnn = None
    outs, offset = [], 0
    for cur, end in loop_bounds(xs.shape[1], chunk, rate_of(sd)):
        y, sub, att, cnn = forward_chunk(sd, xs[:, cur:end], offset, chunk * left_chunks, sub, att, cnn, heads, causal)
        outs.append(y)
        offset += y.shape[1]
    return torch.cat(outs, 1)


def ctc_log_probs(sd: State, enc: Tensor) -> Tensor:
    """CTC.log_softmax (ctc.py:52-60)."""
    return F.log_softmax(F.linear(enc, sd["ctc.ctc_lo.weight"], sd["ctc.ctc_lo.bias"]), dim=2)


def greedy_ids(log_probs: Tensor) -> List[int]:
    """ctc_greedy_search of one utterance's log-probabilities [T, V]."""
    return ctc_ref.greedy(log_probs[None].numpy(), [log_probs.shape[0]])[0][0]


def beam_nbest(log_probs: Tensor, beam: int):
    """ctc_prefix_beam_search of one utterance's log-probabilities [T, V] -> (list of (ids, score) best first, margin)."""
    return ctc_beam_ref.search(log_probs.numpy(), beam)
