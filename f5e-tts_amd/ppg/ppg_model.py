"""PPG extractor mirror (reference ppg/ppg_model.py:11-168, ppg/asr_model.py:221-244 + 814-859, ppg/wenet/transformer/*):
kaldi fbank -> GlobalCMVN -> wenet ConformerEncoder -> 256-d ``linear`` head (the "PPG") -> ``ce.fc`` logits, behind the
reference's ``build_ppg_model`` / ``PPGModelWapper`` API.  It runs once per utterance in front of ``CFM.sample_vc`` /
``sample_tts`` (reference eval/eval_infer_batch_vc.py, model/trainer.py:385-389).

Everything is computed by libf5e_hip.so: the linears, the per-head score / context products and the subsampling conv
(as one Toeplitz-expanded GEMM) on the exact-fp32 MFMA GEMM, LayerNorms, GLU, depthwise conv, row softmax and the fbank
FFT as HIP kernels; torch only holds memory.  Weights-only transforms done once at load: eval-mode BatchNorm and the
global CMVN are folded into the adjacent convolution weights, ``pos_bias_u / v`` into the query projection's bias.

What is built is the configuration the reference ships (``encoder: conformer``, ``input_layer: conv2d`` = 1/2
subsampling for 20 ms PPG frames, ``rel_pos``, macaron feed-forward, convolution module with batch norm, swish, pre-norm,
``causal`` either way).  ``extract(stream=False)`` decodes with the full context; ``extract(stream=True)`` reproduces the
reference's chunk-by-chunk loop (``BaseEncoder.forward_chunk_by_chunk(speech, 16, 17)``, encoder.py:293-355) as ONE pass
with a banded attention kernel (``f5e_relpos_attn``) and a chunk-isolated or causal depthwise convolution
(``f5e_dwconv_stream``); ``forward_encoder_chunk`` is the incremental form with explicit caches.

``ConformerPPG.from_asr_config`` / ``build_asr_model`` build the same model as a RECOGNISER on stock wenet encoders: the
reference's 4x / 6x / 8x fronts (``input_layer: conv2d4 / conv2d6 / conv2d8``, Conv2dSubsampling4 / 6 / 8; their C -> C
strided convolutions run as an implicit GEMM, ``f5e_conv2d_sub_f32``) and ``cnn_module_norm: layer_norm``.  The extractor's
own door (``from_config`` / ``build_ppg_model``) stays 2x and batch-norm: the DiT needs 20 ms PPGs.  Other encoder variants
raise F5EError.
"""
from __future__ import annotations

import json
import math
import os
from functools import partial
from types import SimpleNamespace
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import nn

from .. import _C, ops
from ..xfmr_f32 import fold_layer, layer

F32, I32 = torch.float32, torch.int32
Tensor = torch.Tensor


def load_cmvn(cmvn_file: str, is_json: bool) -> Tuple[np.ndarray, np.ndarray]:
    """(mean, 1 / std) from accumulated statistics (reference ppg/wenet/utils/cmvn.py:21-92; json or kaldi text)."""
    if is_json:
        with open(cmvn_file) as f:
            st = json.load(f)
        means, var, count = list(st["mean_stat"]), list(st["var_stat"]), st["frame_num"]
    else:
        with open(cmvn_file, "r") as f:
            arr = f.read().split()
        if not (arr[0] == "[" and arr[-2] == "0" and arr[-1] == "]"):
            raise ValueError("kaldi cmvn: expected the text format of compute-cmvn-stats --binary=false")
        dim = (len(arr) - 4) // 2
        means = [float(v) for v in arr[1:dim + 1]]
        count = float(arr[dim + 1])
        var = [float(v) for v in arr[dim + 2:2 * dim + 2]]
    for i in range(len(means)):
        means[i] /= count
        var[i] = max(var[i] / count - means[i] * means[i], 1.0e-20)
        var[i] = 1.0 / math.sqrt(var[i])
    return np.array(means), np.array(var)


# ------------------------------------------------------------------ parameter containers (reference state_dict names)

class _GlobalCMVN(nn.Module):
    def __init__(self, mean: Tensor, istd: Tensor):
        super().__init__()
        self.register_buffer("mean", mean)
        self.register_buffer("istd", istd)


class _Subsampling2(nn.Module):
    def __init__(self, idim, odim):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(1, odim, 3, 2), nn.ReLU())
        self.out = nn.Sequential(nn.Linear(odim * ((idim - 1) // 2), odim))


# ``input_layer`` -> subsampling rate, and the (kernel, stride) of every convolution of the stack (subsampling.py:68-280:
# Conv2dSubsampling2 / 4 / 6 / 8; the first is Conv2d(1, C, 3, 2), the others Conv2d(C, C, k, s)).  Lengths, masks, the right
# context and the streaming windows all follow from this table.
CNN_MODULE_NORMS = ("batch_norm", "layer_norm")
INPUT_LAYERS = {"conv2d": 2, "conv2d4": 4, "conv2d6": 6, "conv2d8": 8}
SUBSAMPLING_CONVS = {2: ((3, 2),), 4: ((3, 2), (3, 2)), 6: ((3, 2), (5, 3)), 8: ((3, 2), (3, 2), (3, 2))}


def _convs(rate: int):
    if rate not in SUBSAMPLING_CONVS:
        raise _C.F5EError(f"PPG extractor: subsampling rate {rate} is not built (2, 4, 6 or 8)")
    return SUBSAMPLING_CONVS[rate]


def right_context(rate: int = 2) -> int:
    """``embed.right_context``: sum of (kernel - 1) * frame rate of the layer -> 2 / 6 / 10 / 14."""
    rc, step = 0, 1
    for k, s in _convs(rate):
        rc, step = rc + (k - 1) * step, step * s
    return rc


def subsampled_frames(n: int, rate: int = 2) -> int:
    """Output frames of the stack on ``n`` frames (or bins): n <- (n - k) // s + 1 per convolution, 0 once n < k."""
    for k, s in _convs(rate):
        n = (n - k) // s + 1 if n >= k else 0
    return n


def subsampled_len(length: int, T: int, rate: int = 2) -> int:
    """Valid frames the reference's sliced pad mask leaves to an utterance of ``length`` frames padded to ``T``:
    ``mask[:, :, :-2:2]`` for a (3, 2) convolution, ``[:, :, :-4:3]`` for (5, 3), chained (subsampling.py:119-280)."""
    idx = range(T)
    for k, s in _convs(rate):
        idx = idx[:-(k - 1):s]
    return sum(1 for i in idx if i < int(length))


class _Subsampling(nn.Module):
    """Conv2dSubsampling4 / 6 / 8 by the reference's parameter names: ``conv.{0,2,4}`` (ReLUs between) and ``out.0`` (4x)
    or ``linear`` (6x, 8x)."""

    def __init__(self, idim, odim, rate):
        super().__init__()
        mods = []
        for i, (k, s) in enumerate(_convs(rate)):
            mods += [nn.Conv2d(1 if i == 0 else odim, odim, k, s), nn.ReLU()]
        self.conv = nn.Sequential(*mods)
        width = odim * subsampled_frames(idim, rate)
        if rate == 4:
            self.out = nn.Sequential(nn.Linear(width, odim))
        else:
            self.linear = nn.Linear(width, odim)


class _RelMHA(nn.Module):
    def __init__(self, heads, d):
        super().__init__()
        self.linear_q, self.linear_k, self.linear_v = nn.Linear(d, d), nn.Linear(d, d), nn.Linear(d, d)
        self.linear_out = nn.Linear(d, d)
        self.linear_pos = nn.Linear(d, d, bias=False)
        self.pos_bias_u = nn.Parameter(torch.empty(heads, d // heads))
        self.pos_bias_v = nn.Parameter(torch.empty(heads, d // heads))
        nn.init.xavier_uniform_(self.pos_bias_u)
        nn.init.xavier_uniform_(self.pos_bias_v)


class _FFN(nn.Module):
    def __init__(self, d, units):
        super().__init__()
        self.w_1, self.w_2 = nn.Linear(d, units), nn.Linear(units, d)


class _ConvModule(nn.Module):
    def __init__(self, d, k, norm="batch_norm"):
        super().__init__()
        self.pointwise_conv1 = nn.Conv1d(d, 2 * d, 1)
        self.depthwise_conv = nn.Conv1d(d, d, k, padding=(k - 1) // 2, groups=d)
        self.norm = nn.BatchNorm1d(d) if norm == "batch_norm" else nn.LayerNorm(d)        # convolution.py:63-69
        self.pointwise_conv2 = nn.Conv1d(d, d, 1)


class _ConformerLayer(nn.Module):
    def __init__(self, d, heads, units, k, cnn_norm="batch_norm"):
        super().__init__()
        self.self_attn = _RelMHA(heads, d)
        self.feed_forward, self.feed_forward_macaron = _FFN(d, units), _FFN(d, units)
        self.conv_module = _ConvModule(d, k, cnn_norm)
        for n in ("norm_ff", "norm_mha", "norm_ff_macaron", "norm_conv", "norm_final"):
            setattr(self, n, nn.LayerNorm(d, eps=1e-5))
        self.concat_linear = nn.Linear(2 * d, d)      # a checkpoint key of the reference layer; unused (concat_after False)


class _Encoder(nn.Module):
    def __init__(self, idim, d, heads, units, blocks, k, cmvn, rate=2, cnn_norm="batch_norm"):
        super().__init__()
        self.global_cmvn = cmvn
        self.embed = _Subsampling2(idim, d) if rate == 2 else _Subsampling(idim, d, rate)
        self.after_norm = nn.LayerNorm(d, eps=1e-5)
        self.encoders = nn.ModuleList([_ConformerLayer(d, heads, units, k, cnn_norm) for _ in range(blocks)])


class _CE(nn.Module):
    def __init__(self, d, n):
        super().__init__()
        self.fc = nn.Linear(d, n)


class _CTC(nn.Module):
    """reference ppg/wenet/transformer/ctc.py: only the projection (the loss is a training feature)."""

    def __init__(self, odim, d):
        super().__init__()
        self.ctc_lo = nn.Linear(d, odim)


class _MHA(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.linear_q, self.linear_k, self.linear_v = nn.Linear(d, d), nn.Linear(d, d), nn.Linear(d, d)
        self.linear_out = nn.Linear(d, d)


class _DecoderLayer(nn.Module):
    def __init__(self, d, units):
        super().__init__()
        self.self_attn, self.src_attn = _MHA(d), _MHA(d)
        self.feed_forward = _FFN(d, units)
        self.norm1, self.norm2, self.norm3 = (nn.LayerNorm(d, eps=1e-5) for _ in range(3))
        # checkpoint keys of the reference layer; unused (concat_after False)
        self.concat_linear1, self.concat_linear2 = nn.Linear(2 * d, d), nn.Linear(2 * d, d)


class _TransformerDecoder(nn.Module):
    """reference ppg/wenet/transformer/decoder.py:17-84 (``embed.1`` is the parameter-free positional encoding)."""

    def __init__(self, vocab, d, units, blocks):
        super().__init__()
        self.embed = nn.Sequential(nn.Embedding(vocab, d))
        self.after_norm = nn.LayerNorm(d, eps=1e-5)
        self.output_layer = nn.Linear(d, vocab)
        self.decoders = nn.ModuleList([_DecoderLayer(d, units) for _ in range(blocks)])


class _BiTransformerDecoder(nn.Module):
    def __init__(self, vocab, d, units, blocks, r_blocks):
        super().__init__()
        self.left_decoder = _TransformerDecoder(vocab, d, units, blocks)
        self.right_decoder = _TransformerDecoder(vocab, d, units, r_blocks)


DECODER_DEFAULTS = dict(attention_heads=4, linear_units=2048, num_blocks=6, r_num_blocks=0)
DECODER_FIXED = dict(input_layer="embed", use_output_layer=True, normalize_before=True, concat_after=False)
DECODER_IGNORED = ("dropout_rate", "positional_dropout_rate", "self_attention_dropout_rate", "src_attention_dropout_rate")


def check_decoder_conf(decoder: Optional[str], conf: Optional[dict]) -> dict:
    """The decoder settings that are built (decoder.py:37-52, 205-221): F5EError names every entry that is not."""
    if decoder not in ("transformer", "bitransformer"):
        raise _C.F5EError(f"PPG extractor: unsupported decoder {decoder!r} (transformer and bitransformer are built)")
    conf = dict(conf or {})
    bad = {k: v for k, v in conf.items() if (k in DECODER_FIXED and v != DECODER_FIXED[k]) or
           (k not in DECODER_FIXED and k not in DECODER_DEFAULTS and k not in DECODER_IGNORED)}
    if decoder == "transformer" and conf.get("r_num_blocks", 0):
        bad["r_num_blocks"] = conf["r_num_blocks"]
    if decoder == "bitransformer" and conf.get("r_num_blocks", 0) < 1:
        bad["r_num_blocks"] = conf.get("r_num_blocks", 0)           # init_asr_model asserts r_num_blocks > 0
    if bad:
        raise _C.F5EError(f"PPG extractor: unsupported decoder_conf entries {bad}")
    return {k: int(conf.get(k, v)) for k, v in DECODER_DEFAULTS.items()}


def check_beam(beam_size: int, vocab: int) -> int:
    if not 1 <= int(beam_size) <= min(16, vocab):
        raise _C.F5EError(f"ctc_prefix_beam_search: beam_size must lie in 1..{min(16, vocab)} (got {beam_size})")
    return int(beam_size)


def check_hyps(hyps_lens, U1: int, vocab: int, hyps=None) -> None:
    """Host-side hypothesis lengths (sos included) and ids of ``forward_attention_decoder``: caller bugs raise here."""
    for i, n in enumerate(hyps_lens):
        if not 1 <= int(n) <= U1:
            raise _C.F5EError(f"forward_attention_decoder: hypothesis {i} has length {int(n)}, need 1 <= length <= {U1}")
        if hyps is not None and any(not 0 <= int(v) < vocab for v in hyps[i][:int(n)]):
            raise _C.F5EError(f"forward_attention_decoder: hypothesis {i} holds ids outside [0, {vocab})")


def rescoring_inputs(hyps: List[Tuple[int, ...]], sos: int, eos: int, rows: Optional[int] = None):
    """The decoder inputs and targets of ``attention_rescoring`` (asr_model.py:628-647, 660-670) for one utterance's n-best:
    ys_in = sos + hyp, eos-padded; r_ys_in = sos + reversed hyp, eos-padded; lens = len + 1; the targets whose log-
    probabilities the score sums (hyp then eos at position len, -1 after it; the right-to-left ones reversed).  All i32
    [rows, U + 1] / [rows]; rows past the list (``rows`` > len(hyps)) hold sos alone and no target."""
    rows = len(hyps) if rows is None else rows
    U1 = max([len(h) for h in hyps] + [0]) + 1
    ys, r_ys = np.full((rows, U1), eos, np.int32), np.full((rows, U1), eos, np.int32)
    tg, r_tg = np.full((rows, U1), -1, np.int32), np.full((rows, U1), -1, np.int32)
    lens = np.ones(rows, np.int32)
    ys[:, 0] = r_ys[:, 0] = sos
    for i, h in enumerate(hyps):
        n = len(h)
        ys[i, 1:n + 1], r_ys[i, 1:n + 1] = h, h[::-1]
        tg[i, :n], r_tg[i, :n] = h, h[::-1]
        tg[i, n] = r_tg[i, n] = eos
        lens[i] = n + 1
    return ys, r_ys, lens, tg, r_tg


class CTCAlignment(NamedTuple):
    """``ConformerPPG.ctc_forced_align``: align i32 [B, T'] (class of every encoder frame: blank or a label, -1 past the
    utterance), tok_start / tok_end i32 [B, L] (first / one-past-last frame of every label), score f32 [B] (the path's
    sum of CTC LOGITS, not log-probabilities), frame_lens i32 [B] (valid encoder frames); all on the device."""
    align: Tensor
    tok_start: Tensor
    tok_end: Tensor
    score: Tensor
    frame_lens: Tensor


def check_ctc_lengths(labels, label_lengths, frame_lens, L: int, vocab: Optional[int] = None) -> None:
    """Host-side lengths of a forced alignment are caller bugs when they admit no CTC path (device lengths get -1 / 0 /
    -inf rows from the kernel): 1 <= l <= L and frames >= l + adjacent equal labels.  ``labels``: the ids as nested lists
    when they are known on the host (then the repeats and, with ``vocab``, the id range are checked too), else None."""
    for b, (l, t) in enumerate(zip(label_lengths, frame_lens)):
        l, t = int(l), int(t)
        row = [int(v) for v in labels[b][:max(l, 0)]] if labels is not None else []
        if vocab is not None and any(not 0 <= v < vocab for v in row):
            raise _C.F5EError(f"ctc_forced_align: sequence {b} has no CTC path: label ids must lie in [0, {vocab})")
        rep = sum(1 for i in range(1, len(row)) if row[i] == row[i - 1])
        if not (1 <= l <= L and t >= l + rep):
            raise _C.F5EError(f"ctc_forced_align: sequence {b} has no CTC path: need 1 <= labels ({l}) <= {L} and "
                              f"labels + adjacent repeats ({l} + {rep}) <= encoder frames ({t})")


def check_ctc_loss_lengths(labels, label_lengths, frame_lens, L: int, vocab: Optional[int] = None) -> None:
    """``check_ctc_lengths`` for the CTC likelihood, where an empty transcript and adjacent equal labels are ordinary input:
    0 <= l <= L and frames >= max(1, l + adjacent equal labels) (device lengths get -inf from the kernel instead).
    ``frame_lens=None``: what can be said before the encoder ran (the label lengths and the id range)."""
    for b, l in enumerate(label_lengths):
        l = int(l)
        row = [int(v) for v in labels[b][:max(l, 0)]] if labels is not None else []
        if vocab is not None and any(not 0 <= v < vocab for v in row):
            raise _C.F5EError(f"ctc_loss: sequence {b} has no CTC path: label ids must lie in [0, {vocab})")
        rep = sum(1 for i in range(1, len(row)) if row[i] == row[i - 1])
        if not 0 <= l <= L:
            raise _C.F5EError(f"ctc_loss: sequence {b} has no CTC path: need 0 <= labels ({l}) <= {L}")
        if frame_lens is not None and int(frame_lens[b]) < max(1, l + rep):
            raise _C.F5EError(f"ctc_loss: sequence {b} has no CTC path: need labels + adjacent repeats ({l} + {rep}) <= "
                              f"encoder frames ({int(frame_lens[b])}) and at least one frame")


class ConformerPPG(nn.Module):
    """The part of the reference ``ASRModel`` that ``extract`` touches (asr_model.py:221-244), same state_dict names:
    ``encoder.*``, ``linear.*``, ``ce.fc.*``.  Decoder keys of a checkpoint are not on this path and are skipped by
    ``build_ppg_model`` exactly as the reference's key filter does.  ``ctc=True`` adds the CTC half of the ASR model
    (``ctc.ctc_lo.*``, the reference's key names): ``ctc_greedy_search`` and ``ctc_forced_align``.  The default stays False so
    that ``state_dict()`` is what it was."""

    def __init__(self, input_dim: int = 80, vocab_size: int = 218, output_size: int = 256, attention_heads: int = 4,
                 linear_units: int = 2048, num_blocks: int = 6, cnn_module_kernel: int = 15,
                 global_cmvn: Optional[Tuple[Tensor, Tensor]] = None, causal: bool = False,
                 use_dynamic_chunk: bool = False, static_chunk_size: int = 0, ctc: bool = False,
                 decoder: Optional[str] = None, decoder_conf: Optional[dict] = None, input_layer: str = "conv2d",
                 cnn_module_norm: str = "batch_norm"):
        super().__init__()
        if input_layer not in INPUT_LAYERS or cnn_module_norm not in CNN_MODULE_NORMS:
            raise _C.F5EError(f"PPG extractor: input_layer {input_layer!r} / cnn_module_norm {cnn_module_norm!r} are not built "
                              f"(one of {', '.join(INPUT_LAYERS)}; {', '.join(CNN_MODULE_NORMS)})")
        self.input_layer, self.cnn_module_norm = input_layer, cnn_module_norm
        self.subsampling_rate = INPUT_LAYERS[input_layer]
        self.right_context = right_context(self.subsampling_rate)
        cm = _GlobalCMVN(global_cmvn[0].float(), global_cmvn[1].float()) if global_cmvn is not None else None
        self.encoder = _Encoder(input_dim, output_size, attention_heads, linear_units, num_blocks, cnn_module_kernel, cm,
                                self.subsampling_rate, cnn_module_norm)
        self.linear = nn.Linear(output_size, output_size)
        self.ce = _CE(output_size, vocab_size + 1)
        if ctc:
            self.ctc = _CTC(vocab_size, output_size)
        self.has_ctc, self.vocab_size = bool(ctc), vocab_size
        self.decoder_type, self.decoder_heads = decoder, 0
        if decoder is not None:
            dc = check_decoder_conf(decoder, decoder_conf)
            if output_size % dc["attention_heads"]:
                raise _C.F5EError(f"PPG extractor: decoder_conf attention_heads {dc['attention_heads']} does not divide "
                                  f"output_size {output_size}")
            self.decoder_heads = dc["attention_heads"]
            self.decoder = _TransformerDecoder(vocab_size, output_size, dc["linear_units"], dc["num_blocks"]) \
                if decoder == "transformer" else \
                _BiTransformerDecoder(vocab_size, output_size, dc["linear_units"], dc["num_blocks"], dc["r_num_blocks"])
        self.sos = self.eos = vocab_size - 1                 # asr_model.py: sos = eos = vocab_size - 1
        self.input_dim, self.heads, self.dim = input_dim, attention_heads, output_size
        # causal: the depthwise convolution looks back only (convolution.py:45-52); the chunk settings say whether the
        # model was trained with chunk masks, which the streaming mode requires (encoder.py:327)
        self.causal, self.use_dynamic_chunk, self.static_chunk_size = bool(causal), bool(use_dynamic_chunk), int(static_chunk_size)
        self._engine = None

    @classmethod
    def from_config(cls, configs: dict, ctc: bool = False, decoder: bool = False) -> "ConformerPPG":
        """``init_asr_model`` (asr_model.py:814-859) for the supported encoder family; ``decoder=True`` also builds the
        attention decoder the config names (``decoder`` -- bitransformer when absent, as there -- and ``decoder_conf``)."""
        return cls._from_config(configs, ctc, decoder, ("conv2d",), ("batch_norm",))

    @classmethod
    def from_asr_config(cls, configs: dict, ctc: bool = True, decoder: bool = False) -> "ConformerPPG":
        """``from_config`` for a recogniser rather than the PPG extractor: also the reference's 4x / 6x / 8x fronts
        (``input_layer`` conv2d4 / conv2d6 / conv2d8: Conv2dSubsampling4 / 6 / 8) and ``cnn_module_norm: layer_norm``; the
        CTC head by default.  The DiT needs 20 ms PPGs, so ``from_config`` keeps refusing these."""
        return cls._from_config(configs, ctc, decoder, tuple(INPUT_LAYERS), CNN_MODULE_NORMS)

    @classmethod
    def _from_config(cls, configs: dict, ctc: bool, decoder: bool, input_layers, norms) -> "ConformerPPG":
        enc = dict(configs.get("encoder_conf") or {})
        if configs.get("encoder", "conformer") != "conformer":
            raise _C.F5EError("PPG extractor: only `encoder: conformer` is built for MI355X")
        bad = {k: enc[k] for k, want in dict(pos_enc_layer_type="rel_pos", normalize_before=True,
                                             concat_after=False, macaron_style=True, use_cnn_module=True,
                                             activation_type="swish", use_emb=False,
                                             positionwise_conv_kernel_size=1).items() if k in enc and enc[k] != want}
        bad.update({k: enc[k] for k, ok in (("input_layer", input_layers), ("cnn_module_norm", norms))
                    if k in enc and enc[k] not in ok})
        if bad:
            raise _C.F5EError(f"PPG extractor: unsupported encoder_conf entries {bad}")
        cmvn = None
        if configs.get("cmvn_file") is not None:
            mean, istd = load_cmvn(configs["cmvn_file"], configs["is_json_cmvn"])
            cmvn = (torch.from_numpy(mean).float(), torch.from_numpy(istd).float())
        return cls(configs["input_dim"], configs["output_dim"], enc.get("output_size", 256), enc.get("attention_heads", 4),
                   enc.get("linear_units", 2048), enc.get("num_blocks", 6), enc.get("cnn_module_kernel", 15), cmvn,
                   causal=enc.get("causal", False), use_dynamic_chunk=enc.get("use_dynamic_chunk", False),
                   static_chunk_size=enc.get("static_chunk_size", 0), ctc=ctc,
                   decoder=configs.get("decoder", "bitransformer") if decoder else None,
                   decoder_conf=configs.get("decoder_conf") if decoder else None,
                   input_layer=enc.get("input_layer", "conv2d"), cnn_module_norm=enc.get("cnn_module_norm", "batch_norm"))

    def _apply(self, fn, *a, **kw):
        self._engine = None
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, *a, **kw):
        self._engine = None
        return super().load_state_dict(*a, **kw)

    def engine(self) -> "ConformerEngine":
        dev = next(self.parameters()).device
        if self._engine is None or self._engine.device != dev:
            if dev.type != "cuda":
                raise _C.F5EError(f"PPG model lives on {dev}: move it to the GPU (there is no CPU path)")
            self._engine = ConformerEngine(self.state_dict(), self.heads, dev, self.input_dim, causal=self.causal,
                                           decoder_heads=self.decoder_heads)
        return self._engine

    @torch.no_grad()
    def extract(self, speech: Tensor, speech_lengths: Tensor, stream: bool = False) -> Tuple[Tensor, Tensor]:
        """reference asr_model.py:221-244 -> (ppg [B, T', D], logits [B*T', vocab + 1])."""
        assert speech.shape[0] == speech_lengths.shape[0]
        if stream:
            # forward_chunk_by_chunk(speech, 16, 17): chunk of 16 encoder frames, 17 left chunks; speech_lengths is not
            # used and the batch must be 1 (encoder.py:243), the model chunk-trained (encoder.py:327)
            self._require_stream(speech)
            eng = self.engine()
            return eng.head(eng.forward_chunk_by_chunk(speech, 16, 17))
        return self.engine().forward(speech, speech_lengths)

    def _require_ctc(self, engine: bool = True) -> Optional["ConformerEngine"]:
        """``engine=False``: only the check, for callers that validate more on the host before the engine is built."""
        if not self.has_ctc:
            raise _C.F5EError("PPG extractor: built without the CTC head (ConformerPPG(ctc=True) / build_ppg_model(ctc=True))")
        return self.engine() if engine else None

    def _check_decoding(self, speech: Tensor, decoding_chunk_size: int, simulate_streaming: bool) -> bool:
        """The reference's encoder choice (asr_model.py:281-307) as far as it is built, checked on the host before anything
        touches the device -> whether the chunk-by-chunk encoder runs.  ``decoding_chunk_size`` < 0: full context (the
        default); 0: refused (the reference's four decode methods assert it); > 0 with ``simulate_streaming``: the
        chunk-by-chunk loop, batch 1 and a chunk-trained model; > 0 without: the reference's masked one-pass encoder, which
        is not built."""
        chunk = int(decoding_chunk_size)
        if chunk == 0:
            raise _C.F5EError("PPG extractor: decoding_chunk_size must not be 0 (negative: full context; positive: chunk size)")
        if chunk < 0:
            return False
        if not simulate_streaming:
            raise _C.F5EError("PPG extractor: decoding_chunk_size > 0 without simulate_streaming is the masked one-pass "
                              "encoder, which is out of scope here: pass simulate_streaming=True (chunk by chunk)")
        self._require_stream(speech)
        return True

    def _encoder_out(self, eng: "ConformerEngine", speech: Tensor, speech_lengths: Tensor, decoding_chunk_size: int = -1,
                     num_decoding_left_chunks: int = -1, simulate_streaming: bool = False) -> Tuple[Tensor, Tensor]:
        """``ASRModel._forward_encoder`` -> (encoder output [B, T', D], valid frames i32 [B] on the host): the ONE place where
        the decode methods pick their encoder.  Chunk by chunk, every frame the loop yields is valid (its mask is all ones,
        encoder.py:352-354) and ``speech_lengths`` is not used, as there."""
        if self._check_decoding(speech, decoding_chunk_size, simulate_streaming):
            enc = eng.forward_chunk_by_chunk(speech, int(decoding_chunk_size), int(num_decoding_left_chunks))
            return enc, torch.tensor([enc.shape[1]], dtype=I32)
        return eng._encode(speech, speech_lengths)

    def _ctc_scores(self, speech: Tensor, speech_lengths: Tensor, use_linear: bool,
                    stream: Tuple[int, int, bool] = (-1, -1, False)) -> Tuple[Tensor, Tensor, Tensor]:
        """-> (CTC logits [B, T', V], valid frames i32 [B] on the device, the same on the host).  ``stream``:
        (decoding_chunk_size, num_decoding_left_chunks, simulate_streaming) of ``_encoder_out``."""
        self._check_decoding(speech, stream[0], stream[2])           # caller bugs first: they are the same on any device
        eng = self._require_ctc()
        enc, lens_host = self._encoder_out(eng, speech, speech_lengths, *stream)
        if use_linear:
            enc = eng.head(enc)[0]
        return eng.ctc_logits(enc), lens_host.to(enc.device), lens_host

    @torch.no_grad()
    def ctc_greedy_search(self, speech: Tensor, speech_lengths: Tensor, use_linear: bool = False,
                          pad_id: Optional[int] = None, *, decoding_chunk_size: int = -1,
                          num_decoding_left_chunks: int = -1, simulate_streaming: bool = False) -> Tuple[List[List[int]], Tensor]:
        """reference asr_model.py:416-459 -> (hyps, scores [B, 1]).  ``decoding_chunk_size`` / ``num_decoding_left_chunks`` /
        ``simulate_streaming`` are the reference's (``_check_decoding``): the defaults decode with the full context; a
        positive chunk size with ``simulate_streaming=True`` runs the encoder chunk by chunk (batch 1).
        Argmax, collapse and the frame log-probabilities run on the device (f5e_ctc_greedy) straight from the logits.

        The reference DECODES from the encoder output, although its training forward feeds ``linear(encoder_out)`` to the
        CTC loss (asr_model.py:159-170 against :444-451).  ``use_linear=False`` is what the reference decodes with;
        ``use_linear=True`` is what a checkpoint's CTC head was trained on.

        Frames past an utterance take ``pad_id`` = eos before the collapse, as the reference's masked_fill does: a shorter
        utterance of a batch ends in a trailing eos.  ``scores`` equals ``.values`` of the reference's ``topk_prob.max(1)``
        (the best frame's top-1 log-probability, padded frames included)."""
        assert speech.shape[0] == speech_lengths.shape[0]
        logits, frame_lens, _ = self._ctc_scores(speech, speech_lengths, use_linear,
                                                 (decoding_chunk_size, num_decoding_left_chunks, simulate_streaming))
        hyp, hyp_len, logp = ops.ctc_greedy(logits, frame_lens, blank=0, pad_id=self.eos if pad_id is None else pad_id,
                                            want_logp=True)
        hyp_h, len_h = hyp.cpu(), hyp_len.cpu().tolist()
        return [hyp_h[b, :n].tolist() for b, n in enumerate(len_h)], logp.max(1, keepdim=True).values

    @torch.no_grad()
    def ctc_forced_align(self, speech: Tensor, speech_lengths: Tensor, labels, label_lengths=None,
                         use_linear: bool = False) -> CTCAlignment:
        """Forced alignment of ``labels`` (ids, [B, L] tensor or a list of lists) to the encoder frames
        (wenet/utils/ctc_util.py::forced_align per utterance, here one launch for the batch, fed with the LOGITS: per-frame
        constants cancel in the search).  Lengths that start on the host are validated there (F5EError); device lengths
        that admit no path give -1 / 0 / -inf rows."""
        assert speech.shape[0] == speech_lengths.shape[0]
        logits, frame_lens, lens_host = self._ctc_scores(speech, speech_lengths, use_linear)
        dev = logits.device
        if not torch.is_tensor(labels):
            rows = [list(r) for r in labels]
            label_lengths = [len(r) for r in rows] if label_lengths is None else label_lengths
            L = max(1, max(len(r) for r in rows))
            labels = torch.tensor([r + [0] * (L - len(r)) for r in rows], dtype=I32)
        if label_lengths is None:
            label_lengths = [labels.shape[1]] * labels.shape[0]
        if labels.ndim != 2 or labels.shape[0] != logits.shape[0] or len(label_lengths) != logits.shape[0]:
            raise _C.F5EError(f"ctc_forced_align: labels [B, L] and label_lengths [B] for a batch of {logits.shape[0]}")
        if not (torch.is_tensor(label_lengths) and label_lengths.is_cuda):
            # every length that starts on the host is validated there, whether or not the ids are (the encoder's frame counts
            # are host values); ids on the host add the repeat count and the id range
            check_ctc_lengths(None if labels.is_cuda else labels.tolist(),
                              label_lengths.tolist() if torch.is_tensor(label_lengths) else label_lengths,
                              lens_host.tolist(), labels.shape[1], self.vocab_size)
        l_len = torch.as_tensor(label_lengths, dtype=I32).to(dev)
        out = ops.ctc_align(logits, labels.to(dev, I32).contiguous(), frame_lens, l_len, blank=0)
        return CTCAlignment(*out, frame_lens)

    @staticmethod
    def _ctc_text(text, text_lengths, B: int, name: str):
        """ids as a [B, L] tensor or a list of lists -> (labels i32 [B, L] tensor, lengths: list or tensor [B]); shapes checked."""
        if not torch.is_tensor(text):
            rows = [list(r) for r in text]
            if text_lengths is None:
                text_lengths = [len(r) for r in rows]
            elif len(text_lengths) == len(rows) and not (torch.is_tensor(text_lengths) and text_lengths.is_cuda):
                for b, (n, r) in enumerate(zip(text_lengths, rows)):      # the padding below is the blank id, not a label
                    if int(n) > len(r):
                        raise _C.F5EError(f"{name}: text_lengths[{b}] = {int(n)} exceeds the {len(r)} ids of row {b}")
            L = max([len(r) for r in rows] + [0])
            text = torch.tensor([r + [0] * (L - len(r)) for r in rows], dtype=I32).reshape(len(rows), L)
        if text_lengths is None and text.ndim == 2:
            text_lengths = [text.shape[1]] * text.shape[0]
        if text.ndim != 2 or text.shape[0] != B or len(text_lengths) != B:
            raise _C.F5EError(f"{name}: text [B, L] and text_lengths [B] for a batch of {B}")
        return text, text_lengths

    @torch.no_grad()
    def ctc_loss(self, speech: Tensor, speech_lengths: Tensor, text, text_lengths=None, use_linear: bool = True,
                 reduce: bool = True) -> Tensor:
        """The eval-mode value of the reference's CTC branch (asr_model.py:146-151, 170-172 with wenet/transformer/ctc.py:32-50):
        encoder, ``linear`` (the training forward applies it before the CTC head, hence ``use_linear=True`` here, unlike the
        decode methods), ``ctc_lo``, then the CTC loss, summed over all paths on the device (f5e_ctc_loss) straight from the
        logits.  ``reduce=True``: ``sum_b(-logp[b]) / B``, a 0-d device tensor -- ``CTC.forward``'s "sum, then batch-size
        average"; ``reduce=False``: ``-logp`` f32 [B] (+inf for an utterance without a CTC path).

        ``text``: ids, a [B, L] tensor or a list of lists; entries past ``text_lengths`` are ignored, whatever they hold (the
        reference pads with -1).  An empty transcript and adjacent equal ids are legal.  Lengths that start on the host are
        validated there (F5EError) before anything touches the device; device lengths that admit no path give +inf.

        No gradient is offered: this is a score, not a training loss."""
        assert speech.shape[0] == speech_lengths.shape[0]
        self._require_ctc(engine=False)
        B = speech.shape[0]
        text, text_lengths = self._ctc_text(text, text_lengths, B, "ctc_loss")
        host = None
        if not (torch.is_tensor(text_lengths) and text_lengths.is_cuda):
            # every length that starts on the host is validated there, with the ids when they are host values too: first
            # what does not need the encoder's frame counts, then (below) the path condition against them
            host = (None if text.is_cuda else text.tolist(),
                    text_lengths.tolist() if torch.is_tensor(text_lengths) else [int(v) for v in text_lengths])
            check_ctc_loss_lengths(*host, None, text.shape[1], self.vocab_size)
        logits, frame_lens, lens_host = self._ctc_scores(speech, speech_lengths, use_linear)
        if host is not None:
            check_ctc_loss_lengths(*host, lens_host.tolist(), text.shape[1], self.vocab_size)
        dev = logits.device
        l_len = torch.as_tensor(text_lengths, dtype=I32).to(dev)
        labels = text.to(dev, I32).contiguous()
        nll = -ops.ctc_loss(logits, labels, frame_lens, l_len, blank=0)
        return nll.sum() / B if reduce else nll

    def _require_decoder(self, reverse_weight: float = 0.0) -> "ConformerEngine":
        if self.decoder_type is None:
            raise _C.F5EError("PPG extractor: built without the attention decoder (ConformerPPG(decoder=...) / "
                              "build_ppg_model(decoder=True))")
        if reverse_weight > 0.0 and self.decoder_type != "bitransformer":
            raise _C.F5EError("PPG extractor: reverse_weight > 0 needs the bitransformer decoder (its right-to-left half)")
        return self.engine()

    def _nbest(self, logits: Tensor, frame_lens: Tensor, beam_size: int):
        """f5e_ctc_beam on CTC logits -> per utterance the list of (ids tuple, score), best first (one D2H of the lists)."""
        K = check_beam(beam_size, self.vocab_size)
        hyp, n, sc = ops.ctc_beam_search(logits, frame_lens, K, blank=0)
        hyp_h, n_h, sc_h = hyp.cpu().numpy(), n.cpu().tolist(), sc.cpu().tolist()
        return [[(tuple(int(v) for v in hyp_h[b, k, :n_h[b][k]]), float(sc_h[b][k])) for k in range(K) if n_h[b][k] >= 0]
                for b in range(len(n_h))]

    @torch.no_grad()
    def ctc_prefix_beam_search(self, speech: Tensor, speech_lengths: Tensor, beam_size: int, use_linear: bool = False, *,
                               decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1,
                               simulate_streaming: bool = False) -> List[List[Tuple[Tuple[int, ...], float]]]:
        """reference asr_model.py:461-578 (encoder choice as in ``ctc_greedy_search``) for a batch of ANY size -> per utterance the n-best list of
        (ids, score = logaddexp(pb, pnb)), best first; at batch 1, ``[0]`` is the reference's ``_ctc_prefix_beam_search``
        list.  The search runs on the device (f5e_ctc_beam) straight from the logits, frames past an utterance skipped.
        ``use_linear`` as in ``ctc_greedy_search``."""
        assert speech.shape[0] == speech_lengths.shape[0]
        check_beam(beam_size, self.vocab_size)
        logits, frame_lens, _ = self._ctc_scores(speech, speech_lengths, use_linear,
                                                 (decoding_chunk_size, num_decoding_left_chunks, simulate_streaming))
        return self._nbest(logits, frame_lens, beam_size)

    @torch.no_grad()
    def attention_rescoring(self, speech: Tensor, speech_lengths: Tensor, beam_size: int, ctc_weight: float = 0.0,
                            reverse_weight: float = 0.0, use_linear: bool = False, *, decoding_chunk_size: int = -1,
                            num_decoding_left_chunks: int = -1,
                            simulate_streaming: bool = False) -> List[Tuple[Tuple[int, ...], float]]:
        """reference asr_model.py:580-677 (encoder choice as in ``ctc_greedy_search``) for a batch of any size -> per utterance (ids, score) of the n-best entry the
        attention decoder likes best:  sum_j logp[j][w_j] + logp[len][eos], with reverse_weight > 0 mixed as
        score (1 - rw) + r_score rw with the right-to-left decoder's sum (taken at len - j - 1), plus ctc_weight x the CTC
        score; the first maximum wins.  The decoder runs ONCE per batch on the device: the memory's key / value projections
        once per utterance (the reference repeats the encoder output beam_size times), every hypothesis' queries in one
        launch; f5e_token_logp leaves one float per target, summed here in double precision as the reference does."""
        assert speech.shape[0] == speech_lengths.shape[0]
        self._check_decoding(speech, decoding_chunk_size, simulate_streaming)
        eng = self._require_decoder(reverse_weight)
        self._require_ctc()
        K = check_beam(beam_size, self.vocab_size)
        enc, lens_host = self._encoder_out(eng, speech, speech_lengths, decoding_chunk_size, num_decoding_left_chunks,
                                           simulate_streaming)
        frame_lens = lens_host.to(enc.device)
        nbest = self._nbest(eng.ctc_logits(eng.head(enc)[0] if use_linear else enc), frame_lens, K)
        return self._rescore(eng, enc, lens_host, nbest, K, ctc_weight, reverse_weight)

    def _rescore(self, eng: "ConformerEngine", enc: Tensor, lens_host: Tensor, nbest, K: int, ctc_weight: float,
                 reverse_weight: float) -> List[Tuple[Tuple[int, ...], float]]:
        """The decoder pass of ``attention_rescoring`` over ``nbest`` (per utterance the list of (ids, CTC score)) and the
        encoder output it came from."""
        frame_lens = lens_host.to(enc.device)
        B, dev = len(nbest), enc.device
        U1 = max(len(h) for hyps in nbest for h, _ in hyps) + 1 if any(nbest) else 1
        packs = [rescoring_inputs([h for h, _ in hyps], self.sos, self.eos, rows=K) for hyps in nbest]
        pad = lambda a: np.pad(a, ((0, 0), (0, U1 - a.shape[1])), constant_values=self.eos)          # noqa: E731
        pad_t = lambda a: np.pad(a, ((0, 0), (0, U1 - a.shape[1])), constant_values=-1)               # noqa: E731
        ys = torch.from_numpy(np.concatenate([pad(p[0]) for p in packs])).to(dev)
        r_ys = torch.from_numpy(np.concatenate([pad(p[1]) for p in packs])).to(dev)
        lens = torch.from_numpy(np.concatenate([p[2] for p in packs])).to(dev)
        tg = torch.from_numpy(np.concatenate([pad_t(p[3]) for p in packs])).to(dev)
        r_tg = torch.from_numpy(np.concatenate([pad_t(p[4]) for p in packs])).to(dev)
        ragged = bool(int(lens_host.min()) < enc.shape[1])
        mem_len = frame_lens if ragged else None
        lp = ops.token_logp(eng.decode("left", enc, mem_len, ys, lens, K), tg.view(-1)).view(B, K, U1).cpu().double()
        total = lp.sum(-1)
        if reverse_weight > 0.0:
            r_lp = ops.token_logp(eng.decode("right", enc, mem_len, r_ys, lens, K), r_tg.view(-1)).view(B, K, U1)
            total = total * (1 - reverse_weight) + r_lp.cpu().double().sum(-1) * reverse_weight
        out = []
        for b, hyps in enumerate(nbest):
            best, best_i = -float("inf"), 0
            for i, (_, ctc_score) in enumerate(hyps):
                score = float(total[b, i]) + ctc_score * ctc_weight
                if score > best:
                    best, best_i = score, i
            out.append((hyps[best_i][0] if hyps else tuple(), best))
        return out

    @torch.no_grad()
    def recognize(self, speech: Tensor, speech_lengths: Tensor, beam_size: int = 10, *, reorder_cache: bool = False,
                  nbest: bool = False, sync_every: int = 4, decoding_chunk_size: int = -1,
                  num_decoding_left_chunks: int = -1, simulate_streaming: bool = False) -> Tuple[Tensor, Tensor]:
        """reference asr_model.py:309-414 (encoder choice as in ``ctc_greedy_search``): beam search over the attention decoder (the left one of a
        bitransformer, decoder.py:294) -> (best_hyps i64 [B, L], best_scores f32 [B]) on the device: ``hyps[:, 1:]`` of each
        utterance's max-score row, eos-padded, L as the reference's early stop leaves it.  ``nbest=True`` returns the whole
        beam instead, (hyps [B, beam, L], scores [B, beam]) in beam order (best first).

        The search keeps per-layer key / value caches on the device and never moves a cache row (f5e_attn_decode_f32 follows
        an ancestry table instead).  The reference does not reorder its per-layer cache when the second prune reshuffles the
        beam, so with two or more decoder blocks the layers above the first attend to what their ROW computed earlier, not
        to what the hypothesis' ancestor did; the default reproduces that.  ``reorder_cache=True`` is the corrected search,
        every layer following the ancestry, equal to recomputing the decoder on the whole prefix at every step.
        ``sync_every``: the host asks the device whether every row has finished once per that many steps; the result does
        not depend on it."""
        assert speech.shape[0] == speech_lengths.shape[0]
        # caller bugs first: they are the same on any device
        K = check_beam(beam_size, self.vocab_size) if self.decoder_type is not None else 0
        if int(sync_every) < 1:
            raise _C.F5EError(f"recognize: sync_every must be >= 1 (got {sync_every})")
        self._check_decoding(speech, decoding_chunk_size, simulate_streaming)
        eng = self._require_decoder()
        enc, lens_host = self._encoder_out(eng, speech, speech_lengths, decoding_chunk_size, num_decoding_left_chunks,
                                           simulate_streaming)
        mem_len = lens_host.to(enc.device) if int(lens_host.min()) < enc.shape[1] else None
        hyps, scores = eng.attention_beam_search("left", enc, mem_len, K, self.sos, self.eos, bool(reorder_cache),
                                                 int(sync_every))
        hyps = hyps.long()
        if nbest:
            return hyps, scores
        best_scores, best = scores.max(dim=-1)
        return hyps[torch.arange(hyps.shape[0], device=hyps.device), best], best_scores

    @torch.no_grad()
    def forward_attention_decoder(self, hyps: Tensor, hyps_lens: Tensor, encoder_out: Tensor,
                                  reverse_weight: float = 0) -> Tuple[Tensor, Tensor]:
        """reference asr_model.py:763-811: ``hyps`` [N, U + 1] ids with the leading sos, eos-padded, ``hyps_lens`` [N] counting
        the sos, ``encoder_out`` [1, T', D] -> (log_softmax of the decoder output [N, U + 1, V], the same of the
        right-to-left decoder fed the reversed hypotheses, or tensor(0.0) when reverse_weight is 0)."""
        eng = self._require_decoder(reverse_weight)
        if encoder_out.ndim != 3 or encoder_out.shape[0] != 1 or hyps.ndim != 2 or hyps_lens.shape[0] != hyps.shape[0]:
            raise _C.F5EError("forward_attention_decoder: hyps [N, U + 1], hyps_lens [N] and encoder_out [1, T', D]")
        N, U1 = hyps.shape
        h, n = hyps.detach().cpu().numpy().astype(np.int64), hyps_lens.detach().cpu().numpy().astype(np.int64)
        check_hyps(n, U1, self.vocab_size, h)
        dev = eng.device
        enc = encoder_out.to(dev, F32).contiguous()
        ys = torch.from_numpy(h.astype(np.int32)).to(dev)
        lens = torch.from_numpy(n.astype(np.int32)).to(dev)
        V = self.vocab_size
        out = ops.log_softmax_rows(eng.decode("left", enc, None, ys, lens, N)).view(N, U1, V)
        if not reverse_weight > 0:
            return out, torch.tensor(0.0)
        r = np.full((N, U1), self.eos, np.int32)
        r[:, 0] = self.sos
        for i in range(N):
            r[i, 1:n[i]] = h[i, 1:n[i]][::-1]
        r_out = ops.log_softmax_rows(eng.decode("right", enc, None, torch.from_numpy(r).to(dev), lens, N)).view(N, U1, V)
        return out, r_out

    def _require_stream(self, xs: Tensor) -> None:
        if not (self.static_chunk_size > 0 or self.use_dynamic_chunk):
            raise _C.F5EError("PPG extractor: streaming needs a chunk-trained model (static_chunk_size > 0 or "
                              "use_dynamic_chunk in encoder_conf)")
        if xs.shape[0] != 1:
            raise _C.F5EError(f"PPG extractor: streaming runs one utterance at a time (batch {xs.shape[0]})")

    def streaming_recognizer(self, beam_size: int = 10, decoding_chunk_size: int = 16, num_decoding_left_chunks: int = -1,
                             max_seconds: float = 60.0, use_linear: bool = False):
        """A ``StreamingRecognizer`` (ppg/streaming_asr.py) on this model: audio in as it arrives, the n-best list of the
        resumable CTC prefix beam search out after every block, ``finish()`` for the final result or its attention
        rescoring.  Building it allocates the search state for ``max_seconds`` of audio."""
        from .streaming_asr import StreamingRecognizer
        return StreamingRecognizer(self, beam_size, decoding_chunk_size, num_decoding_left_chunks, max_seconds, use_linear)

    @torch.no_grad()
    def forward_encoder_chunk(self, xs: Tensor, offset: int, required_cache_size: int,
                              subsampling_cache: Optional[Tensor] = None,
                              elayers_output_cache: Optional[List[Tensor]] = None,
                              conformer_cnn_cache: Optional[List[Tensor]] = None):
        """reference asr_model.py:705-737 -> BaseEncoder.forward_chunk (encoder.py:210-291): one window of features
        ``xs`` [1, n, idim] whose first output frame is encoder frame ``offset`` -> (encoder output of the new frames
        [1, n', D], subsampling cache, per-layer output caches, per-layer convolution caches)."""
        self._require_stream(xs)
        return self.engine().forward_chunk(xs, offset, required_cache_size, subsampling_cache, elayers_output_cache,
                                           conformer_cnn_cache)


def _ln(x: Tensor, out: Tensor, pair: Tuple[Tensor, Tensor]) -> Tensor:
    """nn.LayerNorm(eps=1e-5) with ``pair`` = (weight, bias); out may be x."""
    return ops.layernorm(x, out, gamma=pair[0], beta=pair[1], eps=1e-5)


def mask_rows(x: Tensor, keep: Tensor, out: Tensor, eye: Optional[Tensor] = None) -> Tensor:
    """out = x [rows, d] with the rows whose ``keep`` [rows] is 0 zeroed.  row_scale acts on a GEMM's output side, hence the
    identity GEMM; ``eye``: the [d, d] identity when the caller keeps one."""
    eye = torch.eye(x.shape[1], device=x.device) if eye is None else eye
    return ops.gemm_f32(x, eye, None, out=out, row_scale=keep)


def beam_loop(S: SimpleNamespace, step, sync_every: int) -> Tuple[Tensor, Tensor]:
    """The loop control of ``ConformerEngine.attention_beam_search`` around ``step(S)`` (one decode step that ends in
    f5e_beam_step and advances ``S.p``): up to ``S.umax`` steps, ``S.done_at`` read every ``sync_every`` steps -> (hyps i32
    [B, beam, L] without the sos, scores f32 [B, beam]).  L = max_b done_at[b] + 1, the width the reference's per-step check
    leaves, whatever the number of steps run beyond it (they append eos to eos-filled columns); ``S.umax`` when a row never
    finishes."""
    done = None
    while S.p < S.umax:
        step(S)
        if S.p % sync_every == 0 or S.p == S.umax:
            done = S.done_at.cpu()
            if bool((done >= 0).all()):
                break
    width = int(done.max()) + 1 if bool((done >= 0).all()) else S.umax
    hyps = S.hyp[S.p & 1][:, 1:width + 1].reshape(S.B, S.beam, width)
    return hyps, S.score.view(S.B, S.beam)


class ConformerEngine:
    """Repacked fp32 weights + the launch sequence of ``BaseEncoder.forward`` (wenet/transformer/encoder.py:141-209)."""

    def __init__(self, sd: Dict[str, Tensor], heads: int, device, idim: int, causal: bool = False, decoder_heads: int = 0):
        ops.require_device()
        self.device = dv = torch.device(device)
        f = lambda k: sd[k].detach().to(dv, F32).contiguous()   # noqa: E731
        self.heads, self.causal = heads, bool(causal)
        cw, cb = f("encoder.embed.conv.0.weight"), f("encoder.embed.conv.0.bias")        # [C, 1, 3, 3]
        C = cw.shape[0]
        # the front by its parameter names (subsampling.py): conv.2 / conv.4 are the C -> C convolutions of the 4x / 6x / 8x
        # stacks (6x: a 5 x 5 kernel), whose Linear is ``out.0`` (2x, 4x) or ``linear`` (6x, 8x)
        c2 = sd.get("encoder.embed.conv.2.weight")
        self.rate = 2 if c2 is None else (8 if "encoder.embed.conv.4.weight" in sd else (6 if c2.shape[-1] == 5 else 4))
        self.right_context = right_context(self.rate)
        self.context = self.right_context + 1
        lin = "encoder.embed.out.0." if self.rate in (2, 4) else "encoder.embed.linear."
        if lin + "weight" not in sd:
            raise _C.F5EError(f"PPG extractor: a {self.rate}x subsampling front needs {lin}weight in the state_dict")
        ow = f(lin + "weight")                                                           # [D, C * F']
        self.dim = D = ow.shape[0]
        F2, Fo = (idim - 1) // 2, subsampled_frames(idim, self.rate)                     # bins after conv.0 / after the stack
        self.idim = idim
        if Fo < 1 or ow.shape[1] != C * Fo:
            raise _C.F5EError(f"PPG extractor: embed.out expects {ow.shape[1] // C} subsampled bins, input_dim {idim} gives {Fo}")
        # Conv2d(1, C, 3, stride 2) over [T, idim] as ONE dense GEMM per frame triple: row n = c * F2 + f' of a Toeplitz
        # matrix holds w[c, 0, i, j] at column i * idim + 2 f' + j.  Global CMVN ((x - mean) * istd, per feature) is
        # linear in x, so it folds into these weights and a per-row bias (weights-only transform, done once).
        # Rates 4 / 6 / 8: row n = f' * C + c instead, so that the GEMM emits the channels-last [T1, F2, C] activation that
        # f5e_conv2d_sub_f32 reads; its weights go to [C][kt][kf][C], and the Linear's columns from (c, f) to (f, c) order.
        toe = torch.zeros(C * F2, 3 * idim, device=dv)
        n = torch.arange(C * F2, device=dv)
        c_idx, f_idx = (n // F2, n % F2) if self.rate == 2 else (n % C, n // C)
        self.sub_convs = [(ops.pack_conv2d_sub_weight(f(f"encoder.embed.conv.{2 * i}.weight")),
                           f(f"encoder.embed.conv.{2 * i}.bias"), s) for i, (_, s) in enumerate(_convs(self.rate)) if i]
        if self.rate != 2:
            if C % 16:
                raise _C.F5EError(f"PPG extractor: the {self.rate}x front's convolutions need a multiple of 16 channels (got {C})")
            ow = ow.view(D, C, Fo).permute(0, 2, 1).reshape(D, Fo * C).contiguous()
        for i in range(3):
            for j in range(3):
                toe[n, i * idim + 2 * f_idx + j] = cw[c_idx, 0, i, j]
        bias = cb[c_idx].clone()
        if "encoder.global_cmvn.mean" in sd:
            mean, istd = f("encoder.global_cmvn.mean"), f("encoder.global_cmvn.istd")
            s3, m3 = istd.repeat(3), mean.repeat(3)
            bias = bias - (toe * (s3 * m3)[None, :]).sum(1)
            toe = toe * s3[None, :]
        self.sub_w, self.sub_b = toe.contiguous(), bias.contiguous()
        self.sub_k, self.sub_c = 3 * idim, C
        self.out_w, self.out_b = ow, f(lin + "bias")
        self.xscale = math.sqrt(D)
        dk = D // heads
        self.layers = []
        i = 0
        while f"encoder.encoders.{i}.norm_mha.weight" in sd:
            p = f"encoder.encoders.{i}."
            wq, bq = f(p + "self_attn.linear_q.weight"), f(p + "self_attn.linear_q.bias")
            u, v = f(p + "self_attn.pos_bias_u").reshape(-1), f(p + "self_attn.pos_bias_v").reshape(-1)
            cm = p + "conv_module."
            dw, db = f(cm + "depthwise_conv.weight")[:, 0, :], f(cm + "depthwise_conv.bias")       # [D, k]
            # cnn_module_norm: eval-mode BatchNorm1d folds into the depthwise weights; layer_norm (no running statistics in
            # the state_dict) stays a LayerNorm over channels behind the depthwise convolution (convolution.py:122-128)
            bn = cm + "norm.running_var" in sd
            s = f(cm + "norm.weight") / torch.sqrt(f(cm + "norm.running_var") + 1e-5) if bn else torch.ones_like(db)
            if not self.causal and dw.shape[1] % 2 == 0:
                raise _C.F5EError(f"PPG extractor: cnn_module_kernel {dw.shape[1]} must be odd unless causal")
            pb1 = f(cm + "pointwise_conv1.bias")
            self.layers.append(dict(
                ln={n_: (f(p + n_ + ".weight"), f(p + n_ + ".bias"))
                    for n_ in ("norm_ff", "norm_mha", "norm_ff_macaron", "norm_conv", "norm_final")},
                ffm=tuple(f(p + "feed_forward_macaron." + n_) for n_ in ("w_1.weight", "w_1.bias", "w_2.weight", "w_2.bias")),
                ff=tuple(f(p + "feed_forward." + n_) for n_ in ("w_1.weight", "w_1.bias", "w_2.weight", "w_2.bias")),
                # (q + pos_bias_u | q + pos_bias_v) = x Wq^T + (bq + u | bq + v): one GEMM with the weight stacked twice
                wq2=torch.cat((wq, wq), 0).contiguous(), bq2=torch.cat((bq + u, bq + v), 0).contiguous(),
                wk=f(p + "self_attn.linear_k.weight"), bk=f(p + "self_attn.linear_k.bias"),
                wv=f(p + "self_attn.linear_v.weight"), bv=f(p + "self_attn.linear_v.bias"),
                wo=f(p + "self_attn.linear_out.weight"), bo=f(p + "self_attn.linear_out.bias"),
                wp=f(p + "self_attn.linear_pos.weight"),
                pw1=f(cm + "pointwise_conv1.weight")[:, :, 0].contiguous(), pb1=f(cm + "pointwise_conv1.bias"),
                dw=(dw * s[:, None]).t().contiguous(),
                db=((db - f(cm + "norm.running_mean")) * s + f(cm + "norm.bias")).contiguous() if bn else db,
                cn=None if bn else (f(cm + "norm.weight"), f(cm + "norm.bias")),
                # causal: what the depthwise conv sees left of an utterance is GLU(pointwise_conv1(0)) (the reference pads
                # zeros BEFORE pointwise_conv1, convolution.py:103-119)
                fill=(pb1[:D] * torch.sigmoid(pb1[D:])).contiguous(),
                pw2=f(cm + "pointwise_conv2.weight")[:, :, 0].contiguous(), pb2=f(cm + "pointwise_conv2.bias")))
            i += 1
        self.after = (f("encoder.after_norm.weight"), f("encoder.after_norm.bias"))
        self.lin_w, self.lin_b = f("linear.weight"), f("linear.bias")
        self.ce_w, self.ce_b = f("ce.fc.weight"), f("ce.fc.bias")
        self.ctc_w = self.ctc_b = None
        if "ctc.ctc_lo.weight" in sd:
            self.ctc_w, self.ctc_b = f("ctc.ctc_lo.weight"), f("ctc.ctc_lo.bias")
        self.half = torch.full((max(D, 1),), 0.5, device=dv)
        self.eye = torch.eye(D, device=dv)                  # mask_rows of a ragged batch
        self.dk = dk
        # attention decoder(s): decoder.* (transformer) or decoder.left_decoder.* / right_decoder.* (bitransformer)
        self.dec, self.dec_heads = {}, int(decoder_heads)
        for name, pre in (("left", "decoder."), ("left", "decoder.left_decoder."), ("right", "decoder.right_decoder.")):
            if pre + "embed.0.weight" in sd:
                self.dec[name] = self._decoder_weights(f, sd, pre)
        self._pe: Dict[int, Tensor] = {}

    def _decoder_weights(self, f, sd, pre: str) -> dict:
        """One TransformerDecoder's weights, repacked once: the embedding pre-scaled by sqrt(D) (embedding.py:62), q | k | v
        of the self-attention and k | v of the source attention stacked into one GEMM each (``xfmr_f32.fold_layer``)."""
        wb = lambda n: (sd[n + ".weight"], sd[n + ".bias"])   # noqa: E731
        layers, i = [], 0
        while f"{pre}decoders.{i}.norm1.weight" in sd:
            p = f"{pre}decoders.{i}."
            sa, xa = p + "self_attn.linear_", p + "src_attn.linear_"
            layers.append(fold_layer(self.device, wb(p + "norm1"), wb(sa + "q"), wb(sa + "k"), wb(sa + "v"), wb(sa + "out"),
                                     wb(p + "norm3"), wb(p + "feed_forward.w_1"), wb(p + "feed_forward.w_2"), ln_x=wb(p + "norm2"),
                                     xq=wb(xa + "q"), xk=wb(xa + "k"), xv=wb(xa + "v"), xout=wb(xa + "out")))
            i += 1
        return dict(embed=(f(pre + "embed.0.weight") * math.sqrt(self.dim)).contiguous(), layers=layers,
                    after=(f(pre + "after_norm.weight"), f(pre + "after_norm.bias")),
                    out=(f(pre + "output_layer.weight"), f(pre + "output_layer.bias")))

    def decode(self, which: str, memory: Tensor, mem_len: Optional[Tensor], ys_in: Tensor, ys_len: Tensor, n_hyp: int) -> Tensor:
        """TransformerDecoder.forward (decoder.py:86-135, pre-norm) for ``n_hyp`` hypotheses per utterance: memory f32
        [B, T', D], mem_len i32 [B] on the device or None (every frame valid), ys_in i32 [B * n_hyp, U1] (sos + ids, padded),
        ys_len i32 [B * n_hyp] -> logits f32 [B * n_hyp * U1, V].  Per layer: the self-attention is one causal f5e_mha_f32
        over B * n_hyp items of U1 rows (keys < ys_len); the source attention projects the memory's keys and values ONCE per
        utterance and runs one f5e_mha_f32 over B items of n_hyp * U1 queries against T' keys."""
        if which not in self.dec:
            raise _C.F5EError(f"PPG extractor: the state_dict has no {which} attention decoder")
        W, dv, D, H = self.dec[which], self.device, self.dim, self.dec_heads
        B, T2, _ = memory.shape
        NB, U1 = ys_in.shape
        if NB != B * n_hyp or ys_len.shape != (NB,) or H < 1 or D % H:
            raise _C.F5EError(f"decode: ys_in [{B} * {n_hyp}, U1], ys_len [{B * n_hyp}], heads {H} dividing {D}")
        R, scale = NB * U1, 1.0 / math.sqrt(D // H)
        mem = memory.reshape(B * T2, D)
        x = torch.empty(NB, U1, D, device=dv)
        ops.text_gather(ys_in.contiguous(), W["embed"], self.pos_table(U1).contiguous(), None, x)
        x = x.view(R, D)
        hn, ctx, q = torch.empty(R, D, device=dv), torch.empty(R, D, device=dv), torch.empty(R, D, device=dv)
        qkv, kv = torch.empty(R, 3 * D, device=dv), torch.empty(B * T2, 2 * D, device=dv)
        units = W["layers"][0].ff[0].shape[0] if W["layers"] else D
        bufs = (hn, qkv, ctx, q, torch.empty(R, units, device=dv))

        def self_attn(_L, _hn, qkv, ctx):
            ops.mha_f32(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], H, scale, B=NB, kv_len=ys_len, causal=True, out=ctx)

        def src_attn(L, q, ctx):                # the memory's keys and values, projected per layer into one buffer
            ops.gemm_f32(mem, *L.xkv, out=kv)
            ops.mha_f32(q, kv[:, :D], kv[:, D:], H, scale, B=B, kv_len=mem_len, causal=False, out=ctx)

        for L in W["layers"]:
            layer(x, x, L, bufs, pre_norm=True, act=ops.ACT_RELU, eps=1e-5, self_attn=self_attn, cross_attn=src_attn)
        _ln(x, hn, W["after"])
        logits = torch.empty(R, W["out"][0].shape[0], device=dv)
        ops.gemm_f32(hn, *W["out"], out=logits)
        return logits

    def decode_state(self, which: str, memory: Tensor, mem_len: Optional[Tensor], beam: int, sos: int, eos: int,
                     umax: Optional[int] = None) -> SimpleNamespace:
        """Everything ``decode_step`` reads and writes for a search over ``memory`` f32 [B, T', D] with ``beam`` rows per
        utterance: the per-layer key / value caches [layers, R, Umax, D] (Umax = the reference's loop bound, the padded T'),
        the memory's k | v projection of every layer (done ONCE, here), the two hypothesis / ancestry table pairs
        [R, Umax + 1] (hypotheses eos-filled behind column 0 = sos) and the reference's start scores 0, -inf, ..."""
        if which not in self.dec:
            raise _C.F5EError(f"PPG extractor: the state_dict has no {which} attention decoder")
        W, dv, D, H = self.dec[which], self.device, self.dim, self.dec_heads
        B, T2, _ = memory.shape
        if H < 1 or D % H:
            raise _C.F5EError(f"decode_state: heads {H} must divide {D}")
        umax = T2 if umax is None else int(umax)
        if not 1 <= umax <= 4096:
            raise _C.F5EError(f"decode_state: the search runs at most 4096 steps (got {umax})")
        R, nl = B * beam, len(W["layers"])
        units = W["layers"][0].ff[0].shape[0] if nl else D
        V = W["out"][0].shape[0]
        S = SimpleNamespace(W=W, B=B, beam=beam, R=R, umax=umax, eos=eos, mem_len=mem_len, p=0,
                            scale=1.0 / math.sqrt(D // H),
                            kc=torch.empty(nl, R, umax, D, device=dv), vc=torch.empty(nl, R, umax, D, device=dv), kv=[],
                            hyp=[torch.full((R, umax + 1), eos, dtype=I32, device=dv) for _ in range(2)],
                            anc=[torch.zeros(R, umax + 1, dtype=I32, device=dv) for _ in range(2)],
                            score=torch.tensor([0.0] + [-float("inf")] * (beam - 1)).repeat(B).to(dv),
                            last=torch.full((R,), sos, dtype=I32, device=dv),
                            alive=torch.full((B,), beam, dtype=I32, device=dv), done_at=torch.full((B,), -1, dtype=I32, device=dv),
                            x=torch.empty(R, 1, D, device=dv), hn=torch.empty(R, D, device=dv), ctx=torch.empty(R, D, device=dv),
                            q=torch.empty(R, D, device=dv), qkv=torch.empty(R, 3 * D, device=dv),
                            mid=torch.empty(R, units, device=dv), logits=torch.empty(R, V, device=dv))
        for h in S.hyp:
            h[:, 0] = sos
        mem = memory.reshape(B * T2, D)
        for L in W["layers"]:
            S.kv.append(ops.gemm_f32(mem, *L.xkv, out=torch.empty(B * T2, 2 * D, device=dv)))
        # the attention launches of ``layer``, built once; ``decode_step`` sets in ``at`` what a step (p, anc, every = reorder_cache)
        # and a layer (i) change
        S.at = at = SimpleNamespace(i=0, p=0, anc=None, every=False)
        kc, vc, kv, scale = S.kc, S.vc, S.kv, S.scale

        def self_attn(_L, _hn, qkv, ctx):
            ops.attn_decode_f32(qkv, kc[at.i], vc[at.i], at.p, H, scale, anc=at.anc if (at.i == 0 or at.every) else None, out=ctx)

        def src_attn(_L, q, ctx):
            ops.mha_f32(q, kv[at.i][:, :D], kv[at.i][:, D:], H, scale, B=B, kv_len=mem_len, causal=False, out=ctx)
        S.layer = ((S.hn, S.qkv, S.ctx, S.q, S.mid), self_attn, src_attn)
        return S

    def decode_step(self, S: SimpleNamespace, reorder_cache: bool = False, prune: bool = True) -> Tensor:
        """TransformerDecoder.forward_one_step (decoder.py:137-181) for position ``S.p`` of all R rows plus, with ``prune``,
        the beam update of asr_model.py:374-403 -> the step's raw logits [R, V] (a buffer of ``S``).  11 launches per layer
        (``xfmr_f32.layer`` with the two attention launches of ``decode_state``) + 4:
        embedding of the last tokens at position p; per layer LayerNorm, q | k | v, f5e_attn_decode_f32 on the layer's
        cache, out-projection, LayerNorm, q, f5e_mha_f32 of B items x beam queries against the memory, out-projection,
        LayerNorm, two feed-forward GEMMs; after_norm, output layer, f5e_beam_step.  The ancestry table goes to layer 0 alone
        (the reference: its caches of the layers above stay with the row index) or, ``reorder_cache``, to every layer."""
        W, D, H, p = S.W, self.dim, self.dec_heads, S.p
        if p >= S.umax:
            raise _C.F5EError(f"decode_step: the caches hold {S.umax} positions")
        cur, nxt = p & 1, (p & 1) ^ 1
        ops.text_gather(S.last.view(S.R, 1), W["embed"], self.pos_table(1, offset=p), None, S.x)
        x = S.x.view(S.R, D)
        at, (bufs, self_attn, src_attn) = S.at, S.layer
        at.p, at.anc, at.every = p, S.anc[cur], reorder_cache
        for i, L in enumerate(W["layers"]):
            at.i = i
            layer(x, x, L, bufs, pre_norm=True, act=ops.ACT_RELU, eps=1e-5, self_attn=self_attn, cross_attn=src_attn)
        _ln(x, S.hn, W["after"])
        ops.gemm_f32(S.hn, *W["out"], out=S.logits)
        if prune:
            ops.beam_step(S.logits, S.score, S.hyp[cur], S.anc[cur], S.hyp[nxt], S.anc[nxt], S.last, S.alive, S.done_at, p,
                          S.beam, S.eos)
            S.p = p + 1
        return S.logits

    def attention_beam_search(self, which: str, memory: Tensor, mem_len: Optional[Tensor], beam: int, sos: int, eos: int,
                              reorder_cache: bool = False, sync_every: int = 4) -> Tuple[Tensor, Tensor]:
        """The loop of ASRModel.recognize (asr_model.py:364-403) -> (hyps i32 [B, beam, L] without the sos, eos-padded, in
        beam order; scores f32 [B, beam]).  The reference asks the device every step whether all rows have finished; here
        the host reads ``done_at`` every ``sync_every`` steps.  A step run after an utterance is complete appends eos at score
        + 0 and keeps the row order (what the reference does at B > 1 for utterances that finish early), so the result is
        the same for any ``sync_every``: L = max_b done_at[b] + 1, or the loop bound when some row never finishes."""
        S = self.decode_state(which, memory, mem_len, beam, sos, eos)
        return beam_loop(S, lambda st: self.decode_step(st, reorder_cache), sync_every)

    def pos_table(self, t: int, offset: int = 0) -> Tensor:
        """PositionalEncoding.pe[:, offset:offset + t] (embedding.py:34-46, 65-82), a constant table built in fp32 like the
        reference.  One table is cached; threads may race to replace it, so the entry is built into a local, published
        as a whole new dict and returned from the local: a caller never indexes a dict another thread has swapped."""
        n = offset + t
        for have, pe in self._pe.items():       # a snapshot of the dict object; rows do not depend on the table's length
            if have >= n:
                return pe[offset:n]
        d = self.dim
        rows = n if offset == 0 else (n + 511) // 512 * 512       # incremental callers come back with growing offsets
        pe = torch.zeros(rows, d)
        pos = torch.arange(0, rows, dtype=F32).unsqueeze(1)
        div = torch.exp(torch.arange(0, d, 2, dtype=F32) * -(math.log(10000.0) / d))
        pe[:, 0::2], pe[:, 1::2] = torch.sin(pos * div), torch.cos(pos * div)
        pe = pe.to(self.device).contiguous()
        self._pe = {rows: pe}
        return pe[offset:n]

    def forward(self, feats: Tensor, lens: Tensor) -> Tuple[Tensor, Tensor]:
        return self.head(self._encode(feats, lens)[0])

    def ctc_logits(self, enc: Tensor) -> Tensor:
        """``ctc.ctc_lo`` of an encoder output [B, T', D] -> logits f32 [B, T', vocab] (ctc.py: log_softmax without the
        softmax, which the decoding kernels do not need)."""
        if self.ctc_w is None:
            raise _C.F5EError("PPG extractor: the state_dict has no ctc.ctc_lo.* tensors")
        B, T2, D = enc.shape
        logits = torch.empty(B * T2, self.ctc_w.shape[0], device=self.device)
        ops.gemm_f32(enc.reshape(B * T2, D), self.ctc_w, self.ctc_b, out=logits)
        return logits.view(B, T2, -1)

    def encode(self, feats: Tensor, lens: Tensor) -> Tuple[Tensor, Tensor]:
        """BaseEncoder.forward: features -> (encoder output after ``after_norm`` [B, T', D], valid frames i32 [B] on the
        device = the reference's ``encoder_mask.squeeze(1).sum(1)``)."""
        enc, len2 = self._encode(feats, lens)
        return enc, len2.to(self.device)

    def _encode(self, feats: Tensor, lens: Tensor) -> Tuple[Tensor, Tensor]:
        """``encode`` with the frame counts left on the host, where they are computed (``forward`` does not need them)."""
        dv, D = self.device, self.dim
        B, T, _ = feats.shape
        xs = self._subsample(feats.to(dv, F32).contiguous())
        T2 = xs.shape[0] // B
        lens_h = lens.detach().to("cpu", torch.long)
        len2 = torch.tensor([subsampled_len(int(n), T, self.rate) for n in lens_h], dtype=I32)  # mask[:, :, :-2:2] ...
        pos = self.pos_table(T2)
        # masks whenever ANY item is shorter than the padded length (reference BaseEncoder always builds them from xs_lens,
        # ppg/wenet/transformer/encoder.py: also for a single padded utterance); all-full batches need none
        kv_len = keep = None
        if int(len2.min()) < T2:
            kv_len = len2.to(dv)
            keep = (torch.arange(T2)[None, :] < len2[:, None].long()).to(F32).to(dv).reshape(-1).contiguous()      # mask_pad
        S = self._scratch(B, B * T2, pos, masked=keep is not None)
        attn = partial(self._full_attn, B=B, T=T2, kv_len=kv_len, ws=self._full_attn_scratch(T2))
        conv = partial(self._conv_one_pass, chunk=0)
        for L in self.layers:
            self._layer(L, xs, S, attn=attn, conv=conv, keep=keep)
        return _ln(xs, S.hn, self.after).view(B, T2, D), len2

    # ---- the conformer layer (encoder_layer.py:199-268), written once.  Full context (BaseEncoder.forward) and the chunk-by-
    # chunk modes (BaseEncoder.forward_chunk / forward_chunk_by_chunk, encoder.py:210-355) differ in three steps, which the
    # caller picks: the context product, what the depthwise convolution sees left of the rows, and the pad mask.
    #
    # The reference's streaming loop feeds overlapping windows of 2 chunk + 1 feature frames at stride 2 chunk through
    # forward_chunk, which keeps the last chunk * left_chunks rows of every layer's output as keys / values for the next window
    # and convolves each chunk on its own.  Everything in a layer is row-wise except (a) the attention, where a query of chunk
    # c = t // chunk therefore sees keys [max(0, (c - left) chunk), (c + 1) chunk), the position term indexed by the key's
    # absolute position, and (b) the depthwise convolution: causal with kernel - 1 frames of carried left context, or, not
    # causal, zero-padded inside each chunk.  forward_chunk_by_chunk is that as ONE pass (one attention launch per layer
    # whatever the number of chunks); forward_chunk runs the same kernels on [cached rows ; new rows].

    def _subsample(self, x: Tensor) -> Tensor:
        """Conv2dSubsampling2 / 4 / 6 / 8 (+ folded CMVN) + xscale of [B, T, idim] -> [B * T', D]: patches of 3 frames at
        stride 2 -> ReLU(Toeplitz GEMM), one strided GEMM per item -> (rates 4 / 6 / 8: the C -> C convolutions as implicit
        GEMMs on the channels-last activation, f5e_conv2d_sub_f32) -> Linear -> x * sqrt(d) (RelPositionalEncoding).
        Padded frames of a ragged batch are convolved as they are, as the reference does: a valid frame next to the
        padding sees whatever the padding holds."""
        B, T, idim = x.shape
        if idim != self.idim:
            raise _C.F5EError(f"PPG extractor: features have {idim} bins, the model expects {self.idim}")
        if T < self.context:
            raise _C.F5EError(f"PPG extractor: needs at least {self.context} feature frames")
        dv, T2 = self.device, (T - 3) // 2 + 1
        col = torch.empty(B, T, self.sub_k, device=dv)
        ops.im2col(x, col, 3, 0)
        patches = col.view(B * T, self.sub_k)
        h = torch.empty(B * T2, self.sub_w.shape[0], device=dv)
        for b in range(B):
            ops.gemm_f32(patches[b * T:(b + 1) * T:2], self.sub_w, self.sub_b, out=h[b * T2:(b + 1) * T2], M=T2,
                         act=ops.ACT_RELU)
        C = self.sub_c
        for w, bias, stride in self.sub_convs:
            h = ops.conv2d_sub(h.view(B, T2, -1, C), w, bias, stride)
            T2 = h.shape[1]
        h = h.view(B * T2, -1)
        xs = torch.empty(B * T2, self.dim, device=dv)
        ops.gemm_f32(h, self.out_w, self.out_b, out=xs)
        ops.axpby(xs, None, xs, self.xscale, 0.0, 0.0)
        return xs

    def _scratch(self, B: int, R: int, pos: Tensor, q0: int = 0, left: int = 0, masked: bool = False) -> SimpleNamespace:
        """The buffers of ``_layer`` for x of R rows (B sequences) whose rows from q0 on are computed: allocated and cut
        into the views the layer uses ONCE per call.  pos: the position table of the call; left: rows of carried context in
        front of the computed rows in the conv module; masked: a pad mask will be applied."""
        D, n = self.dim, R - q0
        c = n + left
        units = self.layers[0]["ffm"][0].shape[0] if self.layers else D
        e = lambda r, w: torch.empty(r, w, device=self.device)   # noqa: E731
        hn, mid, ctx, gl, dwo = e(R, D), e(R, units), e(R, D), e(c, D), e(c, D)
        return SimpleNamespace(B=B, R=R, q0=q0, pos=pos, hn=hn, hq=hn[q0:], hm=e(n, D) if masked else None, mid=mid,
                               midq=mid[:n], qu=e(R, 2 * D), kb=e(R, D), vb=e(R, D), pb=e(pos.shape[0], D), ctx=ctx,
                               ctxq=ctx[q0:], pw=e(c, 2 * D), gl=gl, gl3=gl.view(B, c // B, D),
                               dwo3=dwo.view(B, c // B, D), dwoq=dwo[left:])

    def _layer(self, L: dict, x: Tensor, S: SimpleNamespace, *, attn, conv,
               keep: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
        """One conformer layer over x [S.R, D] (updated in place): rows < S.q0 are cached rows that only serve as keys /
        values (encoder_layer.py:220-231), rows >= S.q0 are computed.
          attn(L, qu, k, pb, hn, ctx)         the context product into ctx's rows >= q0: ``_full_attn`` or ``_band_attn``
          conv(L, h) -> (src, dw, new_cache)  the rows pointwise_conv1 -> GLU -> depthwise conv run on (h behind S's ``left``
                                              rows of context), f5e_dwconv_stream's mode, and the conv cache to hand back:
                                              ``_conv_one_pass`` or ``_conv_cached``
          keep                                f32 [R] 0 / 1 or None: the pad mask of a ragged batch
        -> (the computed rows' output, a view of x; new conv cache)."""
        ln, hn, hq, mid = L["ln"], S.hn, S.hq, S.mid
        # macaron feed-forward: x += 0.5 * W2 swish(W1 LN(x))
        _ln(x, hn, ln["norm_ff_macaron"])
        ops.gemm_f32(hn, L["ffm"][0], L["ffm"][1], out=mid, act=ops.ACT_SILU)
        ops.gemm_f32(mid, L["ffm"][2], L["ffm"][3], out=x, ch_scale=self.half, addend=x)
        # relative-position self-attention (attention.py:172-222)
        _ln(x, hn, ln["norm_mha"])
        ops.gemm_f32(hn, L["wq2"], L["bq2"], out=S.qu)
        ops.gemm_f32(hn, L["wk"], L["bk"], out=S.kb)
        ops.gemm_f32(S.pos, L["wp"], None, out=S.pb)
        attn(L, S.qu, S.kb, S.pb, hn, S.ctx)
        xq = x[S.q0:] if S.q0 else x
        ops.gemm_f32(S.ctxq, L["wo"], L["bo"], out=xq, addend=xq)
        # convolution module (convolution.py:81-134): mask, pointwise -> GLU -> depthwise (+BN) -> swish -> pointwise, mask
        _ln(xq, hq, ln["norm_conv"])
        # the reference zeroes padded frames BEFORE pointwise_conv1 (whose bias then makes them non-zero again for the
        # depthwise conv's neighbours): mask LN(x) first
        src, dw, new_cache = conv(L, hq if keep is None else mask_rows(hq, keep, S.hm, self.eye))
        ops.gemm_f32(src, L["pw1"], L["pb1"], out=S.pw)
        ops.glu(S.pw, S.gl)
        ops.dwconv_stream(S.gl3, L["dw"], L["db"], S.dwo3, **dw)
        if L["cn"] is not None:
            _ln(S.dwoq, S.dwoq, L["cn"])
        ops.gemm_f32(S.dwoq, L["pw2"], L["pb2"], out=hq, a_act=ops.ACT_SILU, row_scale=keep)
        ops.axpby(xq, hq, xq, 1.0, 1.0)
        # feed-forward + final norm
        _ln(xq, hq, ln["norm_ff"])
        ops.gemm_f32(hq, L["ff"][0], L["ff"][1], out=S.midq, act=ops.ACT_SILU)
        ops.gemm_f32(S.midq, L["ff"][2], L["ff"][3], out=xq, ch_scale=self.half, addend=xq)
        _ln(xq, xq, ln["norm_final"])
        return xq, new_cache

    def _full_attn_scratch(self, T: int) -> Tuple[Tensor, Tensor, Tensor]:
        """(V^T [D, Tp] with zeroed pad columns, scores [T, Tp], probabilities [T, Tp]) of ``_full_attn``, Tp = T up to 4."""
        Tp = (T + 3) // 4 * 4
        return (torch.zeros(self.dim, Tp, device=self.device), torch.empty(T, Tp, device=self.device),
                torch.empty(T, Tp, device=self.device))

    def _full_attn(self, L: dict, qu: Tensor, k: Tensor, pb: Tensor, vsrc: Tensor, ctx: Tensor, *, B: int, T: int,
                   kv_len: Optional[Tensor], ws: Tuple[Tensor, Tensor, Tensor]) -> Tensor:
        """Full-context attention of B sequences of T rows, one sequence and head at a time on the fp32 GEMM: qu [B * T, 2 D]
        (q + u | q + v), k [B * T, D], pb [T, D] projected positions, vsrc [B * T, D] the rows ``L["wv"]`` projects to the
        values, kv_len i32 [B] on the device or None -> ctx [B * T, D]."""
        D, dk, scale = self.dim, self.dk, 1.0 / math.sqrt(self.dk)
        vt, sc, pr = ws
        for b in range(B):
            r0, r1 = b * T, (b + 1) * T
            # V^T [D, T] = Wv . LN(x)^T (bias added after P.V: softmax rows sum to one)
            ops.gemm_f32(L["wv"], vsrc[r0:r1], None, out=vt[:, :T])
            for hd in range(self.heads):
                c0, c1 = hd * dk, (hd + 1) * dk
                ops.gemm_f32(qu[r0:r1, c0:c1], k[r0:r1, c0:c1], None, out=sc[:, :T])               # (q + u) k^T
                ops.gemm_f32(qu[r0:r1, D + c0:D + c1], pb[:, c0:c1], None, out=sc[:, :T], addend=sc[:, :T])  # + (q + v) p^T
                ops.softmax_rows(sc, pr, T, scale, kv_len=kv_len[b:b + 1] if kv_len is not None else None, rows_per_seq=T)
                ops.gemm_f32(pr, vt[c0:c1], L["bv"][c0:c1], out=ctx[r0:r1, c0:c1], K=vt.shape[1])
        return ctx

    def _band_attn(self, L: dict, qu: Tensor, k: Tensor, pb: Tensor, vsrc: Tensor, ctx: Tensor, *, vb: Tensor, q0: int,
                   chunk: int, left: int) -> Tensor:
        """Streaming attention of one sequence in ONE launch (f5e_relpos_attn): the queries from row q0 on against the keys
        of the band (chunk, left), chunk 0: every key.  vb [rows, D]: scratch for the projected values."""
        ops.gemm_f32(vsrc, L["wv"], L["bv"], out=vb)
        return ops.relpos_attn(qu, k, pb, vb, ctx, self.heads, 1.0 / math.sqrt(self.dk), chunk=chunk, left_chunks=left,
                               q_begin=q0)

    def _conv_one_pass(self, L: dict, h: Tensor, *, chunk: int):
        """The conv of whole utterances.  Causal: left of them it sees GLU(pointwise_conv1(0)), ``L["fill"]``.  Otherwise
        symmetric, every chunk of ``chunk`` rows on its own with zero padding (0: the whole sequence)."""
        if self.causal and L["dw"].shape[0] > 1:
            return h, dict(causal=True, fill=L["fill"]), None
        return h, dict(causal=False, chunk=chunk), None

    def _conv_cached(self, L: dict, h: Tensor, *, left: int, cnn_cache: Optional[Tensor]):
        """forward_chunk's conv.  Causal (left = K - 1 > 0): behind the carried ``cnn_cache`` [1, D, left] (None: zeros),
        handing back the last ``left`` rows; otherwise on the rows alone, handing back the reference's dummy
        (convolution.py:113-116)."""
        if not left:
            return h, dict(causal=False, chunk=0), torch.zeros(1, device=self.device)
        prev = cnn_cache[0].t().to(self.device, F32) if cnn_cache is not None else torch.zeros(left, self.dim, device=self.device)
        src = torch.cat((prev, h), 0)
        return src, dict(causal=True), src[-left:].t().unsqueeze(0).contiguous()

    @staticmethod
    def stream_frames(num_frames: int, chunk: int, rate: int = 2, context: int = 3) -> int:
        """Encoder frames the reference's loop yields (encoder.py:328-343): windows of rate (chunk - 1) + context feature
        frames at stride rate chunk, starting while ``cur < num_frames - context + 1``; each window of n frames gives what
        the subsampling stack leaves of n.  The defaults are the 2x front (window 2 (chunk - 1) + 3, (n - 3) // 2 + 1)."""
        window, total = rate * (chunk - 1) + context, 0
        for cur in range(0, num_frames - context + 1, rate * chunk):
            total += subsampled_frames(min(cur + window, num_frames) - cur, rate)
        return total

    def forward_chunk_by_chunk(self, feats: Tensor, decoding_chunk_size: int, num_decoding_left_chunks: int = -1) -> Tensor:
        """BaseEncoder.forward_chunk_by_chunk (encoder.py:293-355) in one pass -> encoder output [1, T', D]."""
        if decoding_chunk_size <= 0:
            raise _C.F5EError("PPG extractor: decoding_chunk_size must be positive")
        if feats.shape[0] != 1:
            raise _C.F5EError(f"PPG extractor: streaming runs one utterance at a time (batch {feats.shape[0]})")
        xs = self._subsample(feats.to(self.device, F32).contiguous())
        n = self.stream_frames(feats.shape[1], decoding_chunk_size, self.rate, self.context)
        if n > xs.shape[0]:
            raise _C.F5EError(f"PPG extractor: the streaming loop yields {n} frames, the subsampling {xs.shape[0]}")
        xs = xs[:n]
        pos = self.pos_table(n)
        S = self._scratch(1, n, pos)
        attn = partial(self._band_attn, vb=S.vb, q0=0, chunk=decoding_chunk_size, left=num_decoding_left_chunks)
        conv = partial(self._conv_one_pass, chunk=decoding_chunk_size)
        for L in self.layers:
            self._layer(L, xs, S, attn=attn, conv=conv)
        return _ln(xs, S.hn, self.after).unsqueeze(0)

    def forward_chunk(self, xs: Tensor, offset: int, required_cache_size: int, subsampling_cache: Optional[Tensor] = None,
                      elayers_output_cache: Optional[List[Tensor]] = None,
                      conformer_cnn_cache: Optional[List[Tensor]] = None):
        """BaseEncoder.forward_chunk (encoder.py:210-291): caches in the reference's shapes (subsampling / layer outputs
        [1, rows, D], convolution [1, D, K - 1] or the dummy [1])."""
        if xs.shape[0] != 1:
            raise _C.F5EError(f"PPG extractor: streaming runs one utterance at a time (batch {xs.shape[0]})")
        dv, D = self.device, self.dim
        new = self._subsample(xs.to(dv, F32).contiguous())
        cs = 0 if subsampling_cache is None else subsampling_cache.shape[1]
        if offset < cs:
            raise _C.F5EError(f"PPG extractor: offset {offset} is smaller than the cache ({cs} frames)")
        x = torch.cat((subsampling_cache[0].to(dv, F32), new), 0) if cs else new
        R = x.shape[0]
        pos = self.pos_table(R, offset - cs)
        start = 0 if required_cache_size < 0 else (R if required_cache_size == 0 else max(R - required_cache_size, 0))
        r_sub, r_att, r_cnn = x[start:].unsqueeze(0).clone(), [], []
        K = self.layers[0]["dw"].shape[0] if self.layers else 1
        left = K - 1 if self.causal else 0                  # rows of the carried conv cache
        S = None
        for i, L in enumerate(self.layers):
            cache = None if elayers_output_cache is None else elayers_output_cache[i][0].to(dv, F32)
            q0 = 0 if cache is None else cache.shape[0]
            if not q0 < R:
                raise _C.F5EError("PPG extractor: the layer output cache must be shorter than cache + chunk")
            if S is None or (S.R, S.q0) != (x.shape[0], q0):      # once per call: the caches of a call have one length
                S = self._scratch(1, x.shape[0], pos, q0, left)
            xq, cnn = self._layer(L, x, S, attn=partial(self._band_attn, vb=S.vb, q0=q0, chunk=0, left=-1),
                                  conv=partial(self._conv_cached, left=left,
                                               cnn_cache=None if conformer_cnn_cache is None else conformer_cnn_cache[i]))
            x = torch.cat((cache, xq), 0) if q0 else xq
            r_att.append(x[start:].unsqueeze(0).clone())
            r_cnn.append(cnn)
        return _ln(x, torch.empty(R, D, device=dv), self.after)[cs:].unsqueeze(0), r_sub, r_att, r_cnn

    def head(self, enc: Tensor) -> Tuple[Tensor, Tensor]:
        """``linear`` (the PPG) and ``ce.fc`` logits of an encoder output [B, T', D] (asr_model.py:241-244)."""
        B, T2, D = enc.shape
        ppg = torch.empty(B * T2, D, device=self.device)
        ops.gemm_f32(enc.reshape(B * T2, D), self.lin_w, self.lin_b, out=ppg)
        logits = torch.empty(B * T2, self.ce_w.shape[0], device=self.device)
        ops.gemm_f32(ppg, self.ce_w, self.ce_b, out=logits)
        return ppg.view(B, T2, D), logits


# ------------------------------------------------------------------ features + wrapper (reference ppg/ppg_model.py)

def _kaldi_mel_banks(num_bins: int, padded: int, sr: float, low: float = 20.0, high: float = 0.0) -> Tensor:
    """torchaudio.compliance.kaldi.get_mel_banks (vtln_warp 1) -> [padded / 2 + 1, num_bins] (Nyquist row zero)."""
    nyq = 0.5 * sr
    high = high + nyq if high <= 0.0 else high
    mel_low, mel_high = 1127.0 * math.log(1.0 + low / 700.0), 1127.0 * math.log(1.0 + high / 700.0)
    delta = (mel_high - mel_low) / (num_bins + 1)
    b = torch.arange(num_bins).unsqueeze(1)
    left, center, right = mel_low + b * delta, mel_low + (b + 1.0) * delta, mel_low + (b + 2.0) * delta
    m = (1127.0 * torch.log(1.0 + (sr / padded) * torch.arange(padded // 2) / 700.0)).unsqueeze(0)
    bins = torch.max(torch.zeros(1), torch.min((m - left) / (center - left), (right - m) / (right - center)))
    return torch.nn.functional.pad(bins, (0, 1)).t().contiguous()


class kaldiFbank(nn.Module):
    """reference ppg/wenet/dataset/feats.py:49-83 (kaldi.fbank per utterance: 80 bins, 25 ms / 10 ms, dither 0)."""

    def __init__(self, sample_rate=16000, n_fft=512, win_length=400, hop_length=160, n_mels=80, spec_mask_time=[5, 10],
                 spec_mask_freq=[5, 10]):
        super().__init__()
        self.f_length, self.f_shift = int(win_length / sample_rate * 1000), int(hop_length / sample_rate * 1000)
        self.sample_rate, self.n_fft, self.n_mels = sample_rate, n_fft, n_mels
        self.win, self.shift = int(sample_rate * self.f_length * 0.001), int(sample_rate * self.f_shift * 0.001)
        if (1 << (self.win - 1).bit_length()) != 512:
            raise _C.F5EError("kaldiFbank: the HIP kernel is built for a 512-point padded window (25 ms at 16 kHz)")
        k = torch.arange(256, dtype=torch.float64)
        self.register_buffer("window", torch.hann_window(self.win, periodic=False).pow(0.85), persistent=False)
        self.register_buffer("twiddle", torch.stack((torch.cos(2 * math.pi * k / 512), -torch.sin(2 * math.pi * k / 512)),
                                                    -1).float(), persistent=False)
        self.register_buffer("fb", _kaldi_mel_banks(n_mels, 512, float(sample_rate)), persistent=False)

    @torch.no_grad()
    def forward(self, x: Tensor, is_spec_aug=[]):
        if len(is_spec_aug) != 0:
            raise _C.F5EError("kaldiFbank: spec augmentation is a training feature (out of scope)")
        if self.window.device.type != "cuda":
            self.to(x.device if x.is_cuda else "cuda")
        wav = x.to(self.window.device, F32).contiguous()
        T = 1 + (wav.shape[1] - self.win) // self.shift
        out = torch.empty(wav.shape[0], T, self.n_mels, device=wav.device)
        ops.kaldi_fbank(wav, self.window, self.twiddle, self.fb, out, self.win, self.shift)
        return out, torch.tensor([T])


def build_ppg_model(ppg_model_path, ppg_config, device="cpu", ctc: bool = False, decoder: bool = False):
    """reference ppg/ppg_model.py:11-29: yaml -> model (cmvn path fallback next to the checkpoint) -> checkpoint keys that
    exist in the model are loaded, the rest (the attention decoder unless ``decoder=True``; the CTC head unless ``ctc=True``)
    ignored."""
    return _build_model(ppg_model_path, ppg_config, device, ctc, decoder, asr=False)


def check_input_layer(input_layer: str, checkpoint_keys) -> None:
    """Upstream wenet names its 4x front ``conv2d``; here (as in the reference) ``conv2d`` is the 2x front and 4x is
    ``conv2d4``.  A config that says ``conv2d`` over a checkpoint that holds a second convolution would load the wrong
    Linear shape: refuse it by name instead."""
    if input_layer == "conv2d" and "encoder.embed.conv.2.weight" in checkpoint_keys:
        raise _C.F5EError("ASR model: the config says `input_layer: conv2d` (the 2x front here) but the checkpoint holds "
                          "encoder.embed.conv.2.weight, a second subsampling convolution: this is an upstream wenet model "
                          "whose `conv2d` means 4x -- use `input_layer: conv2d4`")


def build_asr_model(model_path, config, device="cpu", ctc: bool = True, decoder: bool = False):
    """``build_ppg_model`` for a recogniser (``ConformerPPG.from_asr_config``): the 2x / 4x / 6x / 8x fronts, either
    ``cnn_module_norm``, the CTC head by default.  A 2x batch-norm model gives the model ``build_ppg_model(ctc=True)``
    gives."""
    return _build_model(model_path, config, device, ctc, decoder, asr=True)


def _build_model(ppg_model_path, ppg_config, device, ctc: bool, decoder: bool, asr: bool):
    import yaml
    with open(ppg_config, "r") as fin:
        ppg_configs = yaml.safe_load(fin)
    if ppg_configs.get("cmvn_file") is not None and not os.path.exists(ppg_configs["cmvn_file"]):
        old = ppg_configs["cmvn_file"]
        ppg_configs["cmvn_file"] = os.path.join(os.path.dirname(ppg_model_path), "global_cmvn")
        print(f"{old} not exist, use {ppg_configs['cmvn_file']}")
    model = (ConformerPPG.from_asr_config if asr else ConformerPPG.from_config)(ppg_configs, ctc=ctc, decoder=decoder)
    checkpoint = torch.load(ppg_model_path, map_location="cpu", weights_only=True)
    if asr:
        check_input_layer(model.input_layer, checkpoint.keys())
    model_dict = model.state_dict()
    model_dict.update({k: v for k, v in checkpoint.items() if k in model_dict})
    model.load_state_dict(model_dict)
    return model.to(device).eval()


def make_pad_mask(lengths: Tensor, max_len: int = 0) -> Tensor:
    """reference ppg/ppg_model.py:31-56."""
    max_len = max_len if max_len > 0 else int(lengths.max().item())
    return torch.arange(0, max_len, dtype=torch.int64, device=lengths.device)[None, :] >= lengths.unsqueeze(-1)


class PPGModelWapper(object):
    """reference ppg/ppg_model.py:58-168 (name as spelled there)."""

    def __init__(self, ppg_model_path, ppg_config, device, output_type="ppg", map_mix_ratio=1.0, ppg_frame_length=20,
                 mel_f_shift=10, global_phn_center_path=None, para_softmax_path=None, stream: bool = False):
        print(f"loading ppg model from {ppg_model_path}")
        print(f"output_type : {output_type}")
        self.ppg_model = build_ppg_model(ppg_model_path, ppg_config, device)
        self.device, self.output_type, self.map_mix_ratio = device, output_type, map_mix_ratio
        self.ppg_frame_length, self.mel_f_shift = ppg_frame_length, mel_f_shift
        self.stream = bool(stream)       # extract(stream=True): chunk-by-chunk PPGs for models trained on streaming PPGs
        self.featCal = kaldiFbank().eval()
        if self.output_type == "map":
            import pickle
            self.global_phn_center = torch.from_numpy(np.load(global_phn_center_path)).to(device).to(F32)
            with open(para_softmax_path, "rb") as f:
                para = pickle.load(f)
            self.para_softmax = {"w": torch.from_numpy(para["w"]).to(device).float().contiguous(),
                                 "b": torch.from_numpy(para["b"]).to(device).float().contiguous()}

    @staticmethod
    def norm_ppg(ppg, length):
        raise NotImplementedError("norm_ppg is dead code in the reference (commented out at ppg_model.py:121,128)")

    def ppg_to_target(self, ppg, true_len):
        """reference :112-131: optional map through the phone posteriors' centres, then zero the padded frames."""
        B, T, D = ppg.shape
        keep = (~make_pad_mask(true_len.to(ppg.device), T)).to(F32).reshape(-1).contiguous()
        if self.output_type == "map":
            w, bb, cen = self.para_softmax["w"], self.para_softmax["b"], self.global_phn_center
            logit = torch.empty(B * T, w.shape[0], device=ppg.device)
            ops.gemm_f32(ppg.reshape(B * T, D), w, bb, out=logit)
            Lp = (w.shape[0] + 3) // 4 * 4
            soft = torch.zeros(B * T, Lp, device=ppg.device)
            ops.softmax_rows(logit, soft, w.shape[0], 1.0)
            cen_t = torch.zeros(cen.shape[1], Lp, device=ppg.device)
            cen_t[:, :cen.shape[0]] = cen.t()
            mapped = torch.empty(B * T, cen.shape[1], device=ppg.device)
            ops.gemm_f32(soft, cen_t, None, out=mapped)
            if self.map_mix_ratio != 1.0:
                ops.axpby(ppg.reshape(B * T, D).contiguous(), mapped, mapped, 1 - self.map_mix_ratio, self.map_mix_ratio)
            src = mapped
        elif self.output_type == "ppg":
            src = ppg.reshape(B * T, D).contiguous()
        else:
            raise _C.F5EError(f"unknown output_type {self.output_type!r}")
        return mask_rows(src, keep, torch.empty(B * T, src.shape[1], device=ppg.device)).view(B, T, -1)

    @torch.no_grad()
    def mel_to_ppg(self, mel, mel_lens):
        ppg, _logits = self.ppg_model.extract(mel, mel_lens, stream=getattr(self, "stream", False))
        true_len = (mel_lens.to("cpu") / (self.ppg_frame_length / self.mel_f_shift)).long().clamp(max=ppg.shape[1])
        return self.ppg_to_target(ppg, true_len), true_len.to(ppg.device)

    @torch.no_grad()
    def audio_to_mel(self, audio, sr=None):
        """audio: wav path or [1, l] tensor (reference :142-158)."""
        from ..infer import audio as A
        from ..infer.utils_infer import load_wav
        if isinstance(audio, str):
            audio, sr = load_wav(audio)
        if audio.ndim == 1:
            audio = audio.unsqueeze(0)
        if sr != 16000:
            audio = A.resample(audio.cpu(), sr, 16000)
        feats, feats_len = self.featCal(audio.to(self.device))
        return feats, feats_len.to(self.device)

    @torch.no_grad()
    def audio_to_ppg(self, audio, sr=None):
        feats, feats_len = self.audio_to_mel(audio, sr)
        return self.mel_to_ppg(feats, feats_len)
