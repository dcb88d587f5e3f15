"""Whisper on the device: the recogniser the reference loads through ``transformers`` -- ``openai/whisper-large-v3-turbo`` to
transcribe a prompt without text (infer/utils_infer.py:148-179) and ``whisper-large-v3`` with the forced prompt
``english / transcribe`` for the English WER (eval/utils_eval.py:631-672).  Greedy decoding, or with ``beam_size > 1`` the pooled
beam search of ``transformers``' ``generate(num_beams=K)`` (what eval/utils_eval.py:517-526 asks of its recogniser with
``beam_size=5``); fp32, eval mode, no CPU path: f5e_whisper_logmel, f5e_cross_attn_decode_f32, f5e_greedy_pick and
f5e_whisper_beam_step (csrc/whisper.hip) plus f5e_im2col, f5e_gemm_f32, f5e_layernorm,
f5e_mha_f32, f5e_attn_decode_f32 and f5e_text_gather; every layer is ``xfmr_f32.layer``, which is handed
the attention launches.  The sub-modules only HOLD the weights, under the Hugging Face
parameter names, so ``load_state_dict`` takes a ``WhisperForConditionalGeneration`` state dict:

    model.encoder.conv1.{weight,bias}, model.encoder.conv2.*, model.encoder.embed_positions.weight,
    model.encoder.layers.{i}.self_attn.{q,v,out}_proj.{weight,bias}, .self_attn.k_proj.weight (no bias),
    .self_attn_layer_norm.*, .fc1.*, .fc2.*, .final_layer_norm.*, model.encoder.layer_norm.*,
    model.decoder.embed_tokens.weight, model.decoder.embed_positions.weight,
    model.decoder.layers.{i}.self_attn.*, .encoder_attn.* (k_proj again without bias), .self_attn_layer_norm.*,
    .encoder_attn_layer_norm.*, .fc1.*, .fc2.*, .final_layer_norm.*, model.decoder.layer_norm.*
    (proj_out.weight is tied to model.decoder.embed_tokens.weight: accepted and dropped)

Token and word times (``token_timestamps``, ``generate(return_token_timestamps=True)``, ``WhisperRecognizer.transcribe_words`` /
``align``): the alignment heads' cross-attention, normalised, median-filtered and warped (f5e_cross_attn_probs_f32,
f5e_dtw_cost_f32, f5e_dtw_path; csrc/whisper_align.hip).

Timestamp tokens and long recordings (``generate(return_timestamps=True)``, ``transcribe_long``, ``detect_language``): the rules
of ``WhisperTimeStampLogitsProcessor`` on the device (f5e_whisper_ts_pick, f5e_whisper_beam_step_ts) and the sequential seek loop
of ``transformers``' long-form ``generate`` with ``condition_on_prev_tokens=False``.

Temperature fallback and sampling (``transcribe_long(fallback=Fallback(...))``, ``generate(temperature=, seed=)``): a window whose
compression ratio or average log-probability misses its threshold is decoded again at the next temperature, sampled on the
device under the same rules (f5e_whisper_sample_pick: Gumbel-max with counter-based Philox noise, so a draw depends on the seed,
the utterance, the decode and the position alone).

Conditioning and prompts (``transcribe_long(context=Context(...))``, ``get_prompt_ids`` / ``encode_text``): a window starts with
<|startofprev|>, the previous windows' text and / or an initial prompt; that prefix goes through the decoder in one pass
(``decoder_prefill``: f5e_whisper_embed, f5e_attn_prefill_f32, f5e_mha_f32 with U queries per row; csrc/whisper_prefill.hip), and
ragged prefixes of a batch are left-padded (f5e_attn_decode_from_f32 for the steps that follow).

Assisted generation (``generate`` / ``transcribe_long`` / ``generate_from_kv(assistant=)``): a draft model (large-v3-turbo's
4-layer decoder, a distil-whisper decoder on the shared encoder) proposes a few tokens per round with cheap cached steps and
this model checks them in one pass behind its cache (``decoder_append``: f5e_attn_append_f32, f5e_gemm_f32_skinny for the
handful of rows; f5e_whisper_verify, f5e_whisper_accept; csrc/whisper_append.hip, csrc/gemm_f32_skinny.hip).  Greedy, with or
without the timestamp rules; the tokens are those of this model alone.

Out of scope: speculative sampling (an assistant with temperature > 0), beam search with an assistant, ``transformers``'
heuristic draft schedule and confidence threshold, per-row positions (the rows of a batch advance together), beam-sample, top-k / top-p, the pipeline's strided ``chunk_length_s`` merging, word timestamps across windows,
the prefill inside ``alignment_probs`` / ``token_timestamps``, patience, CTranslate2's exact search, beam search, assisted
generation and word timestamps from a captured step.

16-bit weights (``Whisper(config, weights="fp16" | "bf16")``, ``from_pretrained_dir(path, weights="auto")``): every
Linear matrix, both conv kernels and the token embedding live on the device once, in the checkpoint's 16 bits, and are widened in
registers by the GEMM that reads them (f5e_gemm_f32_w16, f5e_gemm_f32_w16_skinny, f5e_whisper_embed_w16(_dev);
csrc/gemm_f32_w16.hip).  Biases, LayerNorms, both position tables, activations and caches stay fp32.  Widening is exact and the
summation order is the fp32 kernels', so every decode mode gives the bits of the fp32 model that holds the same (rounded)
values, at half the weight memory and half the bytes per decode step.  That buys memory, not time: the step is bound by its
launches (measured, DESIGN 4o: the captured skinny step is level with fp32), the eager step runs on the register-staged tile and
is 2.3x slower than in fp32, so decode a 16-bit model with ``step_graph=True, step_gemm="skinny"``; the encoder, on the same
tile, is 5 % slower per window.  Out of scope there: 16-bit self or cross K/V caches,
16-bit activations or bf16 / fp16 MFMA for the encoder (it stays compute-bound on the fp32 MFMA and gains memory only), 16-bit
weights for WavLM, wav2vec2 or the wenet models, fp8.

The captured step (``generate`` / ``transcribe_long`` / ``generate_from_kv(step_graph=True)``): the picks of a greedy, ruled or
sampled decode are replayed from one decode step captured as a hipGraph; the position lives in a device record that the
device-position kernels read and advance (f5e_attn_decode_dev_f32, f5e_whisper_embed_dev, f5e_greedy_pick_dev,
f5e_whisper_ts_pick_dev, f5e_whisper_sample_pick_dev; csrc/whisper_step.hip).  The same bits as the eager step.

Ragged batches: samples at or beyond ``lens[b]`` count as zero, and the row is zero-padded to the chunk length as the feature
extractor does; Whisper attends those frames, and so does this.  Row b of a batch equals its own B = 1 run."""
from __future__ import annotations

import json
import math
import os
import struct
import warnings
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from .. import _C, ops
from ..xfmr_f32 import fold, fold_layer, layer

Tensor = torch.Tensor
F32, I32 = torch.float32, torch.int32
# ``Whisper(weights=)``: the type the matrices are stored in on the device (None: fp32, as always)
WEIGHT_MODES = {"f32": None, "fp16": torch.float16, "bf16": torch.bfloat16}

SAMPLE_RATE, N_FFT, HOP = 16000, 400, 160

LANGUAGE_NAMES = {"english": "en", "chinese": "zh", "mandarin": "zh", "german": "de", "spanish": "es", "russian": "ru",
                  "korean": "ko", "french": "fr", "japanese": "ja", "portuguese": "pt", "turkish": "tr", "polish": "pl",
                  "catalan": "ca", "dutch": "nl", "arabic": "ar", "swedish": "sv", "italian": "it", "indonesian": "id",
                  "hindi": "hi", "finnish": "fi", "vietnamese": "vi", "hebrew": "he", "ukrainian": "uk", "greek": "el",
                  "cantonese": "yue"}


@dataclass
class WhisperConfig:
    """Defaults = whisper-large-v3 (the turbo model has decoder_layers = 4)."""
    vocab_size: int = 51866
    num_mel_bins: int = 128
    d_model: int = 1280
    encoder_layers: int = 32
    encoder_attention_heads: int = 20
    encoder_ffn_dim: int = 5120
    decoder_layers: int = 32
    decoder_attention_heads: int = 20
    decoder_ffn_dim: int = 5120
    max_source_positions: int = 1500
    max_target_positions: int = 448
    eos_token_id: int = 50257
    decoder_start_token_id: int = 50258
    activation_function: str = "gelu"
    scale_embedding: bool = False
    # generation_config.json
    suppress_tokens: Tuple[int, ...] = ()
    begin_suppress_tokens: Tuple[int, ...] = ()
    lang_to_id: Dict[str, int] = field(default_factory=dict)
    task_to_id: Dict[str, int] = field(default_factory=dict)
    no_timestamps_token_id: Optional[int] = None
    alignment_heads: Tuple[Tuple[int, int], ...] = ()       # (decoder layer, head) pairs; empty: no token timestamps
    max_initial_timestamp_index: Optional[int] = None       # the first timestamp of a window is at most this many steps of 0.02 s
    prev_sot_token_id: Optional[int] = None                 # <|startofprev|>: leads the previous text / an initial prompt
    median_filter_width: int = 7                            # config.json

    @classmethod
    def from_dicts(cls, config: dict, generation: Optional[dict] = None) -> "WhisperConfig":
        names = {f for f in cls.__dataclass_fields__}
        kw = {k: v for k, v in config.items() if k in names and v is not None}
        for k, v in (generation or {}).items():
            if k in ("suppress_tokens", "begin_suppress_tokens", "lang_to_id", "task_to_id", "no_timestamps_token_id",
                     "alignment_heads", "max_initial_timestamp_index", "prev_sot_token_id") and v is not None:
                kw[k] = v
        for k in ("suppress_tokens", "begin_suppress_tokens"):
            kw[k] = tuple(int(t) for t in kw.get(k) or ())
        heads = kw.get("alignment_heads") or ()
        if any(not isinstance(h, (list, tuple)) or len(h) != 2 for h in heads):
            raise _C.F5EError(f"Whisper: alignment_heads must be [layer, head] pairs (got {heads!r})")
        kw["alignment_heads"] = tuple((int(l), int(h)) for l, h in heads)
        eos = kw.get("eos_token_id")
        if isinstance(eos, (list, tuple)):
            kw["eos_token_id"] = int(eos[0])
        return cls(**kw)

    @property
    def timestamp_begin(self) -> int:
        """The id of <|0.00|>: the class after <|notimestamps|>.  Refused by name when the generation config lacks it."""
        if self.no_timestamps_token_id is None:
            raise _C.F5EError("Whisper: generation_config has no no_timestamps_token_id; timestamp decoding needs it")
        if not self.eos_token_id <= self.no_timestamps_token_id < self.vocab_size - 1:
            raise _C.F5EError(f"Whisper: no_timestamps_token_id = {self.no_timestamps_token_id} leaves no timestamp classes "
                              f"(eos {self.eos_token_id}, vocab_size {self.vocab_size})")
        return self.no_timestamps_token_id + 1

    @property
    def no_speech_token_id(self) -> int:
        """<|nospeech|> = no_timestamps_token_id - 1, the way ``transformers`` derives it for its no-speech detector."""
        return self.timestamp_begin - 2

    def check(self) -> None:
        def refuse(name, why):
            raise _C.F5EError(f"Whisper: {name} = {getattr(self, name)!r} is not built: {why}")
        if self.num_mel_bins not in (80, 128):
            refuse("num_mel_bins", "the front-end has 80 or 128 filters")
        if self.activation_function != "gelu":
            refuse("activation_function", "only the erf GELU is")
        if self.scale_embedding:
            refuse("scale_embedding", "no released checkpoint scales its embeddings")
        for side in ("encoder", "decoder"):
            D, H = self.d_model, getattr(self, side + "_attention_heads")
            if D % H or D // H not in (16, 32, 64, 128):
                refuse(side + "_attention_heads", f"head dim {D / H:g} (16, 32, 64 and 128 are)")
            if getattr(self, side + "_ffn_dim") % 4 or getattr(self, side + "_layers") < 1:
                refuse(side + "_ffn_dim", "a multiple of 4, and at least one layer")
        if self.d_model % 4 or self.max_source_positions < 1 or self.max_source_positions > 4096:
            refuse("max_source_positions", "1 .. 4096 positions, d_model a multiple of 4")
        if not 2 <= self.max_target_positions <= 4096:
            refuse("max_target_positions", "2 .. 4096")
        if not 0 <= self.eos_token_id < self.vocab_size or not 0 <= self.decoder_start_token_id < self.vocab_size:
            refuse("eos_token_id", "eos and decoder_start_token_id must be ids of the vocabulary")
        if len(self.alignment_heads) > 64 or any(not (0 <= l < self.decoder_layers and 0 <= h < self.decoder_attention_heads)
                                                 for l, h in self.alignment_heads):
            refuse("alignment_heads", f"at most 64 (layer, head) pairs with layer < {self.decoder_layers} and head < "
                                      f"{self.decoder_attention_heads}")
        if not 1 <= self.median_filter_width <= 15 or self.median_filter_width % 2 == 0:
            refuse("median_filter_width", "an odd width of 1 .. 15")


# ---- host constants of the front-end (float64, rounded once) ------------------------------------------------------------------
def hann_window(n: int = N_FFT) -> np.ndarray:
    """Periodic Hann."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) * (27.0 / np.log(6.4)), 3.0 * f / 200.0)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), 200.0 * m / 3.0)


def mel_filters(n_mels: int, n_fft: int = N_FFT, sr: int = SAMPLE_RATE) -> np.ndarray:
    """Slaney mel scale, Slaney (area) normalisation, 0 .. sr / 2: float64 [n_fft / 2 + 1][n_mels], the extractor's
    ``mel_filters``."""
    bins = n_fft // 2 + 1
    fft_freqs = np.linspace(0.0, sr // 2, bins)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2.0), n_mels + 2))
    diff = np.diff(edges)
    slopes = edges[None, :] - fft_freqs[:, None]
    fb = np.maximum(0.0, np.minimum(-slopes[:, :-2] / diff[:-1], slopes[:, 2:] / diff[1:]))
    return fb * (2.0 / (edges[2:n_mels + 2] - edges[:n_mels]))[None, :]


def dft_twiddle(n: int = N_FFT) -> np.ndarray:
    a = 2.0 * np.pi * np.arange(n, dtype=np.float64) / n
    return np.stack([np.cos(a), np.sin(a)], 1)


def sinusoids(length: int, channels: int, max_timescale: float = 10000.0) -> Tensor:
    """The encoder's fixed position table (what a fresh ``WhisperEncoder`` holds; checkpoints carry it too)."""
    inc = math.log(max_timescale) / (channels // 2 - 1)
    inv = torch.exp(-inc * torch.arange(channels // 2, dtype=torch.float32))
    t = torch.arange(length, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.cat([t.sin(), t.cos()], 1)


# ---- byte-level detokenisation ------------------------------------------------------------------------------------------------
def bytes_to_unicode() -> Dict[int, str]:
    """GPT-2's byte -> printable character table: the printable Latin-1 bytes map to themselves, the others to 256, 257, ..."""
    keep = set(range(ord("!"), ord("~") + 1)) | set(range(0xA1, 0xAD)) | set(range(0xAE, 0x100))
    table, n = {}, 0
    for b in range(256):
        if b in keep:
            table[b] = chr(b)
        else:
            table[b] = chr(256 + n)
            n += 1
    return table


_U2B = {c: b for b, c in bytes_to_unicode().items()}


def decode_pieces(id_to_piece: Dict[int, str], first_special: int, ids: Sequence[int], skip_special_tokens: bool = True) -> str:
    """Byte-level BPE pieces -> text: the pieces' characters back to bytes, UTF-8 with ``errors="replace"`` (a character split
    across tokens is joined first).  Ids at or above ``first_special`` are dropped (or, kept, spelled as they are)."""
    out, raw = [], bytearray()
    for i in ids:
        i = int(i)
        if i >= first_special:
            if not skip_special_tokens and i in id_to_piece:
                out.append(raw.decode("utf-8", errors="replace"))
                raw = bytearray()
                out.append(id_to_piece[i])
            continue
        piece = id_to_piece.get(i)
        if piece is None:
            continue
        raw.extend(_U2B[c] for c in piece if c in _U2B)
    out.append(raw.decode("utf-8", errors="replace"))
    return "".join(out)


# ---- byte-level tokenisation (GPT-2's BPE, what WhisperTokenizer applies to plain text) ------------------------------------------------
GPT2_PATTERN = r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"


def bpe_merge(word: Sequence[str], ranks: Dict[Tuple[str, str], int]) -> List[str]:
    """The symbols of one pre-token merged greedily by rank: the lowest-ranked adjacent pair, every occurrence left to right,
    until no pair has a rank."""
    word = list(word)
    while len(word) > 1:
        best = min(((ranks.get(pair, math.inf), pair) for pair in zip(word[:-1], word[1:])), key=lambda t: t[0])
        if best[0] == math.inf:
            break
        a, b = best[1]
        out, i = [], 0
        while i < len(word):
            if i + 1 < len(word) and word[i] == a and word[i + 1] == b:
                out.append(a + b)
                i += 2
            else:
                out.append(word[i])
                i += 1
        word = out
    return word


# ---- tokens -> words (transformers' tokenization_whisper.py: _combine_tokens_into_words) ----------------------------------------
UNSPACED_LANGUAGES = {"zh", "ja", "th", "lo", "my", "yue", "chinese", "japanese", "thai", "lao", "myanmar", "cantonese"}
PREPEND_PUNCTUATIONS = "\"'“¡¿([{-"
APPEND_PUNCTUATIONS = "\"'.。,，!！?？:：”)]}、"
_ASCII_PUNCTUATION = "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"


def group_tokens(id_to_piece: Dict[int, str], first_special: int, ids: Sequence[int], language: Optional[str] = None,
                 special_from: Optional[int] = None) -> Tuple[List[str], List[List[int]]]:
    """-> (words, token indices per word), the reference's grouping rules:
    1. cut wherever the tokens so far decode to whole unicode characters (specials spelled out): a character split across tokens
       stays in one piece; a replacement character that the full text has at that place too counts as whole;
    2. unless the language is written without spaces (zh / ja / th / lo / my / yue), a piece joins the word before it unless it
       is a special (first id >= ``special_from``, the eos id), starts with a space, is ASCII punctuation, or is the first;
    3. a word that starts with a space and is otherwise a prepend mark ("'([{- ...) joins the word after it (right to left), then a
       word that is an append mark (.,!?:)]} ...) joins a word before it that does not end with a space (left to right)."""
    ids = [int(i) for i in ids]
    special_from = first_special if special_from is None else special_from

    def dec(tok):
        return decode_pieces(id_to_piece, first_special, tok, skip_special_tokens=False)
    full, bad = dec(ids), "�"
    words, index, cur, offset = [], [], [], 0
    for k in range(len(ids)):
        cur.append(k)
        text = dec([ids[i] for i in cur])
        at = offset + text.index(bad) if bad in text else -1
        if at < 0 or at >= len(full) or full[at] == bad:
            words.append(text)
            index.append(cur)
            cur = []
            offset += len(text)
    if (language or "en").lower() not in UNSPACED_LANGUAGES:
        pieces, words, index = list(zip(words, index)), [], []
        for text, idx in pieces:
            if ids[idx[0]] >= special_from or text.startswith(" ") or text.strip() in _ASCII_PUNCTUATION or not words:
                words.append(text)
                index.append(list(idx))
            else:
                words[-1] += text
                index[-1].extend(idx)
    i, j = len(words) - 2, len(words) - 1
    while i >= 0:
        if words[i].startswith(" ") and words[i].strip() in PREPEND_PUNCTUATIONS:
            words[j], index[j] = words[i] + words[j], index[i] + index[j]
            words[i], index[i] = "", []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(words):
        if not words[i].endswith(" ") and words[j] in APPEND_PUNCTUATIONS:
            words[i], index[i] = words[i] + words[j], index[i] + index[j]
            words[j], index[j] = "", []
        else:
            i = j
        j += 1
    keep = [k for k in range(len(words)) if words[k]]
    return [words[k] for k in keep], [index[k] for k in keep]


# ---- long-form: a window's tokens -> segments (transformers' generation_whisper.py: _retrieve_segment) ----------------------------
TIME_PRECISION, INPUT_STRIDE = 0.02, 2      # seconds per timestamp step; mel frames per encoder position
STEP_STATES = 4                             # captured decode steps kept per model (``step_graph``): an LRU


@dataclass
class Segment:
    """One segment of ``transcribe_long``: times in seconds from the start of the recording, the tokens of the slice (its
    timestamp tokens included), the window's first frame, and the window's figures (shared by the segments of a window)."""
    start_s: float
    end_s: float
    tokens: List[int]
    seek: int
    avg_logprob: float
    no_speech_prob: float
    compression_ratio: float
    temperature: float = 0.0      # of the attempt that was kept for the window (``Fallback``)


@dataclass(frozen=True)
class Fallback:
    """Temperature fallback of ``transcribe_long`` (``transformers``' ``generate_with_fallback`` / ``_need_fallback``): a window is
    decoded at ``temperatures[0]`` and again at the next entry while its compression ratio exceeds
    ``compression_ratio_threshold`` or its average log-probability falls below ``logprob_threshold`` (None: that test is off);
    the last attempt is kept.  0 decodes greedily (or with the beams asked for), a positive entry samples one row per utterance
    with f5e_whisper_sample_pick and ``seed``.  ``logprob_threshold`` is also the one the no-speech skip uses."""
    temperatures: Tuple[float, ...] = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)
    compression_ratio_threshold: Optional[float] = None
    logprob_threshold: Optional[float] = None
    seed: int = 0

    def __post_init__(self):
        t = self.temperatures
        try:
            t = tuple(float(v) for v in ((t,) if isinstance(t, (int, float)) else t))
        except (TypeError, ValueError):
            raise _C.F5EError(f"Fallback: temperatures = {self.temperatures!r} is not a sequence of numbers") from None
        if not t or not all(math.isfinite(v) and v >= 0.0 for v in t):
            raise _C.F5EError(f"Fallback: temperatures = {self.temperatures!r} must be a non-empty sequence of finite values >= 0")
        for name in ("compression_ratio_threshold", "logprob_threshold"):
            v = getattr(self, name)
            if v is not None and not (isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)):
                raise _C.F5EError(f"Fallback: {name} = {v!r} must be None or a finite number")
        if isinstance(self.seed, bool) or not isinstance(self.seed, int) or not 0 <= self.seed < 1 << 64:
            raise _C.F5EError(f"Fallback: seed = {self.seed!r} must be an integer in 0 .. 2^64 - 1")
        object.__setattr__(self, "temperatures", t)


@dataclass(frozen=True)
class Context:
    """What a window of ``transcribe_long`` is given in front of its forced tokens (``transformers``' long-form ``generate``):
    ``condition_on_prev_tokens``: <|startofprev|> and the row's previous text (``previous_text``); ``prompt_ids``: an initial
    prompt, ``[<|startofprev|>, ids ...]`` as ``Whisper.get_prompt_ids`` makes it.  ``prompt_condition_type``:
      * "first-segment": the prompt (without its <|startofprev|>) counts as the row's first previous segment, so under
        conditioning it leads the first window's previous text and then scrolls out of the last ``max_target_positions // 2 -
        1`` tokens; a window that is NOT conditioned gets the whole prompt in front of its forced tokens, every such window, as
        ``_prepare_decoder_input_ids`` does.  The returned segments never contain it;
      * "all-segments": the prompt takes the place of <|startofprev|> in front of the previous text of every window; it needs
        conditioning (refused otherwise, as ``transformers`` refuses it)."""
    condition_on_prev_tokens: bool = False
    prompt_ids: Optional[Tuple[int, ...]] = None
    prompt_condition_type: str = "first-segment"

    def __post_init__(self):
        if not isinstance(self.condition_on_prev_tokens, bool):
            raise _C.F5EError(f"Context: condition_on_prev_tokens = {self.condition_on_prev_tokens!r} must be a bool")
        if self.prompt_condition_type not in ("first-segment", "all-segments"):
            raise _C.F5EError(f"Context: prompt_condition_type = {self.prompt_condition_type!r} must be 'first-segment' or "
                              "'all-segments'")
        if self.prompt_condition_type == "all-segments" and not self.condition_on_prev_tokens:
            raise _C.F5EError("Context: prompt_condition_type = 'all-segments' needs condition_on_prev_tokens = True")
        ids = self.prompt_ids
        if ids is not None:
            try:
                ids = tuple(int(t) for t in (ids.tolist() if hasattr(ids, "tolist") else ids))
            except (TypeError, ValueError):
                raise _C.F5EError(f"Context: prompt_ids = {self.prompt_ids!r} is not a sequence of token ids") from None
            if not ids:
                raise _C.F5EError("Context: prompt_ids is empty (None switches the prompt off)")
            object.__setattr__(self, "prompt_ids", ids)


def conditions_next_window(temperature: Optional[float]) -> bool:
    """``is_low_temperature`` of ``generate_with_fallback``: a window kept at a temperature of 0.5 or more does not condition
    the next one."""
    return temperature is None or temperature < 0.5


def previous_text(history: Sequence[Sequence[int]], ts_begin: int, cut: int) -> List[int]:
    """The tokens of a row's segments so far (timestamps included) as ``_pad_to_max_length(skip_ending_double_timestamps=True,
    cut_off_length=cut)`` joins them: a segment of more than two tokens whose last but one is a timestamp loses its last token
    (the closing pair's second timestamp), and the whole is cut to its LAST ``cut`` tokens."""
    seq: List[int] = []
    for seg in history:
        seg = [int(t) for t in seg]
        seq.extend(seg[:-1] if len(seg) > 2 and seg[-2] >= ts_begin else seg)
    return seq[-cut:] if cut > 0 else []


def window_prompt(ctx: Optional[Context], forced: Sequence[int], history: Sequence[Sequence[int]], conditioned: bool,
                  prev_sot: Optional[int], ts_begin: int, cut: int) -> List[int]:
    """The decoder input of one row's window (``_prepare_decoder_input_ids`` for that row alone): ``forced`` = <|startof
    transcript|> <|lang|> <|task|>; ``history``: the row's segments so far (with the "first-segment" prompt as the first of
    them); ``conditioned``: the context conditions and the row's last window was kept at a low temperature.  A row is
    conditioned iff it has history of its own."""
    forced = [int(t) for t in forced]
    if ctx is None:
        return forced
    if conditioned and ctx.condition_on_prev_tokens and len(history) > 0:
        lead = list(ctx.prompt_ids) if ctx.prompt_ids is not None and ctx.prompt_condition_type == "all-segments" else [prev_sot]
        return lead + previous_text(history, ts_begin, cut) + forced
    if ctx.prompt_ids is not None:
        return list(ctx.prompt_ids) + forced
    return forced


def split_segments(seq: Sequence[int], ts_begin: int, seek_frames: int, num_frames: int
                   ) -> Tuple[List[Tuple[float, float, List[int]]], int]:
    """The generated tokens of one window (prompt and closing eos removed) -> ([(start_s, end_s, tokens)], mel frames by which
    the window advances).  ``seek_frames``: the window's first frame, ``num_frames``: the frames of the recording it covers.
      * consecutive timestamp pairs cut the sequence; a segment runs from its first token's time to its closing timestamp's;
      * the sequence ends ``text, timestamp`` (single timestamp ending): the rest is the last segment, and the whole window is
        consumed; otherwise what follows the last pair is dropped and the next window starts at that pair's time;
      * no pair at all: one segment over the window, ending at the last timestamp if there is one other than <|0.00|>, else
        at the window's end (``int(num_frames * 0.01 / 0.02)`` steps, in float32 as the reference evaluates it).
    Times are float64: seek_frames * 0.02 / 2 + steps * 0.02."""
    seq = [int(t) for t in seq]
    is_ts = [t >= ts_begin for t in seq]
    offset = float(seek_frames) * TIME_PRECISION / INPUT_STRIDE
    single = is_ts[-2:] == [False, True]
    cuts = [i + 1 for i in range(len(seq) - 1) if is_ts[i] and is_ts[i + 1]]
    if not cuts:
        stamps = [t for t in seq if t >= ts_begin]
        last_pos = int(np.float32(num_frames) * np.float32(0.01) / np.float32(TIME_PRECISION))
        if stamps and stamps[-1] != ts_begin:
            last_pos = float(stamps[-1] - ts_begin)
        return [(offset, offset + last_pos * TIME_PRECISION, seq)], int(num_frames)
    if single:
        cuts.append(len(seq))
    else:
        cuts[-1] += 1                          # the last segment keeps the pair's second timestamp
    out, lo = [], 0
    for k, hi in enumerate(cuts):
        piece = seq[lo:hi]
        end_tok = piece[-1] if (k < len(cuts) - 1 or single) else piece[-2]
        out.append((offset + float(piece[0] - ts_begin) * TIME_PRECISION, offset + float(end_tok - ts_begin) * TIME_PRECISION, piece))
        lo = hi
    return out, int(num_frames) if single else (seq[lo - 2] - ts_begin) * INPUT_STRIDE


def compression_ratio(tokens: Sequence[int], vocab_size: int) -> float:
    """zlib on the tokens' little-endian bytes, as ``_retrieve_compression_ratio``: reported, and acted on by ``Fallback``."""
    import zlib
    width = int(math.log2(vocab_size) / 8) + 1
    raw = b"".join(int(t).to_bytes(width, "little") for t in tokens)
    return len(raw) / len(zlib.compress(raw)) if raw else 0.0


# ---- checkpoint reading (the safetensors container: u64 header length, JSON header, raw little-endian data) ---------------------
_ST_DTYPES = {"F32": np.dtype("<f4"), "F16": np.dtype("<f2"), "BF16": np.dtype("<u2"), "F64": np.dtype("<f8")}


def read_safetensors(path: str, stored: bool = False) -> Dict[str, Tensor]:
    """Every floating tensor of a ``.safetensors`` file as float32 (fp16 and bf16 are widened, which is exact).  ``stored``: in
    the type the file stores it in instead (F16 -> torch.float16, BF16 -> torch.bfloat16, F32, F64), bit for bit."""
    out = {}
    with open(path, "rb") as f:
        (n,) = struct.unpack("<Q", f.read(8))
        header = json.loads(f.read(n).decode("utf-8"))
        base = 8 + n
        for name, meta in header.items():
            if name == "__metadata__" or meta["dtype"] not in _ST_DTYPES:
                continue
            lo, hi = meta["data_offsets"]
            f.seek(base + lo)
            arr = np.frombuffer(f.read(hi - lo), dtype=_ST_DTYPES[meta["dtype"]])
            if stored:
                t = torch.from_numpy(np.array(arr).view(np.int16) if meta["dtype"] == "BF16" else np.array(arr))
                out[name] = (t.view(torch.bfloat16) if meta["dtype"] == "BF16" else t).reshape(meta["shape"])
                continue
            if meta["dtype"] == "BF16":
                arr = (arr.astype(np.uint32) << 16).view(np.float32)
            out[name] = torch.from_numpy(np.array(arr, dtype=np.float32).reshape(meta["shape"]))
    return out


def cast_checked(name: str, t: Tensor, dtype) -> Tensor:
    """``t`` in ``dtype``: a pure copy when it has that type, otherwise rounded to nearest-even where ``dtype`` does not hold
    the value.  A finite value that would become infinite (fp32 -> fp16 beyond 65504) is refused, naming the parameter."""
    if not isinstance(t, Tensor) or not t.is_floating_point():
        raise _C.F5EError(f"Whisper.load_state_dict: {name} must be a floating tensor (got {getattr(t, 'dtype', type(t))})")
    if t.dtype == dtype:
        return t
    r = t.detach().to(dtype)                     # torch converts floating types with round-to-nearest-even
    bad = torch.isinf(r) & torch.isfinite(t)
    if bool(bad.any()):
        worst = float(t.detach()[bad].double().abs().max())
        raise _C.F5EError(f"Whisper.load_state_dict: {name} holds {worst:g}, which {str(dtype).replace('torch.', '')} cannot "
                          f"hold (its largest finite value is {torch.finfo(dtype).max:g}): load it with another weights= mode")
    return r


_MATRIX_SUFFIXES = ("_proj.weight", "fc1.weight", "fc2.weight", "conv1.weight", "conv2.weight", "embed_tokens.weight")


def is_matrix(name: str) -> bool:
    """Whether the parameter ``name`` is stored in the weight mode's type: the Linear matrices, both conv kernels and the token
    embedding.  Everything else (biases, LayerNorms, both position tables) is fp32 in every mode."""
    return name.endswith(_MATRIX_SUFFIXES)


# ---- weight holders -------------------------------------------------------------------------------------------------------------
class _Attn(nn.Module):
    def __init__(self, D: int):
        super().__init__()
        self.q_proj, self.v_proj, self.out_proj = nn.Linear(D, D), nn.Linear(D, D), nn.Linear(D, D)
        self.k_proj = nn.Linear(D, D, bias=False)


class _EncLayer(nn.Module):
    def __init__(self, D: int, FF: int):
        super().__init__()
        self.self_attn, self.self_attn_layer_norm = _Attn(D), nn.LayerNorm(D)
        self.fc1, self.fc2, self.final_layer_norm = nn.Linear(D, FF), nn.Linear(FF, D), nn.LayerNorm(D)


class _DecLayer(_EncLayer):
    def __init__(self, D: int, FF: int):
        super().__init__(D, FF)
        self.encoder_attn, self.encoder_attn_layer_norm = _Attn(D), nn.LayerNorm(D)


class _Encoder(nn.Module):
    def __init__(self, cfg: WhisperConfig):
        super().__init__()
        D = cfg.d_model
        self.conv1 = nn.Conv1d(cfg.num_mel_bins, D, 3, padding=1)
        self.conv2 = nn.Conv1d(D, D, 3, stride=2, padding=1)
        self.embed_positions = nn.Embedding(cfg.max_source_positions, D)
        self.layers = nn.ModuleList([_EncLayer(D, cfg.encoder_ffn_dim) for _ in range(cfg.encoder_layers)])
        self.layer_norm = nn.LayerNorm(D)
        with torch.no_grad():
            self.embed_positions.weight.copy_(sinusoids(cfg.max_source_positions, D))


class _Decoder(nn.Module):
    def __init__(self, cfg: WhisperConfig):
        super().__init__()
        D = cfg.d_model
        self.embed_tokens = nn.Embedding(cfg.vocab_size, D)
        self.embed_positions = nn.Embedding(cfg.max_target_positions, D)
        self.layers = nn.ModuleList([_DecLayer(D, cfg.decoder_ffn_dim) for _ in range(cfg.decoder_layers)])
        self.layer_norm = nn.LayerNorm(D)


class _Model(nn.Module):
    def __init__(self, cfg: WhisperConfig):
        super().__init__()
        self.encoder, self.decoder = _Encoder(cfg), _Decoder(cfg)


def _prompt_len(prompt) -> int:
    """Tokens of a prompt given as ids for all rows or as [B, n0] ids."""
    if isinstance(prompt, Tensor):
        return prompt.shape[-1]
    return len(prompt[0]) if len(prompt) and isinstance(prompt[0], (list, tuple)) else len(prompt)


def _gemm(a, w, bias=None, **kw):
    """``ops.gemm_f32`` or, for a 16-bit weight, ``ops.gemm_f32_w16``: the ``gemm`` hook of ``xfmr_f32.layer``."""
    return (ops.gemm_f32 if w.dtype == F32 else ops.gemm_f32_w16)(a, w, bias, **kw)


def _gemm_skinny(a, w, bias=None, **kw):
    return (ops.gemm_f32_skinny if w.dtype == F32 else ops.gemm_f32_w16_skinny)(a, w, bias, **kw)


def _embed(ids, emb, *a):
    return (ops.whisper_embed if emb.dtype == F32 else ops.whisper_embed_w16)(ids, emb, *a)


def _f(t: Tensor, dev) -> Tensor:
    return t.detach().to(dev, F32).contiguous()


class Whisper(nn.Module):
    def __init__(self, config: Optional[WhisperConfig] = None, weights: str = "f32"):
        """``weights``: "f32" (the default: nothing changes), or "fp16" / "bf16": the matrices (``is_matrix``) are held in that
        type, once, and widened in registers by the GEMMs that read them; every decode path gives the bits of the fp32 model
        with the same values."""
        super().__init__()
        self.cfg = cfg = config or WhisperConfig()
        cfg.check()
        if weights not in WEIGHT_MODES:
            raise _C.F5EError(f"Whisper: weights = {weights!r} must be one of {sorted(WEIGHT_MODES)}")
        self.weights, self.wdtype = weights, WEIGHT_MODES[weights]
        self.model = _Model(cfg)
        if self.wdtype is not None:
            for name, p in self.named_parameters():
                if is_matrix(name):
                    p.data = p.data.to(self.wdtype)
        self.id_to_piece: Dict[int, str] = {}
        self.first_special = cfg.eos_token_id
        self.bpe_ranks: Dict[Tuple[str, str], int] = {}
        self._piece_to_id: Optional[Dict[str, int]] = None
        self._folded = None
        super().train(False)
        for p in self.parameters():
            p.requires_grad_(False)

    # ---- loading ---------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_pretrained_dir(cls, path: str, weights: str = "f32") -> "Whisper":
        """A local Hugging Face model directory: ``config.json``, ``generation_config.json``, ``model.safetensors`` (or
        ``model.safetensors.index.json`` and its shards), ``vocab.json`` and ``added_tokens.json``.  ``weights``: the mode of
        ``Whisper(weights=)``, or "auto": the type the checkpoint stores its matrices in (fp16 files load as "fp16" without
        a rounding; a file of mixed or other types as "f32")."""
        if weights != "auto" and weights not in WEIGHT_MODES:
            raise _C.F5EError(f"Whisper.from_pretrained_dir: weights = {weights!r} must be 'auto' or one of {sorted(WEIGHT_MODES)}")
        def js(name, required=True):
            p = os.path.join(path, name)
            if not os.path.exists(p):
                if required:
                    raise _C.F5EError(f"Whisper.from_pretrained_dir: {p} is missing")
                return None
            with open(p, encoding="utf-8") as f:
                return json.load(f)
        config = WhisperConfig.from_dicts(js("config.json"), js("generation_config.json", False))
        index = js("model.safetensors.index.json", False)
        files = sorted(set(index["weight_map"].values())) if index else ["model.safetensors"]
        sd = {}
        for name in files:
            p = os.path.join(path, name)
            if not os.path.exists(p):
                raise _C.F5EError(f"Whisper.from_pretrained_dir: {p} is missing")
            sd.update(read_safetensors(p, stored=weights != "f32"))
        if weights == "auto":
            stored = {v.dtype for k, v in sd.items() if is_matrix(k)}
            weights = {(torch.float16,): "fp16", (torch.bfloat16,): "bf16"}.get(tuple(stored), "f32")
        model = cls(config, weights=weights)
        model.load_state_dict(sd)
        vocab = js("vocab.json", False)
        if vocab is not None:
            model.set_vocab(vocab, js("added_tokens.json", False))
        merges = os.path.join(path, "merges.txt")
        if os.path.exists(merges):
            with open(merges, encoding="utf-8") as f:
                model.set_merges(f.read().split("\n"))
        return model

    def set_vocab(self, vocab: Dict[str, int], added: Optional[Dict[str, int]] = None) -> None:
        """``vocab.json`` (piece -> id) and ``added_tokens.json`` (special -> id); the first special id is the lowest added id
        (the eos id when there is no such file)."""
        self.id_to_piece = {int(i): p for p, i in vocab.items()}
        self._piece_to_id = None
        self.first_special = self.cfg.eos_token_id
        if added:
            self.id_to_piece.update({int(i): p for p, i in added.items()})
            self.first_special = min(min(int(i) for i in added.values()), self.cfg.eos_token_id)

    def set_merges(self, merges: Sequence) -> None:
        """``merges.txt``: its lines ("a b"; a "#version" header and empty lines are skipped) or (a, b) pairs, best first."""
        pairs = []
        for m in merges:
            if isinstance(m, str):
                if not m.strip() or m.startswith("#version"):
                    continue
                m = m.split(" ")
            if len(m) != 2:
                raise _C.F5EError(f"Whisper.set_merges: {m!r} is not a pair of symbols")
            pairs.append((str(m[0]), str(m[1])))
        self.bpe_ranks = {pair: i for i, pair in enumerate(pairs)}

    def encode_text(self, text: str) -> List[int]:
        """Plain text -> ids: the GPT-2 pre-tokeniser pattern, the pieces' UTF-8 bytes as printable characters, merged by the
        ranks of ``merges.txt`` (what ``WhisperTokenizer`` does with text that holds no special token).  ``decode_ids`` undoes it."""
        if not self.id_to_piece or not self.bpe_ranks:
            raise _C.F5EError("Whisper.encode_text: needs vocab.json and merges.txt (set_vocab and set_merges, or a checkpoint "
                              "directory that holds both)")
        try:
            import regex
        except ImportError:
            raise _C.F5EError("Whisper.encode_text: the 'regex' module is not installed (the GPT-2 pre-tokeniser pattern needs "
                              "\\p{L} / \\p{N})") from None
        if self._piece_to_id is None:                                   # reset by set_vocab
            self._piece_to_id = {p: i for i, p in self.id_to_piece.items()}
        piece_to_id = self._piece_to_id
        b2u, ids = bytes_to_unicode(), []
        for tok in regex.findall(GPT2_PATTERN, text):
            for piece in bpe_merge([b2u[b] for b in tok.encode("utf-8")], self.bpe_ranks):
                if piece not in piece_to_id:
                    raise _C.F5EError(f"Whisper.encode_text: piece {piece!r} of {tok!r} is not in the vocabulary")
                ids.append(piece_to_id[piece])
        return ids

    def get_prompt_ids(self, text: str) -> List[int]:
        """``WhisperTokenizer.get_prompt_ids``: [<|startofprev|>] + the ids of " " + text.strip(); for ``Context(prompt_ids=)``.
        Text that spells a special token is refused."""
        if self.cfg.prev_sot_token_id is None:
            raise _C.F5EError("Whisper.get_prompt_ids: generation_config has no prev_sot_token_id (<|startofprev|>)")
        for i, piece in self.id_to_piece.items():
            if i >= self.first_special and piece and piece in text:
                raise _C.F5EError(f"Whisper.get_prompt_ids: the text contains the special token {piece}, which a prompt must not")
        return [self.cfg.prev_sot_token_id] + self.encode_text(" " + text.strip())

    def decode_ids(self, ids: Sequence[int], skip_special_tokens: bool = True) -> str:
        if not self.id_to_piece:
            raise _C.F5EError("Whisper.decode_ids: no vocabulary is loaded (set_vocab / from_pretrained_dir with vocab.json)")
        return decode_pieces(self.id_to_piece, self.first_special, ids, skip_special_tokens)

    def words_from_tokens(self, ids: Sequence[int], times: Sequence[float], language: Optional[str] = None
                          ) -> List[Tuple[str, float, float]]:
        """A hypothesis (prompt and closing eos included) and its token times -> [(word, start_s, end_s)] by ``group_tokens``;
        specials are skipped.  A word starts at its first token's time and ends at the time of the token after its last one (the
        next word's start; for the last word the closing token's time), or at its last token's time when nothing follows."""
        if not self.id_to_piece:
            raise _C.F5EError("Whisper.words_from_tokens: no vocabulary is loaded (set_vocab / from_pretrained_dir with vocab.json)")
        ids, times = [int(i) for i in ids], [float(t) for t in times]
        if len(times) != len(ids):
            raise _C.F5EError(f"Whisper.words_from_tokens: {len(ids)} tokens need {len(ids)} times (got {len(times)})")
        words, index = group_tokens(self.id_to_piece, self.first_special, ids, language, self.cfg.eos_token_id)
        out = []
        for word, idx in zip(words, index):
            if ids[idx[0]] >= self.cfg.eos_token_id:
                continue
            out.append((word, times[idx[0]], times[min(idx[-1] + 1, len(ids) - 1)]))
        return out

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """Any floating dtype per tensor (``cast_checked``): a matrix goes to the weight mode's type, everything else to fp32; a
        tensor that has its target type is copied as it is."""
        sd = {k: cast_checked(k, v, self.wdtype if self.wdtype is not None and is_matrix(k) else F32)
              for k, v in state_dict.items() if k != "proj_out.weight"}            # tied to model.decoder.embed_tokens.weight
        self._folded = None
        return super().load_state_dict(sd, strict=strict, **kw)

    def device_bytes(self) -> int:
        """Bytes of device memory behind every tensor the model holds (parameters and what ``_fold`` keeps beside them: stacked
        projections, the front-end's tables, suppression lists; no decode state), each storage counted once."""
        fd = self._fold()
        seen, stack = {}, [list(self.parameters()), {k: v for k, v in fd.items() if k != "step_states"}]
        while stack:
            o = stack.pop()
            if isinstance(o, Tensor):
                if o.is_cuda:
                    st = o.untyped_storage()
                    seen[st.data_ptr()] = st.nbytes()
            elif isinstance(o, dict):
                stack.extend(o.values())
            elif isinstance(o, (list, tuple)):
                stack.extend(o)
        return sum(seen.values())

    def train(self, mode: bool = True):
        if mode:
            raise _C.F5EError("Whisper: training is out of scope (eval mode only)")
        return super().train(False)

    def _apply(self, fn, *a, **kw):
        self._folded = None
        return super()._apply(fn, *a, **kw)

    # ---- weights as the kernels take them, once per load -----------------------------------------------------------------------
    def _fold(self) -> dict:
        dev = self.model.decoder.embed_tokens.weight.device
        if self._folded is not None and self._folded["device"] == dev:
            return self._folded
        if dev.type != "cuda":
            raise _C.F5EError(f"Whisper lives on {dev}: move it to the GPU (there is no CPU path)")
        cfg, enc, dec = self.cfg, self.model.encoder, self.model.decoder

        def rec(lyr, ca=None):        # k_proj has no bias: fold_layer leaves zeros in the k third of qkv[1], the k half of xkv[1]
            sa = lyr.self_attn
            x = dict(ln_x=lyr.encoder_attn_layer_norm, xq=ca.q_proj, xk=ca.k_proj, xv=ca.v_proj, xout=ca.out_proj) if ca else {}
            W = fold_layer(dev, lyr.self_attn_layer_norm, sa.q_proj, sa.k_proj, sa.v_proj, sa.out_proj, lyr.final_layer_norm,
                           lyr.fc1, lyr.fc2, wdtype=wd, **x)
            if wd is not None:        # stored once: q, k, v (and the cross k, v) become views of the stacked record
                share(W.qkv, sa.q_proj, sa.k_proj, sa.v_proj)
                if ca:
                    share(W.xkv, ca.k_proj, ca.v_proj)
            return W

        def share(pair, *ms):
            r = 0
            for m in ms:
                n = m.weight.shape[0]
                m.weight.data = pair[0][r:r + n]
                if m.bias is not None:
                    m.bias.data = pair[1][r:r + n]
                r += n

        def conv_w(conv):             # tap-major: k = tap * C_in + ic, the column order of f5e_im2col
            w = conv.weight.detach().to(dev).permute(0, 2, 1)
            w2 = w.reshape(w.shape[0], -1).contiguous()
            if wd is not None:        # the parameter becomes the [out, in, tap] view of the layout the GEMM reads
                conv.weight.data = w2.view(w.shape).permute(0, 2, 1)
            return w2
        wd = self.wdtype
        mat = (lambda t: _f(t, dev)) if wd is None else (lambda t: t.detach().to(dev).contiguous())   # noqa: E731
        fd = dict(device=dev,
                  window=torch.from_numpy(hann_window()).to(dev, F32), twiddle=torch.from_numpy(dft_twiddle()).to(dev, F32).contiguous(),
                  fb=torch.from_numpy(mel_filters(cfg.num_mel_bins)).to(dev, F32).contiguous(),
                  c1_w=mat(conv_w(enc.conv1)), c1_b=_f(enc.conv1.bias, dev),
                  c2_w=mat(conv_w(enc.conv2)), c2_b=_f(enc.conv2.bias, dev),
                  enc_pos=_f(enc.embed_positions.weight, dev), enc_ln=fold(dev, enc.layer_norm), enc=[rec(l) for l in enc.layers],
                  emb=mat(dec.embed_tokens.weight), dec_pos=_f(dec.embed_positions.weight, dev), dec_ln=fold(dev, dec.layer_norm),
                  dec=[rec(l, l.encoder_attn) for l in dec.layers])
        fd["suppress"] = torch.tensor(list(cfg.suppress_tokens), dtype=I32, device=dev) if cfg.suppress_tokens else None
        fd["begin_suppress"] = torch.tensor(list(cfg.begin_suppress_tokens), dtype=I32, device=dev) if cfg.begin_suppress_tokens else None
        # language detection = a greedy pick that suppresses every class but the language ids
        langs = {int(v) for v in cfg.lang_to_id.values()}
        fd["not_lang"] = torch.tensor([v for v in range(cfg.vocab_size) if v not in langs], dtype=I32, device=dev) if langs else None
        # alignment heads, in the order of the list: layer -> [(first slot, heads i32 [k])], one entry per run of consecutive pairs
        # of that layer (one f5e_cross_attn_probs_f32 launch each)
        fd["align"] = {}
        s = 0
        while s < len(cfg.alignment_heads):
            e = s
            while e < len(cfg.alignment_heads) and cfg.alignment_heads[e][0] == cfg.alignment_heads[s][0]:
                e += 1
            heads = torch.tensor([h for _, h in cfg.alignment_heads[s:e]], dtype=I32, device=dev)
            fd["align"].setdefault(cfg.alignment_heads[s][0], []).append((s, heads))
            s = e
        self._folded = fd
        return fd

    # ---- front-end + encoder --------------------------------------------------------------------------------------------------
    @property
    def n_frames(self) -> int:
        return 2 * self.cfg.max_source_positions

    def _check_audio(self, wav: Tensor, lens, name: str) -> Tuple[Tensor, Optional[Tensor]]:
        if not isinstance(wav, Tensor) or wav.ndim != 2 or wav.dtype != F32 or wav.shape[0] < 1 or wav.shape[1] < 1:
            raise _C.F5EError(f"Whisper.{name}: wav must be a non-empty float32 tensor [B, S]")
        if not wav.is_cuda:
            raise _C.F5EError(f"Whisper.{name}: wav lives on {wav.device}; there is no CPU path")
        B, S = wav.shape
        if lens is not None and not (isinstance(lens, Tensor) and lens.is_cuda):
            host = [int(v) for v in (lens.tolist() if isinstance(lens, Tensor) else lens)]
            if len(host) != B or min(host) < 0 or max(host) > S:
                raise _C.F5EError(f"Whisper.{name}: lens must be {B} values in [0, {S}]; got {host}")
            lens = torch.tensor(host, dtype=I32).to(wav.device)
        elif lens is not None and (lens.dtype != I32 or lens.shape != (B,)):
            raise _C.F5EError(f"Whisper.{name}: lens must be i32 [{B}] (got {lens.dtype} {tuple(lens.shape)})")
        return wav.contiguous(), lens

    @torch.no_grad()
    def features(self, wav: Tensor, lens=None) -> Tensor:
        """wav f32 [B, S] at 16 kHz on the GPU -> the extractor's features, channels-last: f32 [B, 2 * max_source_positions,
        num_mel_bins].  Rows are zero-padded (or cut) to the chunk length."""
        wav, lens = self._check_audio(wav, lens, "features")
        fd = self._fold()
        return ops.whisper_logmel(wav, lens, fd["window"], fd["twiddle"], fd["fb"], self.n_frames)

    @torch.no_grad()
    def encode_features(self, feats: Tensor) -> Tensor:
        """feats f32 [B, T, num_mel_bins] (channels-last, T = 2 * max_source_positions) -> the encoder's last hidden state f32
        [B, T / 2, d_model]."""
        cfg, fd = self.cfg, self._fold()
        B, T, M = feats.shape
        D, Tp = cfg.d_model, cfg.max_source_positions
        if T != 2 * Tp or M != cfg.num_mel_bins or feats.dtype != F32 or not feats.is_cuda:
            raise _C.F5EError(f"Whisper.encode_features: feats must be f32 [B, {2 * Tp}, {cfg.num_mel_bins}] on the GPU")
        dev = feats.device
        col1 = ops.im2col(feats.contiguous(), torch.empty(B, T, 3 * M, dtype=F32, device=dev), 3, 1)
        h1 = torch.empty(B * T, D, dtype=F32, device=dev)
        _gemm(col1.view(B * T, 3 * M), fd["c1_w"], fd["c1_b"], out=h1, act=ops.ACT_GELU_ERF)
        col2 = ops.im2col(h1.view(B, T, D), torch.empty(B, T, 3 * D, dtype=F32, device=dev), 3, 1)
        x = torch.empty(B * Tp, D, dtype=F32, device=dev)
        # stride 2: output frame t reads im2col row 2 t (T is even, so this holds across the rows of a batch): lda doubled
        _gemm(torch.as_strided(col2, (B * Tp, 3 * D), (6 * D, 1)), fd["c2_w"], fd["c2_b"], out=x, act=ops.ACT_GELU_ERF,
              addend=fd["enc_pos"])
        del col1, h1, col2
        M_ = B * Tp
        z = lambda n: torch.empty(M_, n, dtype=F32, device=dev)   # noqa: E731
        bufs, H = (z(D), z(3 * D), z(D), None, z(cfg.encoder_ffn_dim)), cfg.encoder_attention_heads

        def self_attn(_W, _xn, qkv, ao):
            ops.mha_f32(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], H, (D // H) ** -0.5, B=B, out=ao)

        for W in fd["enc"]:
            layer(x, x, W, bufs, pre_norm=True, act=ops.ACT_GELU_ERF, eps=1e-5, self_attn=self_attn, gemm=_gemm)
        ops.layernorm(x, x, *fd["enc_ln"], eps=1e-5)
        return x.view(B, Tp, D)

    @torch.no_grad()
    def cross_kv(self, enc_out: Tensor, out: Optional[Sequence[Tensor]] = None) -> List[Tuple[Tensor, Tensor]]:
        """Every decoder layer's cross keys and values, once per utterance: views [B, Tp, D] of one [B, Tp, 2 D] buffer each.
        ``out``: one contiguous f32 [B, Tp, 2 D] buffer per layer to project into (the storage of a captured step's state, so
        that nothing is copied afterwards); None: fresh buffers, as always."""
        fd = self._fold()
        B, Tp, D = enc_out.shape
        if out is not None and (len(out) != len(fd["dec"]) or any(tuple(b.shape) != (B, Tp, 2 * D) or b.dtype != F32 or
                                                                  not b.is_contiguous() for b in out)):
            raise _C.F5EError(f"Whisper.cross_kv: out must be {len(fd['dec'])} contiguous f32 buffers [{B}, {Tp}, {2 * D}]")
        res = []
        for i, p in enumerate(fd["dec"]):
            kv = torch.empty(B * Tp, 2 * D, dtype=F32, device=enc_out.device) if out is None else out[i].view(B * Tp, 2 * D)
            _gemm(enc_out.view(B * Tp, D), *p.xkv, out=kv)
            kv = kv.view(B, Tp, 2 * D)
            res.append((kv[..., :D], kv[..., D:]))
        return res

    @torch.no_grad()
    def encode(self, wav: Tensor, lens=None) -> List[Tuple[Tensor, Tensor]]:
        """wav f32 [B, S] at 16 kHz on the GPU, lens samples per row -> (K, V) per decoder layer, f32 [B, Tp, D] views."""
        return self.cross_kv(self.encode_features(self.features(wav, lens)))

    # ---- decoder ---------------------------------------------------------------------------------------------------------------
    def _dec_state(self, R: int, Umax: int, dev) -> dict:
        cfg = self.cfg
        D, V = cfg.d_model, cfg.vocab_size
        Vp = (V + 3) // 4 * 4
        z = lambda *s: torch.empty(*s, dtype=F32, device=dev)   # noqa: E731
        st = dict(x=z(R, 1, D), xn=z(R, D), qkv=z(R, 3 * D), ao=z(R, D), q=z(R, D), ff=z(R, cfg.decoder_ffn_dim),
                  logits=z(R, Vp)[:, :V], caches=[(z(R, Umax, D), z(R, Umax, D)) for _ in range(cfg.decoder_layers)])
        # the attention launches of ``layer``, built once per state; ``_dec_step`` sets in ``at`` what a step (p, anc, kv, align)
        # and a layer (i) change
        H, caches, align_of = cfg.decoder_attention_heads, st["caches"], self._fold()["align"]
        scale, at = (D // H) ** -0.5, SimpleNamespace(i=0, p=0, anc=None, kv=None, align=None, begin=None)

        def self_attn(_W, _xn, qkv, ao):
            kc, vc = caches[at.i]
            ops.attn_decode_f32(qkv, kc, vc, at.p, H, scale, anc=at.anc, out=ao, begin=at.begin)

        def cross_attn(_W, q, ao):
            (K, Vv), align = at.kv[at.i], at.align
            ops.cross_attn_decode_f32(q, K, Vv, H, scale, rows_per_utt=R // K.shape[0], out=ao)
            if align is not None:
                for s0, heads in align_of.get(at.i, ()):
                    ops.cross_attn_probs_f32(q, K, heads, H, scale, align[0][:, s0:s0 + heads.shape[0], align[1]],
                                             rows_per_utt=R // K.shape[0], m_len=align[2])
        st["layer"] = (at, (st["xn"], st["qkv"], st["ao"], st["q"], st["ff"]), self_attn, cross_attn)
        return st

    def _dec_step(self, st: dict, kv: List[Tuple[Tensor, Tensor]], last: Tensor, p: int, want_logits: bool,
                  anc: Optional[Tensor] = None, align: Optional[Tuple[Tensor, int, Tensor]] = None,
                  begin: Optional[Tensor] = None) -> Optional[Tensor]:
        """Feeds the tokens ``last`` i32 [R] at position p through the cached decoder; -> logits f32 [R, V] of position p + 1.
        ``anc`` i32 [R, >= p]: the beam's ancestry table, followed by every layer (None: a row reads its own cache).
        ``align`` = (probs f32 [R, heads, N, ld], t, m_len i32 [B]): the layers that own an alignment head also write those
        heads' cross-attention probabilities of this position to probs[:, :, t, :m_len] (an extra launch; nothing else changes).
        ``begin`` i32 [R] (None: the launches as they always were): row r is left-padded by begin[r] positions, so it stands at
        position p - begin[r] of the position table and reads the cached positions begin[r] .. p."""
        cfg, fd = self.cfg, self._fold()
        R, D = last.shape[0], cfg.d_model
        x3, xn, (at, bufs, self_attn, cross_attn) = st["x"], st["xn"], st["layer"]
        at.p, at.anc, at.kv, at.align, at.begin = p, anc, kv, align, begin
        if begin is None and fd["emb"].dtype == F32:
            ops.text_gather(last.view(R, 1), fd["emb"], fd["dec_pos"][p:p + 1], None, x3)
        else:                         # a 16-bit table without padding: the same sum, emb[last] + pos[p]
            _embed(last.view(R, 1), fd["emb"], fd["dec_pos"], x3, p, begin)
        x = x3.view(R, D)
        for i, W in enumerate(fd["dec"]):
            at.i = i
            layer(x, x, W, bufs, pre_norm=True, act=ops.ACT_GELU_ERF, eps=1e-5, self_attn=self_attn, cross_attn=cross_attn,
                  gemm=_gemm)
        if not want_logits:
            return None
        ops.layernorm(x, xn, *fd["dec_ln"], eps=1e-5)
        return _gemm(xn, fd["emb"], None, out=st["logits"])

    @torch.no_grad()
    def decoder_prefill(self, st: dict, kv: List[Tuple[Tensor, Tensor]], ids, begin: Optional[Tensor] = None,
                        want: Sequence[int] = ()) -> Optional[Tensor]:
        """Feeds positions 0 .. U0 - 1 of ``ids`` i32 [R, U0] through the decoder in ONE pass per layer: the
        embedding is f5e_whisper_embed, every projection one f5e_gemm_f32 over the R * U0 rows, the self-attention
        f5e_attn_prefill_f32 (which files the keys and values in slots 0 .. U0 - 1 of the caches of ``st``, as U0 single steps
        would have), the cross-attention f5e_mha_f32 with U0 queries per row.  -> logits f32 [R, len(want), V] of the positions
        listed in ``want`` (the vocabulary GEMM runs for those rows alone), or None when none is wanted.
        ``begin`` i32 [R] on the device: row r is left-padded by begin[r] positions (they are fed, filed and never read).
        A state of R * K rows (beam search) takes the R prompts into the FIRST row of each group of K; the caller points the
        ancestry table there.  ``ids`` given as a list is checked against the vocabulary here; a device tensor is clamped."""
        cfg, fd = self.cfg, self._fold()
        if not isinstance(ids, Tensor):
            host = np.asarray(ids, dtype=np.int64)
            if host.ndim != 2 or host.size == 0 or host.min() < 0 or host.max() >= cfg.vocab_size:
                raise _C.F5EError(f"Whisper.decoder_prefill: ids must be [R, U0] ids in [0, {cfg.vocab_size}) "
                                  f"(got shape {host.shape}, range {host.min() if host.size else 0} .. {host.max() if host.size else 0})")
            ids = torch.from_numpy(host)
        if ids.ndim != 2 or ids.shape[0] < 1 or ids.shape[1] < 1:
            raise _C.F5EError(f"Whisper.decoder_prefill: ids must be [R, U0] with U0 >= 1 (got shape {tuple(ids.shape)})")
        R, U0 = ids.shape
        kc0 = st["caches"][0][0]
        Rs, Umax, D = kc0.shape
        B, dev = kv[0][0].shape[0], kc0.device
        want = [int(w) for w in want]
        if Rs % R or R % B or U0 > Umax or any(not 0 <= w < U0 for w in want):
            raise _C.F5EError(f"Whisper.decoder_prefill: {R} prompts of {U0} tokens do not fit a state of {Rs} rows and {Umax} "
                              f"positions over {B} utterances (or a wanted position of {want} lies outside the prompt)")
        if begin is not None and (not isinstance(begin, Tensor) or begin.shape != (R,) or begin.dtype != I32 or not begin.is_cuda):
            raise _C.F5EError(f"Whisper.decoder_prefill: begin must be i32 [{R}] on the device")
        ids = ids.to(device=dev, dtype=I32).contiguous()
        K, H, M = Rs // R, cfg.decoder_attention_heads, R * U0
        scale, at = (D // H) ** -0.5, SimpleNamespace(i=0)
        z = lambda n: torch.empty(M, n, dtype=F32, device=dev)   # noqa: E731
        x = _embed(ids, fd["emb"], fd["dec_pos"], torch.empty(R, U0, D, dtype=F32, device=dev), 0, begin).view(M, D)
        bufs = (z(D), z(3 * D), z(D), z(D), z(cfg.decoder_ffn_dim))

        def self_attn(_W, _xn, qkv, ao):
            kc, vc = st["caches"][at.i]
            ops.attn_prefill_f32(qkv, kc[::K], vc[::K], U0, H, scale, begin=begin, out=ao)

        def cross_attn(_W, q, ao):                       # the R / B rows of an utterance are (R / B) * U0 queries on its keys
            Kx, Vx = kv[at.i]
            ops.mha_f32(q, Kx.view(-1, D), Vx.view(-1, D), H, scale, B=B, out=ao)

        for i, W in enumerate(fd["dec"]):
            at.i = i
            layer(x, x, W, bufs, pre_norm=True, act=ops.ACT_GELU_ERF, eps=1e-5, self_attn=self_attn, cross_attn=cross_attn,
                  gemm=_gemm)
        if not want:
            return None
        V = cfg.vocab_size
        rows = x.view(R, U0, D)[:, want].reshape(R * len(want), D)
        ops.layernorm(rows, rows, *fd["dec_ln"], eps=1e-5)
        logits = torch.empty(R * len(want), (V + 3) // 4 * 4, dtype=F32, device=dev)[:, :V]
        return _gemm(rows, fd["emb"], None, out=logits).view(R, len(want), V)

    @torch.no_grad()
    def decoder_append(self, st: dict, kv: List[Tuple[Tensor, Tensor]], ids: Tensor, p0: int, begin: Optional[Tensor] = None,
                       want: Optional[Sequence[int]] = None) -> Optional[Tensor]:
        """Feeds ``ids`` i32 [R, U] on the device at positions p0 .. p0 + U - 1 BEHIND what the caches of ``st`` hold, in one pass
        per layer (the verify pass of assisted generation): ``decoder_prefill``'s body at p0, with
        f5e_attn_append_f32 for the self-attention (cached positions begin[r] .. p0 - 1 from the caches, the new ones from the
        projection; slots p0 .. p0 + U - 1 are filed) and, while R * U <= 16 rows, f5e_gemm_f32_skinny for the projections, the
        feed-forward and the vocabulary (f5e_gemm_f32 beyond; ``_append_gemm``).  The cross-attention is f5e_mha_f32 with U queries per row.
        -> logits f32 [R, len(want), V] of the positions p0 + w for w in ``want`` (None: all U), or None for an empty ``want``.
        Slots beyond p0 + U - 1 keep what they held: whatever a rejected draft left there is overwritten before it is read."""
        cfg, fd = self.cfg, self._fold()
        if not isinstance(ids, Tensor) or ids.ndim != 2 or ids.shape[0] < 1 or ids.shape[1] < 1 or not ids.is_cuda:
            raise _C.F5EError("Whisper.decoder_append: ids must be [R, U] ids with U >= 1 on the GPU; there is no CPU path")
        R, U = ids.shape
        kc0 = st["caches"][0][0]
        Rs, Umax, D = kc0.shape
        B, dev, p0 = kv[0][0].shape[0], kc0.device, int(p0)
        want = list(range(U)) if want is None else [int(w) for w in want]
        if Rs % R or R % B or p0 < 0 or p0 + U > Umax or any(not 0 <= w < U for w in want):
            raise _C.F5EError(f"Whisper.decoder_append: {R} rows of {U} tokens at position {p0} do not fit a state of {Rs} rows and "
                              f"{Umax} positions over {B} utterances (or a wanted position of {want} lies outside the {U} new ones)")
        if begin is not None and (not isinstance(begin, Tensor) or begin.shape != (R,) or begin.dtype != I32 or not begin.is_cuda):
            raise _C.F5EError(f"Whisper.decoder_append: begin must be i32 [{R}] on the device")
        ids = ids.to(I32).contiguous()
        K, H, M = Rs // R, cfg.decoder_attention_heads, R * U
        scale, at = (D // H) ** -0.5, SimpleNamespace(i=0)
        scratch = st.setdefault("append", {})             # the pass's buffers, kept per row count: a round allocates nothing
        if M not in scratch:
            z = lambda *n: torch.empty(*n, dtype=F32, device=dev)   # noqa: E731
            scratch[M] = (z(R, U, D), (z(M, D), z(M, 3 * D), z(M, D), z(M, D), z(M, cfg.decoder_ffn_dim)))
        x3, bufs = scratch[M]
        x = _embed(ids, fd["emb"], fd["dec_pos"], x3, p0, begin).view(M, D)

        def gemm(a, w, bias=None, *, out, act=ops.ACT_NONE, addend=None):
            fn = self._append_gemm(a.shape[0], w.shape[0], w.shape[1])
            if w.dtype != F32:        # the 16-bit sibling of whichever the rule chose
                fn = ops.gemm_f32_w16_skinny if fn is ops.gemm_f32_skinny else ops.gemm_f32_w16
            return fn(a, w, bias, out=out, act=act, addend=addend)

        def self_attn(_W, _xn, qkv, ao):
            kc, vc = st["caches"][at.i]
            ops.attn_append_f32(qkv, kc[::K], vc[::K], U, p0, H, scale, begin=begin, out=ao)

        def cross_attn(_W, q, ao):                       # the R / B rows of an utterance are (R / B) * U queries on its keys
            Kx, Vx = kv[at.i]
            ops.mha_f32(q, Kx.view(-1, D), Vx.view(-1, D), H, scale, B=B, out=ao)

        for i, W in enumerate(fd["dec"]):
            at.i = i
            layer(x, x, W, bufs, pre_norm=True, act=ops.ACT_GELU_ERF, eps=1e-5, self_attn=self_attn, cross_attn=cross_attn,
                  gemm=gemm)
        if not want:
            return None
        V, Mw = cfg.vocab_size, R * len(want)
        rows = x if len(want) == U and want == list(range(U)) else x.view(R, U, D)[:, want].reshape(Mw, D)
        ops.layernorm(rows, rows, *fd["dec_ln"], eps=1e-5)
        key = ("logits", Mw)
        if key not in scratch:
            scratch[key] = torch.empty(Mw, (V + 3) // 4 * 4, dtype=F32, device=dev)
        return gemm(rows, fd["emb"], None, out=scratch[key][:, :V]).view(R, len(want), V)

    @staticmethod
    def _append_gemm(M: int, N: int, K: int):
        """The GEMM a verify pass of M rows runs against an [N, K] weight: f5e_gemm_f32_skinny up to 16 rows, f5e_gemm_f32
        beyond.  Launched back to back on one cache-resident weight the two are level at the decoder's K = 1280 shapes (one
        launch latency each; the skinny one wins 3.4x at K = 5120 and 1.3x .. 1.9x on the vocabulary), but inside a pass, where
        every weight comes from HBM, sending those shapes to f5e_gemm_f32 made the pass slower, 21.5 ms against 19.7 ms (and
        23.2 ms with f5e_gemm_f32 everywhere), so no shape is routed away."""
        return ops.gemm_f32_skinny if M <= ops.SKINNY_MAX_M else ops.gemm_f32

    @torch.no_grad()
    def decoder_logits(self, kv: List[Tuple[Tensor, Tensor]], ids: Tensor, one_pass: bool = False) -> Tensor:
        """Teacher forcing through the cached step: ids i32 [B, U] on the device -> logits f32 [B, U, V] (position u predicts
        token u + 1).  ``one_pass``: through ``decoder_prefill`` instead (the same numbers up to fp32 summation order)."""
        B, U = ids.shape
        if U > self.cfg.max_target_positions:
            raise _C.F5EError(f"Whisper.decoder_logits: {U} tokens exceed max_target_positions = {self.cfg.max_target_positions}")
        st = self._dec_state(B, U, ids.device)
        if one_pass:
            return self.decoder_prefill(st, kv, ids, want=range(U)).contiguous()
        out = torch.empty(B, U, self.cfg.vocab_size, dtype=F32, device=ids.device)
        ids = ids.to(I32)
        for p in range(U):
            out[:, p] = self._dec_step(st, kv, ids[:, p].contiguous(), p, True)
        return out

    def prompt_ids(self, language: str, task: str = "transcribe", timestamps: bool = False) -> List[int]:
        """``<|startoftranscript|> <|lang|> <|task|> <|notimestamps|>``: what the reference's forced_decoder_ids produce.
        ``timestamps``: without the last token (the model then emits timestamp tokens)."""
        cfg = self.cfg
        if not language:
            raise _C.F5EError("Whisper: language is required (language detection is out of scope)")
        code = LANGUAGE_NAMES.get(language.lower(), language.lower())
        key = code if code.startswith("<|") else f"<|{code}|>"
        if key not in cfg.lang_to_id:
            raise _C.F5EError(f"Whisper: language {language!r} is not in generation_config.lang_to_id "
                              f"({', '.join(sorted(cfg.lang_to_id)[:8])}, ...)")
        if task not in cfg.task_to_id:
            raise _C.F5EError(f"Whisper: task {task!r} is not in generation_config.task_to_id ({sorted(cfg.task_to_id)})")
        if cfg.no_timestamps_token_id is None:
            raise _C.F5EError("Whisper: generation_config has no no_timestamps_token_id")
        ids = [cfg.decoder_start_token_id, cfg.lang_to_id[key], cfg.task_to_id[task], cfg.no_timestamps_token_id]
        return ids[:3] if timestamps else ids

    def _prompt_rows(self, prompt, B: int, dev) -> Tensor:
        """One prompt for all rows (a sequence of ids) or one per row ([B, n0], equal lengths) -> i32 [B, n0] on the device."""
        t = prompt if isinstance(prompt, Tensor) else torch.tensor(np.asarray(prompt, dtype=np.int64))
        t = t.to(device=dev, dtype=I32)
        if t.ndim == 1:
            t = t[None, :].expand(B, -1)
        if t.ndim != 2 or t.shape[0] != B:
            raise _C.F5EError(f"Whisper.generate: the prompt must be n0 ids or [{B}, n0] ids (got shape {tuple(t.shape)})")
        return t.contiguous()

    @torch.no_grad()
    def detect_language(self, kv: List[Tuple[Tensor, Tensor]]) -> Tensor:
        """-> i32 [B]: the language id of every utterance, ``transformers``' ``detect_language``: one cached step on
        ``<|startoftranscript|>``, then the first maximum over the ids of ``lang_to_id`` (f5e_greedy_pick with every other class
        suppressed)."""
        cfg, fd = self.cfg, self._fold()
        if fd["not_lang"] is None:
            raise _C.F5EError("Whisper.detect_language: generation_config has no lang_to_id")
        B, dev = kv[0][0].shape[0], kv[0][0].device
        tokens = torch.full((B, 2), cfg.decoder_start_token_id, dtype=I32, device=dev)
        last, done = tokens[:, 0].clone(), torch.zeros(B, dtype=I32, device=dev)
        logits = self._dec_step(self._dec_state(B, 1, dev), kv, last, 0, True)
        ops.greedy_pick(logits, tokens, last, done, torch.zeros(1, dtype=I32, device=dev), 0, cfg.eos_token_id, suppress=fd["not_lang"])
        return last

    def _prompts(self, kv, language, task: str, timestamps: bool):
        """The prompt of ``generate``: a list of ids for a named language, i32 [B, n0] with the detected ids for None."""
        if language is not None:
            return self.prompt_ids(language, task, timestamps)
        if not self.cfg.lang_to_id:
            raise _C.F5EError("Whisper: language = None asks for detection, but generation_config has no lang_to_id")
        ids = self.prompt_ids(sorted(self.cfg.lang_to_id)[0], task, timestamps)      # checks task and no_timestamps_token_id
        rows = torch.tensor(ids, dtype=I32, device=kv[0][0].device)[None, :].repeat(kv[0][0].shape[0], 1)
        rows[:, 1] = self.detect_language(kv)
        return rows

    # ---- token timestamps (alignment heads and DTW) ------------------------------------------------------------------
    @torch.no_grad()
    def alignment_probs(self, kv: List[Tuple[Tensor, Tensor]], tokens: Tensor, n, frames, n0: int,
                        include_last: bool = False) -> Tuple[Optional[Tensor], Tensor, Tensor]:
        """The teacher-forced pass of ``token_timestamps``: -> (probs f32 [B, heads, N_cap, ld] or None when no row has a fed
        position, n_rows i32 [B], m_len i32 [B]).  probs[b, s, t, :m_len[b]] for t < n_rows[b] is the cross-attention of alignment
        head s for the token at position n0 + t, softmax over all encoder keys; everything else of the buffer is zero or
        belongs to positions beyond the row's own.  One host read (n), to size the buffer by the longest hypothesis."""
        cfg = self.cfg
        if not cfg.alignment_heads:
            raise _C.F5EError("Whisper.token_timestamps: this model has no alignment_heads (generation_config.json); token "
                              "timestamps are not available for it")
        if not isinstance(tokens, Tensor) or tokens.ndim != 2 or not tokens.is_cuda:
            raise _C.F5EError("Whisper.token_timestamps: tokens must be an integer tensor [B, U] on the GPU; there is no CPU path")
        B, U = tokens.shape
        dev, Tp = tokens.device, cfg.max_source_positions
        n_host = [int(v) for v in (n.tolist() if isinstance(n, Tensor) else n)]
        fr = frames.tolist() if isinstance(frames, Tensor) else frames
        fr_host = [int(fr)] * B if isinstance(fr, (int, float)) else [int(v) for v in fr]
        n0 = int(n0)
        if kv[0][0].shape[0] != B or len(n_host) != B or len(fr_host) != B or n0 < 1 or min(n_host) < n0 or max(n_host) > U:
            raise _C.F5EError(f"Whisper.token_timestamps: {B} rows need {B} lengths in [{n0}, {U}] and {B} frame counts "
                              f"(got n = {n_host}, frames = {fr_host}, {kv[0][0].shape[0]} utterances of keys)")
        rows = [max(v - n0 - (0 if include_last else 1), 0) for v in n_host]
        N_cap, cols = max(rows), [min(max(f // 2, 1), Tp) for f in fr_host]
        n_rows = torch.tensor(rows, dtype=I32).to(dev)
        m_len = torch.tensor(cols, dtype=I32).to(dev)
        if N_cap == 0:
            return None, n_rows, m_len
        if n0 + N_cap > cfg.max_target_positions or N_cap > ops.DTW_MAX_N:
            raise _C.F5EError(f"Whisper.token_timestamps: {n0} + {N_cap} positions exceed max_target_positions = "
                              f"{cfg.max_target_positions} (or the {ops.DTW_MAX_N} rows of the DTW kernel)")
        probs = torch.zeros(B, len(cfg.alignment_heads), N_cap, (max(cols) + 3) // 4 * 4, dtype=F32, device=dev)
        ids = tokens.to(I32)
        st = self._dec_state(B, n0 + N_cap, dev)
        for p in range(n0 + N_cap):
            self._dec_step(st, kv, ids[:, p].contiguous(), p, False, align=(probs, p - n0, m_len) if p >= n0 else None)
        return probs, n_rows, m_len

    @torch.no_grad()
    def token_timestamps(self, kv: List[Tuple[Tensor, Tensor]], tokens: Tensor, n, frames, n0: int,
                         include_last: bool = False) -> Tensor:
        """Teacher-forced token times: tokens i32 [B, U] on the device (row b holds n[b] tokens, n0 of them the prompt), ``frames``
        mel frames per utterance (samples // 160; an int, a list or a tensor) -> times f32 [B, U] in seconds: zeros for the
        prompt, 0.02 x the encoder position at which the DTW path over the alignment heads' cross-attention enters the token's
        row for positions n0 .. n[b] - 2, position n[b] - 1 repeating n[b] - 2 (the last token is never fed, as in
        ``transformers``), zeros beyond.  ``include_last``: the last token is fed too and takes its own row (OpenAI's rule).
        The given tokens go through the cached step; the layers that own an alignment head write those heads' probabilities
        (f5e_cross_attn_probs_f32), then f5e_dtw_cost_f32 and f5e_dtw_path.  Row b of a ragged batch equals its own B = 1 run."""
        probs, n_rows, m_len = self.alignment_probs(kv, tokens, n, frames, n0, include_last)
        B, U = tokens.shape
        times = torch.zeros(B, U, dtype=F32, device=tokens.device)
        if probs is None:
            return times
        N_cap, n0 = probs.shape[2], int(n0)
        cost = ops.dtw_cost_f32(probs, n_rows, m_len, self.cfg.median_filter_width)
        first = ops.dtw_path(cost, n_rows, m_len)
        # float32(frame * 0.02 in float64): the reference's own rounding
        sec = (first.clamp(min=0).to(torch.float64) * 0.02).to(F32)
        fed = torch.arange(N_cap, device=tokens.device)[None, :] < n_rows[:, None]
        times[:, n0:n0 + N_cap] = torch.where(fed, sec, torch.zeros_like(sec))
        if not include_last:
            bi = torch.nonzero(n_rows > 0)[:, 0]
            last = n0 + n_rows[bi].to(torch.int64)
            times[bi, last] = times[bi, last - 1]
        return times

    # ---- the captured step: one decode step as a hipGraph, replayed per token -----------------------------------------
    @staticmethod
    def _check_step_graph(step_graph, step_gemm, beam_size, return_beams, assistant, return_token_timestamps) -> bool:
        """-> whether the picks are replayed from a captured step; refusals by name, before any launch."""
        if step_gemm not in ("f32", "skinny"):
            raise _C.F5EError(f"Whisper.generate: step_gemm = {step_gemm!r} must be 'f32' or 'skinny'")
        if not isinstance(step_graph, bool):
            raise _C.F5EError(f"Whisper.generate: step_graph = {step_graph!r} must be a bool")
        if not step_graph:
            if step_gemm != "f32":
                raise _C.F5EError(f"Whisper.generate: step_gemm = {step_gemm!r} needs step_graph = True (it chooses the GEMM of "
                                  "the captured step; the eager step keeps f5e_gemm_f32)")
            return False
        if int(beam_size) != 1 or return_beams:
            raise _C.F5EError(f"Whisper.generate: step_graph with beam_size = {beam_size} / return_beams is out of scope (the beam's "
                              "two table pairs alternate per step: it needs a two-step graph and device-position beam kernels)")
        if assistant is not None:
            raise _C.F5EError("Whisper.generate: step_graph with assistant is out of scope (assisted generation from a graph is "
                              "not built)")
        if return_token_timestamps:
            raise _C.F5EError("Whisper.generate: step_graph with return_token_timestamps is out of scope (the teacher-forced "
                              "pass of token_timestamps writes alignment rows at a host position)")
        return True

    def _step_state(self, B: int, kind: str, padded: bool, step_gemm: str, Tp: int, dev) -> SimpleNamespace:
        """The decode state a captured step runs on, cached on the folded weights (so a reload or a move drops it with its
        graph) under (rows, pick kind, begin present, GEMM, cross positions, device): an LRU of at most ``STEP_STATES``.  The
        state owns every buffer the graph's kernels touch: the self-attention caches, ``max_target_positions`` deep, its own
        cross keys / values (``_step_load`` copies a call's into them), tokens, last, done, alive, sum_logp, begin, row_key,
        serial, the step's scratch and logits, the step record and the skinny GEMM's workspace."""
        if step_gemm == "skinny" and B > ops.SKINNY_MAX_M:
            raise _C.F5EError(f"Whisper.generate: step_gemm = 'skinny' is built for at most {ops.SKINNY_MAX_M} rows (got {B}); "
                              "step_gemm = 'f32' takes the rest")
        cfg, fd = self.cfg, self._fold()
        cache = fd.setdefault("step_states", {})
        # the GEMM field names the weight mode too where there is one: "skinny+fp16" captures the _w16 launches
        key = (B, kind, padded, step_gemm if self.wdtype is None else f"{step_gemm}+{self.weights}", Tp, str(dev))
        S = cache.pop(key, None)
        if S is None:
            D, P, FF, V = cfg.d_model, cfg.max_target_positions, cfg.decoder_ffn_dim, cfg.vocab_size
            zi = lambda *s: torch.zeros(*s, dtype=I32, device=dev)   # noqa: E731
            S = SimpleNamespace(key=key, kind=kind, R=B, graph=None, captures=0, replays=0, st=self._dec_state(B, P, dev), tokens=zi(B, P), last=zi(B),
                                done=zi(B), alive=zi(1), sum_logp=torch.zeros(B, dtype=F32, device=dev), row_key=zi(B),
                                serial=zi(B), begin=zi(B) if padded else None, rec=zi(ops.STEP_REC_WORDS),
                                xkv=[torch.empty(B, Tp, 2 * D, dtype=F32, device=dev) for _ in fd["dec"]], gemm=_gemm,
                                stream=torch.cuda.Stream(device=dev))
            S.kv = [(b[..., :D], b[..., D:]) for b in S.xkv]
            H, scale, at = cfg.decoder_attention_heads, (D // cfg.decoder_attention_heads) ** -0.5, S.st["layer"][0]

            def self_attn(_W, _xn, qkv, ao):
                kc, vc = S.st["caches"][at.i]
                ops.attn_decode_dev_f32(qkv, kc, vc, S.rec, H, scale, out=ao, begin=S.begin)
            S.self_attn = self_attn
            if step_gemm == "skinny":      # its scratch belongs to the state: the default one is kept per stream, allocated on use
                need = max(ops._skinny_need(n, k, dev) for n, k in ((3 * D, D), (D, D), (FF, D), (D, FF), (V, D)))
                ws = torch.empty(max(need, 16) // 4, dtype=F32, device=dev)

                def gemm(a, w, bias=None, *, out, act=ops.ACT_NONE, addend=None):
                    return _gemm_skinny(a, w, bias, out=out, act=act, addend=addend, workspace=ws)
                S.gemm, S.ws = gemm, ws
        cache[key] = S                                          # most recently used last
        while len(cache) > STEP_STATES:
            old = cache.pop(next(iter(cache)))
            if old.graph is not None:                           # its launches may still be queued: parked behind an event
                old.graph.retire()
        ops.Graph.reap()
        return S

    @staticmethod
    def _step_load(S: SimpleNamespace, kv: List[Tuple[Tensor, Tensor]]) -> None:
        """A call's cross keys / values into the state's own storage, whose addresses the graph holds: one device copy per
        layer when k | v are the two halves of one buffer (what ``cross_kv`` returns), two otherwise, none when they ARE the
        state's storage (``cross_kv(enc, out=S.xkv)``, what ``generate`` does)."""
        B, Tp, D2 = S.xkv[0].shape
        if len(kv) != len(S.xkv):
            raise _C.F5EError(f"Whisper.generate: {len(kv)} layers of cross keys / values for {len(S.xkv)} decoder layers")
        for buf, (k, v) in zip(S.xkv, kv):
            if tuple(k.shape) != (B, Tp, D2 // 2) or tuple(v.shape) != tuple(k.shape) or k.dtype != F32 or v.dtype != F32:
                raise _C.F5EError(f"Whisper.generate: cross keys / values must be f32 [{B}, {Tp}, {D2 // 2}] per layer")
            if k.data_ptr() == buf.data_ptr() and v.data_ptr() == buf.data_ptr() + 2 * D2 and k.stride() == (Tp * D2, D2, 1) and \
                    v.stride() == k.stride():
                continue
            if k.stride() == (Tp * D2, D2, 1) and v.stride() == k.stride() and v.data_ptr() == k.data_ptr() + 2 * D2 and \
                    k.untyped_storage().data_ptr() == v.untyped_storage().data_ptr():
                buf.copy_(torch.as_strided(k, (B, Tp, D2), k.stride()))
            else:
                buf[..., :D2 // 2].copy_(k)
                buf[..., D2 // 2:].copy_(v)

    def _step_dev(self, S: SimpleNamespace, ts: bool) -> None:
        """The launches of ONE pick step on the state ``S`` with the position read from ``S.rec``: ``_dec_step`` and the pick
        with the device-position kernels (csrc/whisper_step.hip) in the place of the host-position ones, nothing else.  No
        allocation, no copy, no host read: this is what the graph captures."""
        cfg, fd = self.cfg, self._fold()
        R, D, eos = S.R, cfg.d_model, cfg.eos_token_id
        st = S.st
        at, bufs, _, cross_attn = st["layer"]
        at.anc, at.kv, at.align, at.begin = None, S.kv, None, S.begin
        (ops.whisper_embed_dev if fd["emb"].dtype == F32 else ops.whisper_embed_w16_dev)(S.last, fd["emb"], fd["dec_pos"], st["x"],
                                                                                         S.rec, S.begin)
        x = st["x"].view(R, D)
        for i, W in enumerate(fd["dec"]):
            at.i = i
            layer(x, x, W, bufs, pre_norm=True, act=ops.ACT_GELU_ERF, eps=1e-5, self_attn=S.self_attn, cross_attn=cross_attn,
                  gemm=S.gemm)
        ops.layernorm(x, st["xn"], *fd["dec_ln"], eps=1e-5)
        S.gemm(st["xn"], fd["emb"], None, out=st["logits"])
        kw = dict(suppress=fd["suppress"], begin_suppress=fd["begin_suppress"])
        if S.kind.startswith("sample"):
            ops.whisper_sample_pick_dev(st["logits"], S.tokens, S.last, S.done, S.alive, S.sum_logp, S.rec, eos,
                                        cfg.timestamp_begin - 1 if ts else None, S.row_key, S.serial,
                                        max_initial=cfg.max_initial_timestamp_index if ts else None, **kw)
        elif ts:
            ops.whisper_ts_pick_dev(st["logits"], S.tokens, S.last, S.done, S.alive, S.sum_logp, S.rec, eos, cfg.timestamp_begin - 1,
                                    max_initial=cfg.max_initial_timestamp_index, **kw)
        else:
            ops.greedy_pick_dev(st["logits"], S.tokens, S.last, S.done, S.alive, S.rec, eos, **kw)

    def _step_capture(self, S: SimpleNamespace, ts: bool) -> None:
        """Captures ``_step_dev`` on the state's side stream: one stream, a linear chain.  Capturing executes nothing, so it
        needs no ordering against the caller's stream, where the graph is then launched."""
        g = ops.Graph()
        with torch.cuda.stream(S.stream):
            g.begin()
            try:
                self._step_dev(S, ts)
            finally:
                g.end()
        S.graph = g

    def _frames_of(self, wav: Tensor, lens) -> List[int]:
        """Mel frames of every row of a batch: samples // hop, at most the chunk."""
        B, S = wav.shape
        host = [S] * B if lens is None else [int(v) for v in (lens.tolist() if isinstance(lens, Tensor) else lens)]
        return [min(min(v, S) // HOP, self.n_frames) for v in host]

    @torch.no_grad()
    def generate_from_kv(self, kv: List[Tuple[Tensor, Tensor]], prompt: Sequence[int], max_new_tokens: Optional[int] = None,
                         sync_every: int = 8, beam_size: int = 1, length_penalty: float = 1.0, return_beams: bool = False,
                         return_token_timestamps: bool = False, frames=None, return_timestamps: bool = False,
                         stats: Optional[dict] = None, temperature: float = 0.0, seed: int = 0, row_key: Optional[Tensor] = None,
                         serial: Optional[Tensor] = None, begin: Optional[Tensor] = None, prefill: bool = False,
                         assistant: Optional[tuple] = None, num_assistant_tokens: int = 5, *, step_graph: bool = False,
                         step_gemm: str = "f32"):
        """``generate`` from the cross keys / values.  ``prompt``: ids for all rows, or [B, n0] ids.  ``return_token_timestamps``:
        one more item at the end, the times f32 [B, U] of the returned best hypothesis = ``token_timestamps`` on the returned
        tokens (a teacher-forced pass after the search, greedy or beam); ``frames``: mel frames per utterance (None: the whole
        chunk).  ``return_timestamps``: the picks follow Whisper's timestamp rules (f5e_whisper_ts_pick /
        f5e_whisper_beam_step_ts; the prompt must not end in <|notimestamps|>).  ``stats``: a dict that receives
        ``no_speech_logp`` f32 [B] (the log-probability of <|nospeech|> after <|startoftranscript|>) and ``sum_logp`` f32 [B]
        (ruled greedy: the sum of the picks' log-probabilities among the allowed classes; beam: the best hypothesis' score times
        its generated length).  ``temperature`` > 0: every pick is a draw from softmax(logits / temperature) over the allowed
        classes (f5e_whisper_sample_pick, with or without the timestamp rules; ``sum_logp`` is then the sum of the picks' T = 1
        log-probabilities); the noise is a function of ``seed``, the position and per row ``row_key`` (None: the row's index)
        and ``serial`` (None: 0), i32 [B] on the device, so a row's draws do not depend on its batch.
        ``prefill``: the prompt's tokens but the last go through ``decoder_prefill`` in one pass instead of one cached step
        each; the picks start at n0 as before.  ``begin`` i32 [B] on the device (or a list): row b of the [B, n0] prompt is
        left-padded by begin[b] tokens (any valid id), which it neither attends nor counts as positions, so ragged prompts
        share one n0 and a row equals its own B = 1 run.  With either, ``no_speech_logp`` is read at the prompt's
        <|startoftranscript|> (the last one of row 0; left-padding puts it in the same column for every row).  The bound
        ``max_target_positions`` counts the padded columns, so a padded row has begin[b] fewer picks than alone: with ``begin``,
        ``stats`` also receives ``at_bound`` i32 [B], non-zero for a row that was still open when the last step of the bound ran
        (only such a row can differ from its own unpadded run; ``transcribe_long`` decodes it again alone).
        ``assistant`` = (draft, draft_kv): assisted generation (speculative decoding, ``_assisted_from_kv``): ``draft``, a
        smaller ``Whisper`` with the same vocabulary, proposes up to ``num_assistant_tokens`` tokens per round from its own
        cross keys / values ``draft_kv``, and this model checks them in one pass (``decoder_append``, f5e_whisper_verify,
        f5e_whisper_accept).  Greedy only; the tokens are those of the run without an assistant, and ``stats`` also receives
        ``assistant`` = {"rounds", "drafted", "accepted"}.
        ``step_graph``: the picks are replayed from ONE decode step captured as a hipGraph: the prompt runs as
        above, then the step record (position, prompt length, seed, temperature) is written and the captured step, which reads
        and advances it on the device, is launched once per token.  The state it runs on (caches ``max_target_positions`` deep,
        its own copy of the cross keys / values, the token table) is cached on the model per (rows, pick, ``begin`` present,
        ``step_gemm``), at most ``STEP_STATES`` of them, so only the first call of a key captures; the results are fresh
        tensors.  Greedy, ruled and sampled picks, ``begin``, ``prefill`` and ``stats``, which also receives ``step_graph`` =
        {"captures", "replays"}; the step that ``no_speech_logp`` is read at stays eager.  Same bits as the eager run.
        ``step_gemm``: "f32" replays the eager step's launches; "skinny" runs the step's GEMMs through f5e_gemm_f32_skinny (at
        most 16 rows; the same numbers up to fp32 summation order).  The defaults take the launches they always took."""
        graphed = self._check_step_graph(step_graph, step_gemm, beam_size, return_beams, assistant, return_token_timestamps)
        n0 = _prompt_len(prompt)
        sample = self._check_sampling(temperature, seed, beam_size, return_beams)
        if assistant is not None:
            if not isinstance(assistant, (tuple, list)) or len(assistant) != 2:
                raise _C.F5EError("Whisper.generate: assistant must be (draft, draft_kv): a Whisper and its cross keys / values")
            self._check_assistant(assistant[0], num_assistant_tokens, beam_size, return_beams, temperature)
        sot_pos = 0
        if begin is not None or prefill:
            if return_token_timestamps:
                raise _C.F5EError("Whisper.generate: return_token_timestamps with begin / prefill is out of scope (the "
                                  "teacher-forced pass of token_timestamps feeds unpadded rows)")
            begin, sot_pos = self._check_begin(begin, prompt, kv[0][0].shape[0], n0, stats is not None)
            if int(beam_size) != 1 or return_beams:
                return self._beam_from_kv(kv, prompt, max_new_tokens, sync_every, int(beam_size), float(length_penalty),
                                          return_beams, bool(return_timestamps), stats, begin, bool(prefill), sot_pos)
        if return_token_timestamps:
            if not self.cfg.alignment_heads:
                raise _C.F5EError("Whisper.generate: return_token_timestamps needs alignment_heads in generation_config.json")
            res = self.generate_from_kv(kv, prompt, max_new_tokens, sync_every, beam_size, length_penalty, return_beams,
                                        return_timestamps=return_timestamps, stats=stats, temperature=temperature, seed=seed,
                                        row_key=row_key, serial=serial, assistant=assistant,
                                        num_assistant_tokens=num_assistant_tokens)
            times = self.token_timestamps(kv, res[0], res[1], self.n_frames if frames is None else frames, n0)
            return tuple(res) + (times,)
        if int(beam_size) != 1 or return_beams:
            if not return_timestamps and stats is None:
                return self._beam_from_kv(kv, prompt, max_new_tokens, sync_every, int(beam_size), float(length_penalty), return_beams)
            return self._beam_from_kv(kv, prompt, max_new_tokens, sync_every, int(beam_size), float(length_penalty), return_beams,
                                      bool(return_timestamps), stats)
        if assistant is not None:
            return self._assisted_from_kv(kv, prompt, max_new_tokens, bool(return_timestamps), stats, begin, bool(prefill), sot_pos,
                                          assistant[0], assistant[1], int(num_assistant_tokens))
        cfg, fd = self.cfg, self._fold()
        B = kv[0][0].shape[0]
        dev = kv[0][0].device
        ts_begin = cfg.timestamp_begin if return_timestamps else None
        Umax = cfg.max_target_positions if max_new_tokens is None else min(cfg.max_target_positions, n0 + int(max_new_tokens))
        if n0 < 1 or n0 >= Umax or sync_every < 1:
            raise _C.F5EError(f"Whisper.generate: a prompt of {n0} tokens leaves no room below {Umax} positions (or sync_every < 1)")
        eos = cfg.eos_token_id
        S = None
        if graphed:                          # the cached state's buffers in the place of fresh ones; everything else as below
            kind = ("sample" if sample else "greedy") + ("_ts" if return_timestamps else "")
            S = self._step_state(B, kind, begin is not None, step_gemm, kv[0][0].shape[1], dev)
            self._step_load(S, kv)
            kv, st, tokens, last, done, alive = S.kv, S.st, S.tokens[:, :Umax], S.last, S.done, S.alive
            tokens.fill_(eos)
            tokens[:, :n0] = self._prompt_rows(prompt, B, dev)
            last.copy_(tokens[:, 0])
            done.zero_()
            alive.fill_(B)
            sum_logp = S.sum_logp.zero_() if return_timestamps or sample else None
            if sample:
                row_key = S.row_key.copy_(torch.arange(B, dtype=I32, device=dev) if row_key is None else row_key.to(dev, I32))
                serial = S.serial.zero_() if serial is None else S.serial.copy_(serial.to(dev, I32))
            if begin is not None:
                begin = S.begin.copy_(begin)
            armed, counts = False, dict(captures=0, replays=0)
        else:
            tokens = torch.full((B, Umax), eos, dtype=I32, device=dev)
            tokens[:, :n0] = self._prompt_rows(prompt, B, dev)
            last = tokens[:, 0].clone()
            done = torch.zeros(B, dtype=I32, device=dev)
            alive = torch.full((1,), B, dtype=I32, device=dev)
            sum_logp = torch.zeros(B, dtype=F32, device=dev) if return_timestamps or sample else None
            if sample:
                row_key = torch.arange(B, dtype=I32, device=dev) if row_key is None else row_key.to(dev, I32).contiguous()
                serial = torch.zeros(B, dtype=I32, device=dev) if serial is None else serial.to(dev, I32).contiguous()
            st = self._dec_state(B, Umax, dev)
        first_p = 0
        if prefill and n0 > 1:
            first_p = n0 - 1
            logits = self.decoder_prefill(st, kv, tokens[:, :first_p].contiguous(), begin,
                                          (sot_pos,) if stats is not None and sot_pos < first_p else ())
            if logits is not None:
                stats["no_speech_logp"] = self._no_speech_logp(logits[:, 0])
            last.copy_(tokens[:, first_p])
        at_bound = None
        for p in range(first_p, Umax - 1):
            forced = p + 1 < n0
            if p == Umax - 2 and begin is not None and stats is not None:
                at_bound = 1 - done                          # rows still open when the last step of the shared bound runs
            if S is not None and not forced and not (p == sot_pos and stats is not None):
                if not armed:                # the record once per call; the step advances it on the device from here on
                    S.rec.copy_(ops.whisper_step_record(p, n0, seed if sample else 0, temperature if sample else 0.0))
                    armed = True
                    if S.graph is None:
                        self._step_capture(S, bool(return_timestamps))
                        counts["captures"] += 1
                S.graph.launch()
                counts["replays"] += 1
                if (p + 2 - n0) % sync_every == 0 and int(alive.item()) == 0:
                    break
                continue
            logits = self._dec_step(st, kv, last, p, not forced or (p == sot_pos and stats is not None), begin=begin)
            if p == sot_pos and stats is not None:
                stats["no_speech_logp"] = self._no_speech_logp(logits)
            if forced:                       # all prompt tokens but the last go through the same cached step; nothing is picked
                last.copy_(tokens[:, p + 1])
                continue
            if sample:
                ops.whisper_sample_pick(logits, tokens, last, done, alive, sum_logp, p, n0, eos,
                                        ts_begin - 1 if return_timestamps else None, float(temperature), int(seed), row_key, serial,
                                        suppress=fd["suppress"], begin_suppress=fd["begin_suppress"],
                                        max_initial=cfg.max_initial_timestamp_index if return_timestamps else None)
            elif return_timestamps:
                ops.whisper_ts_pick(logits, tokens, last, done, alive, sum_logp, p, n0, eos, ts_begin - 1, suppress=fd["suppress"],
                                    begin_suppress=fd["begin_suppress"], max_initial=cfg.max_initial_timestamp_index)
            else:
                ops.greedy_pick(logits, tokens, last, done, alive, p, eos, suppress=fd["suppress"],
                                begin_suppress=fd["begin_suppress"], first_step=p + 1 == n0)
            if (p + 2 - n0) % sync_every == 0 and int(alive.item()) == 0:
                break
        if S is not None:                    # fresh tensors, never views of the state
            S.captures, S.replays = S.captures + counts["captures"], S.replays + counts["replays"]
            tokens = tokens.clone(memory_format=torch.contiguous_format)
            sum_logp = None if sum_logp is None else sum_logp.clone()
            if stats is not None:
                stats["step_graph"] = counts
        # a finished row holds eos from its end on (done rows keep getting eos; untouched columns were eos from the start)
        gen = tokens[:, n0:]
        is_eos = gen == eos
        first = torch.where(is_eos.any(1), is_eos.to(torch.int64).argmax(1) + 1, torch.full((B,), Umax - n0, dtype=torch.int64, device=dev))
        if stats is not None:
            stats["sum_logp"] = sum_logp
            if begin is not None:
                stats["at_bound"] = torch.zeros(B, dtype=I32, device=dev) if at_bound is None else at_bound
        return tokens, (first + n0).to(I32)

    def _check_assistant(self, draft, num_assistant_tokens, beam_size, return_beams, temperature) -> None:
        """Refusals of assisted generation by name, before any launch."""
        if not isinstance(draft, Whisper):
            raise _C.F5EError(f"Whisper.generate: assistant = {type(draft).__name__} must be a Whisper model")
        if int(beam_size) != 1 or return_beams:
            raise _C.F5EError(f"Whisper.generate: assistant with beam_size = {beam_size} / return_beams is out of scope (assisted "
                              "generation is greedy: the draft proposes one continuation per row)")
        if temperature != 0:
            raise _C.F5EError(f"Whisper.generate: assistant with temperature = {temperature!r} is out of scope (speculative "
                              "sampling is not built; sampled attempts take the path without an assistant)")
        if isinstance(num_assistant_tokens, bool) or not isinstance(num_assistant_tokens, int) or num_assistant_tokens < 1:
            raise _C.F5EError(f"Whisper.generate: num_assistant_tokens = {num_assistant_tokens!r} must be an integer >= 1")
        for name in ("vocab_size", "eos_token_id", "max_target_positions", "suppress_tokens", "begin_suppress_tokens"):
            mine, theirs = getattr(self.cfg, name), getattr(draft.cfg, name)
            if (tuple(mine) != tuple(theirs)) if isinstance(mine, (tuple, list)) else (mine != theirs):
                raise _C.F5EError(f"Whisper.generate: the assistant's {name} differs from this model's ({theirs!r} vs {mine!r}); "
                                  "a draft must share the vocabulary, eos, positions and suppress lists")

    def _check_shared_encoder(self, draft: "Whisper", shares: bool, who: str) -> None:
        """A draft that reads this model's encoder output needs this model's width and encoder shape; one that encodes the
        window's features itself (``transcribe_long``) needs this model's mel bins and window."""
        names = ("d_model", "max_source_positions", "encoder_layers", "encoder_attention_heads", "encoder_ffn_dim",
                 "num_mel_bins") if shares else (("num_mel_bins", "max_source_positions") if who == "transcribe_long" else ())
        for name in names:
            if getattr(self.cfg, name) != getattr(draft.cfg, name):
                raise _C.F5EError(f"Whisper.{who}: the assistant's {name} = {getattr(draft.cfg, name)} differs from this model's "
                                  f"{getattr(self.cfg, name)}" + ("; assistant_shares_encoder needs one encoder shape" if shares else
                                                                 "; the windows' features are computed once, with this model's front-end"))

    @torch.no_grad()
    def _assisted_from_kv(self, kv, prompt, max_new_tokens, ts: bool, stats: Optional[dict], begin: Optional[Tensor], prefill: bool,
                          sot_pos: int, draft: "Whisper", dkv, N: int):
        """Greedy decoding with a draft model (``transformers``' assisted generation with a constant schedule and a confidence
        threshold of 0).  A round at position p, with U = min(N, Umax - 2 - p) (0: an ordinary step of this model):
          1. the draft catches up: the final tokens from the first position its cache does not hold to p - 1, one cached step
             each (one or two per round);
          2. the draft makes U ordinary steps from p on its own table ``hist`` (a copy of ``tokens`` up to p) with this model's
             pick kernel and rules, on its own last / done / alive scratch;
          3. this model feeds hist[:, p .. p + U] at p0 = p through ``decoder_append`` and takes the logits of all U + 1 positions;
          4. f5e_whisper_verify picks at all of them; f5e_whisper_accept keeps, per row, the picks up to the first one that
             differs from its draft, advances ALL rows by the smallest such count a (so the position stays one scalar: a row that
             keeps fewer tokens than it could is still its own greedy run), and writes tokens, last, done, sum_logp and alive
             as a single steps would have;
          5. the host reads a and the alive count (one synchronisation per round).  Cache slots of rejected drafts, this model's
             and the draft's, are overwritten before they are read.
        Both models prefill the same left-padded prompt.  The outputs are those of the path without an assistant; ``stats`` on a
        model without timestamp classes (no <|nospeech|>) carries no ``no_speech_logp`` instead of refusing, since it is also how
        the assistant's figures are returned."""
        cfg, fd = self.cfg, self._fold()
        n0 = _prompt_len(prompt)
        B, dev = kv[0][0].shape[0], kv[0][0].device
        if len(dkv) != draft.cfg.decoder_layers or dkv[0][0].shape[0] != B or dkv[0][0].shape[-1] != draft.cfg.d_model:
            raise _C.F5EError(f"Whisper.generate: the assistant's cross keys / values must be those of its {draft.cfg.decoder_layers} "
                              f"decoder layers for the same {B} utterances")
        draft._fold()
        want_ns = stats is not None and cfg.no_timestamps_token_id is not None and \
            cfg.eos_token_id <= cfg.no_timestamps_token_id < cfg.vocab_size - 1
        no_ts = cfg.timestamp_begin - 1 if ts else None
        max_initial = cfg.max_initial_timestamp_index if ts else None
        Umax = cfg.max_target_positions if max_new_tokens is None else min(cfg.max_target_positions, n0 + int(max_new_tokens))
        if n0 < 1 or n0 >= Umax:
            raise _C.F5EError(f"Whisper.generate: a prompt of {n0} tokens leaves no room below {Umax} positions")
        eos, V = cfg.eos_token_id, cfg.vocab_size
        tokens = torch.full((B, Umax), eos, dtype=I32, device=dev)
        tokens[:, :n0] = self._prompt_rows(prompt, B, dev)
        hist = tokens.clone()                                # the draft's table
        zi = lambda *s: torch.zeros(*s, dtype=I32, device=dev)   # noqa: E731
        last, done, sync = tokens[:, 0].clone(), zi(B), zi(2)
        alive, adv = sync[0:1], sync[1:2]                    # read together, once per round
        alive.fill_(B)
        sum_logp = torch.zeros(B, dtype=F32, device=dev) if ts else None
        dlast, ddone, dalive = last.clone(), zi(B), zi(1)
        dsum = torch.zeros(B, dtype=F32, device=dev) if ts else None
        out = {u: (torch.empty(B, u + 1, dtype=I32, device=dev), torch.empty(B, u + 1, dtype=F32, device=dev))
               for u in range(1, N + 1)}                     # cand, logp per draft length (only the last rounds are shorter)
        st, dst = self._dec_state(B, Umax, dev), draft._dec_state(B, Umax, dev)

        def pick(logits, table, last_, done_, alive_, sum_, p):
            if ts:
                ops.whisper_ts_pick(logits, table, last_, done_, alive_, sum_, p, n0, eos, no_ts, suppress=fd["suppress"],
                                    begin_suppress=fd["begin_suppress"], max_initial=max_initial)
            else:
                ops.greedy_pick(logits, table, last_, done_, alive_, p, eos, suppress=fd["suppress"],
                                begin_suppress=fd["begin_suppress"], first_step=p + 1 == n0)

        p = 0
        if prefill and n0 > 1:
            p = n0 - 1
            ids = tokens[:, :p].contiguous()
            logits = self.decoder_prefill(st, kv, ids, begin, (sot_pos,) if want_ns and sot_pos < p else ())
            if logits is not None:
                stats["no_speech_logp"] = self._no_speech_logp(logits[:, 0])
            draft.decoder_prefill(dst, dkv, ids, begin)
            last.copy_(tokens[:, p])
        dnext = p                                            # the first position the draft's cache does not hold
        while p + 1 < n0:                                    # the forced tokens: the cached step, nothing is picked
            logits = self._dec_step(st, kv, last, p, p == sot_pos and want_ns, begin=begin)
            if p == sot_pos and want_ns:
                stats["no_speech_logp"] = self._no_speech_logp(logits)
            p += 1
            last.copy_(tokens[:, p])
        rounds = drafted = accepted = 0
        while p < Umax - 1:
            U = min(N, Umax - 2 - p)
            rounds += 1
            if U == 0:                                       # the last position below the bound: nothing to draft
                logits = self._dec_step(st, kv, last, p, True, begin=begin)
                if p == sot_pos and want_ns:
                    stats["no_speech_logp"] = self._no_speech_logp(logits)
                pick(logits, tokens, last, done, alive, sum_logp, p)
                p += 1
                break
            for q in range(dnext, p):
                draft._dec_step(dst, dkv, tokens[:, q].contiguous(), q, False, begin=begin)
            dlast.copy_(last)
            ddone.copy_(done)
            for k in range(U):
                pick(draft._dec_step(dst, dkv, dlast, p + k, True, begin=begin), hist, dlast, ddone, dalive, dsum, p + k)
            logits = self.decoder_append(st, kv, hist[:, p:p + U + 1], p, begin)
            if p == sot_pos and want_ns:
                stats["no_speech_logp"] = self._no_speech_logp(logits[:, 0])
            cand, logp = out[U]
            ops.whisper_verify(logits.view(B * (U + 1), V), hist, cand, logp, p, n0, eos, no_ts, suppress=fd["suppress"],
                               begin_suppress=fd["begin_suppress"], max_initial=max_initial)
            ops.whisper_accept(cand, logp, hist, tokens, last, done, alive, sum_logp, adv, p, eos)
            n_alive, a = sync.tolist()
            dnext = min(p + U, p + a)
            drafted += U
            accepted += min(a - 1, U)
            p += a
            if n_alive == 0:
                break
        gen = tokens[:, n0:]
        is_eos = gen == eos
        first = torch.where(is_eos.any(1), is_eos.to(torch.int64).argmax(1) + 1, torch.full((B,), Umax - n0, dtype=torch.int64, device=dev))
        if stats is not None:
            stats["sum_logp"] = sum_logp
            stats["assistant"] = dict(rounds=rounds, drafted=drafted, accepted=accepted)
            if begin is not None:                            # rows still open when the last step of the shared bound ran
                open_ = ~(tokens[:, n0:Umax - 1] == eos).any(1) if p == Umax - 1 else torch.zeros(B, dtype=torch.bool, device=dev)
                stats["at_bound"] = open_.to(I32)
        return tokens, (first + n0).to(I32)

    @staticmethod
    def _check_sampling(temperature, seed, beam_size, return_beams) -> bool:
        """-> whether the decode samples; refusals by name, before any launch."""
        if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not math.isfinite(temperature) or \
                temperature < 0:
            raise _C.F5EError(f"Whisper.generate: temperature = {temperature!r} must be a finite number >= 0")
        if temperature == 0:
            return False
        if int(beam_size) != 1 or return_beams:
            raise _C.F5EError(f"Whisper.generate: temperature = {temperature!r} with beam_size = {beam_size} is out of scope "
                              "(beam-sample is not built; sampling decodes one row per utterance)")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise _C.F5EError(f"Whisper.generate: seed = {seed!r} must be an integer in 0 .. 2^64 - 1")
        return True

    def _check_begin(self, begin, prompt, B: int, n0: int, want_sot: bool) -> Tuple[Optional[Tensor], int]:
        """-> (begin as i32 [B] on the device or None, the column of <|startoftranscript|>); refusals before any launch."""
        dev = self._fold()["device"]
        if begin is not None:
            host = [int(v) for v in (begin.tolist() if isinstance(begin, Tensor) else begin)]
            if len(host) != B or min(host) < 0 or max(host) >= n0:
                raise _C.F5EError(f"Whisper.generate: begin must be {B} pad counts in [0, {n0}) (got {host})")
            begin = torch.tensor(host, dtype=I32).to(dev)
        sot_pos = 0
        if want_sot:
            row = prompt[0] if isinstance(prompt, Tensor) and prompt.ndim == 2 else prompt
            row = row.tolist() if isinstance(row, Tensor) else (row[0] if len(row) and isinstance(row[0], (list, tuple)) else row)
            at = [i for i, t in enumerate(row) if int(t) == self.cfg.decoder_start_token_id]
            if not at:
                raise _C.F5EError("Whisper.generate: the prompt has no <|startoftranscript|> to read the no-speech probability at")
            sot_pos = at[-1]
        return begin, sot_pos

    def _no_speech_logp(self, logits: Tensor) -> Tensor:
        """log softmax(logits)[<|nospeech|>] per row (f5e_token_logp), from the step that fed <|startoftranscript|>."""
        target = torch.full((logits.shape[0],), self.cfg.no_speech_token_id, dtype=I32, device=logits.device)
        return ops.token_logp(logits, target)

    @torch.no_grad()
    def _beam_from_kv(self, kv: List[Tuple[Tensor, Tensor]], prompt: Sequence[int], max_new_tokens: Optional[int], sync_every: int,
                      K: int, length_penalty: float, return_beams: bool, ts: bool = False, stats: Optional[dict] = None,
                      begin: Optional[Tensor] = None, prefill: bool = False, sot_pos: int = 0):
        """The pooled beam search (f5e_whisper_beam_step has the rules): B * K rows, row b K + i = open hypothesis i of utterance
        b.  Every layer's self-attention follows the ancestry table, the cross-attention reads an utterance's keys once for its
        K rows, and no cache row ever moves.  The prompt goes through the same step without a pick (the K rows of an utterance
        are equal until the first pick).  Caches: K x the greedy figure, sized by the prompt + ``max_new_tokens`` when given.
        ``prefill``: the prompt but its last token is prefilled ONCE per utterance, into the cache row of its first beam, and the
        ancestry table sends every beam there for those positions (the rows are equal until the first pick, so this is what
        K equal prefills would leave).  ``begin`` i32 [B]: left-padding per utterance, shared by its K rows."""
        cfg = self.cfg
        V, eos = cfg.vocab_size, cfg.eos_token_id
        n0 = _prompt_len(prompt)
        ts_begin = cfg.timestamp_begin if ts else None
        banned = {t for t in tuple(cfg.suppress_tokens) + tuple(cfg.begin_suppress_tokens) if 0 <= t < V}
        if not 1 <= K <= 16:
            raise _C.F5EError(f"Whisper.generate: beam_size must lie in 1 .. 16 (got {K})")
        if V - len(banned) < 2 * K:
            raise _C.F5EError(f"Whisper.generate: beam_size = {K} needs {2 * K} classes that the first step does not suppress; "
                              f"{V} - {len(banned)} are left")
        fd = self._fold()
        B, dev = kv[0][0].shape[0], kv[0][0].device
        R = B * K
        Umax = cfg.max_target_positions if max_new_tokens is None else min(cfg.max_target_positions, n0 + int(max_new_tokens))
        if n0 < 1 or n0 >= Umax or sync_every < 1 or R > 65535:
            raise _C.F5EError(f"Whisper.generate: a prompt of {n0} tokens leaves no room below {Umax} positions (or sync_every < 1, "
                              f"or more than 65535 rows)")
        hyp = [torch.full((R, Umax), eos, dtype=I32, device=dev) for _ in range(2)]
        anc = [torch.arange(R, dtype=I32, device=dev)[:, None].repeat(1, Umax) for _ in range(2)]   # prompt: a row's own cache
        rows = self._prompt_rows(prompt, B, dev).repeat_interleave(K, 0)
        for h in hyp:
            h[:, :n0] = rows
        desc = torch.zeros(R, 4, dtype=I32, device=dev) if ts else None
        last = hyp[0][:, 0].clone()
        score = torch.full((B, K), -math.inf, dtype=F32, device=dev)
        score[:, 0] = 0.0
        score = score.view(R)
        pool_hyp = torch.full((B, K, Umax), eos, dtype=I32, device=dev)
        pool_len = torch.zeros(B, K, dtype=I32, device=dev)
        pool_score = torch.full((B, K), -math.inf, dtype=F32, device=dev)
        pool_n, open_, alive = (torch.full((B,), v, dtype=I32, device=dev) for v in (0, 1, 1))
        scratch = torch.empty(max(ops.whisper_beam_scratch(B, K, V), 4), dtype=torch.uint8, device=dev)
        st = self._dec_state(R, Umax, dev)
        cur, first_p = 0, 0
        begin_rows = None if begin is None else begin.repeat_interleave(K).contiguous()
        if prefill and n0 > 1:
            first_p = n0 - 1
            logits = self.decoder_prefill(st, kv, hyp[0][::K, :first_p].contiguous(), begin,
                                          (sot_pos,) if stats is not None and sot_pos < first_p else ())
            if logits is not None:
                stats["no_speech_logp"] = self._no_speech_logp(logits[:, 0])
            for a in anc:                                  # prompt positions live in the row of the utterance's first beam
                a[:, :first_p] = (torch.arange(R, dtype=I32, device=dev) // K * K)[:, None]
            last.copy_(hyp[0][:, first_p])
        at_bound = None
        for p in range(first_p, Umax - 1):
            forced = p + 1 < n0
            if p == Umax - 2 and begin is not None and stats is not None:
                at_bound = alive.clone()                     # utterances still searching when the last step of the bound runs
            logits = self._dec_step(st, kv, last, p, not forced or (p == sot_pos and stats is not None), anc=anc[cur],
                                    begin=begin_rows)
            if p == sot_pos and stats is not None:
                stats["no_speech_logp"] = self._no_speech_logp(logits)[::K].contiguous()
            if forced:
                last.copy_(hyp[0][:, p + 1])
                continue
            if ts:
                ops.whisper_beam_step_ts(logits, score, hyp[cur], anc[cur], hyp[1 - cur], anc[1 - cur], last, pool_hyp, pool_len,
                                         pool_score, pool_n, open_, alive, p, n0, Umax, eos, K, ts_begin - 1, desc,
                                         max_initial=cfg.max_initial_timestamp_index, suppress=fd["suppress"],
                                         begin_suppress=fd["begin_suppress"], length_penalty=length_penalty, scratch=scratch)
            else:
                ops.whisper_beam_step(logits, score, hyp[cur], anc[cur], hyp[1 - cur], anc[1 - cur], last, pool_hyp, pool_len,
                                      pool_score, pool_n, open_, alive, p, n0, Umax, eos, K, suppress=fd["suppress"],
                                      begin_suppress=fd["begin_suppress"], length_penalty=length_penalty, scratch=scratch)
            cur = 1 - cur
            if (p + 2 - n0) % sync_every == 0 and int(alive.sum().item()) == 0:
                break
        # columns at or beyond an entry's length are not defined by the step: eos there, as in the greedy layout
        col = torch.arange(Umax, device=dev)
        beams = torch.where(col[None, None, :] < pool_len[:, :, None], pool_hyp, torch.full_like(pool_hyp, eos))
        best = (beams[:, 0].contiguous(), pool_len[:, 0].contiguous())
        if stats is not None:
            stats["sum_logp"] = pool_score[:, 0] * (pool_len[:, 0] - n0).clamp(min=1).to(F32) ** length_penalty
            if begin is not None:
                stats["at_bound"] = torch.zeros(B, dtype=I32, device=dev) if at_bound is None else at_bound
        return best + ((beams, pool_len, pool_score),) if return_beams else best

    @torch.no_grad()
    def generate(self, wav: Tensor, lens=None, language: Optional[str] = None, task: str = "transcribe",
                 max_new_tokens: Optional[int] = None, sync_every: int = 8, beam_size: int = 1, length_penalty: float = 1.0,
                 return_beams: bool = False, return_token_timestamps: bool = False, return_timestamps: bool = False,
                 temperature: float = 0.0, seed: int = 0, assistant: Optional["Whisper"] = None, num_assistant_tokens: int = 5,
                 assistant_shares_encoder: bool = False, stats: Optional[dict] = None, *, step_graph: bool = False,
                 step_gemm: str = "f32"):
        """Recognition of B utterances: wav f32 [B, S] at 16 kHz on the GPU, lens samples per row -> (tokens i32 [B, U] starting
        with the prompt, eos from a row's end on; n i32 [B] = tokens of every row, its closing eos included when it ended by
        itself).  The host reads the alive count every ``sync_every`` steps; the result does not depend on it.  The bound is
        ``max_target_positions`` (or the prompt + ``max_new_tokens``).  ``beam_size`` 1: greedy, one row per utterance.
        ``beam_size`` K > 1: the pooled beam search of ``transformers``' ``generate(num_beams=K, length_penalty=...)``, K rows
        per utterance; the best finished hypothesis is returned in the same layout, and with ``return_beams`` a third item
        (pool tokens i32 [B, K, U], lens i32 [B, K], scores f32 [B, K] = sum of log-probabilities / generated length **
        length_penalty, best first).  ``return_token_timestamps``: one more item at the end, times f32 [B, U] in seconds of the
        returned tokens (``token_timestamps``; needs ``alignment_heads`` in the generation config).  ``language`` None: detected
        per row (``detect_language``); "" is refused as before.  ``return_timestamps``: the prompt has no <|notimestamps|> and
        the picks follow the timestamp rules, so the tokens carry <|t|> ids (``cfg.timestamp_begin`` + t / 0.02).
        ``temperature`` > 0: the picks are draws from softmax(logits / temperature) over the allowed classes, a function of
        ``seed``, the row's index and the position (``generate_from_kv``); with ``beam_size`` > 1 that is refused.
        ``assistant``: a draft ``Whisper`` for assisted generation (``generate_from_kv(assistant=)``; greedy only, the same
        tokens as without it).  ``assistant_shares_encoder`` False: the draft encodes the same audio itself; True: its cross keys
        and values are projected from THIS model's encoder output (large-v3-turbo and distil-whisper drafts; equal ``d_model``
        and encoder shape, checked).  ``stats`` (with an assistant or ``step_graph``): receives what ``generate_from_kv`` puts
        there.  ``step_graph`` / ``step_gemm``: the picks are replayed from a captured decode step (``generate_from_kv``; greedy,
        ruled or sampled, one row per utterance)."""
        if self._check_step_graph(step_graph, step_gemm, beam_size, return_beams, assistant, return_token_timestamps):
            self._check_sampling(temperature, seed, beam_size, return_beams)
            if return_timestamps:
                self.cfg.timestamp_begin                                    # refused by name before any launch
            elif language is not None:
                self.prompt_ids(language, task)
            enc = self.encode_features(self.features(wav, lens))
            kind = ("sample" if temperature > 0 else "greedy") + ("_ts" if return_timestamps else "")
            S = self._step_state(enc.shape[0], kind, False, step_gemm, enc.shape[1], enc.device)
            kv = self.cross_kv(enc, out=S.xkv)               # straight into the state the call below finds under the same key
            return self.generate_from_kv(kv, self._prompts(kv, language, task, return_timestamps), max_new_tokens, sync_every, 1,
                                         length_penalty, return_timestamps=return_timestamps, stats=stats, temperature=temperature,
                                         seed=seed, step_graph=True, step_gemm=step_gemm)
        if assistant is not None:
            self._check_sampling(temperature, seed, beam_size, return_beams)
            self._check_assistant(assistant, num_assistant_tokens, beam_size, return_beams, temperature)
            self._check_shared_encoder(assistant, assistant_shares_encoder, "generate")
            if return_timestamps:
                self.cfg.timestamp_begin                                    # refused by name before any launch
            elif language is not None:
                self.prompt_ids(language, task)
            enc = self.encode_features(self.features(wav, lens))
            kv = self.cross_kv(enc)
            dkv = assistant.cross_kv(enc) if assistant_shares_encoder else assistant.encode(wav, lens)
            return self.generate_from_kv(kv, self._prompts(kv, language, task, return_timestamps), max_new_tokens, sync_every, 1,
                                         length_penalty, False, return_token_timestamps,
                                         self._frames_of(wav, lens) if return_token_timestamps else None, return_timestamps,
                                         stats=stats, assistant=(assistant, dkv), num_assistant_tokens=num_assistant_tokens)
        if self._check_sampling(temperature, seed, beam_size, return_beams):
            if return_timestamps:
                self.cfg.timestamp_begin                                    # refused by name before any launch
            kv = self.encode(wav, lens)
            return self.generate_from_kv(kv, self._prompts(kv, language, task, return_timestamps), max_new_tokens, sync_every, 1,
                                         length_penalty, False, return_token_timestamps,
                                         self._frames_of(wav, lens) if return_token_timestamps else None, return_timestamps,
                                         temperature=temperature, seed=seed)
        if language is not None and not return_timestamps:
            prompt = self.prompt_ids(language, task)
            if not return_token_timestamps:
                return self.generate_from_kv(self.encode(wav, lens), prompt, max_new_tokens, sync_every, beam_size, length_penalty,
                                             return_beams)
            return self.generate_from_kv(self.encode(wav, lens), prompt, max_new_tokens, sync_every, beam_size, length_penalty,
                                         return_beams, True, self._frames_of(wav, lens))
        if return_timestamps:
            self.cfg.timestamp_begin                                    # refused by name before any launch
        kv = self.encode(wav, lens)
        return self.generate_from_kv(kv, self._prompts(kv, language, task, return_timestamps), max_new_tokens, sync_every, beam_size,
                                     length_penalty, return_beams, return_token_timestamps,
                                     self._frames_of(wav, lens) if return_token_timestamps else None, return_timestamps)

    # ---- long recordings: the sequential seek loop -------------------------------------------------------------------
    @torch.no_grad()
    def transcribe_long(self, wav: Tensor, lens=None, language: Optional[str] = None, task: str = "transcribe", beam_size: int = 1,
                        no_speech_threshold: Optional[float] = None, logprob_threshold: Optional[float] = None,
                        sync_every: int = 8, fallback: Optional[Fallback] = None, row_keys: Optional[Sequence[int]] = None,
                        trace: Optional[list] = None, context: Optional[Context] = None, assistant: Optional["Whisper"] = None,
                        num_assistant_tokens: int = 5, assistant_shares_encoder: bool = False, *, step_graph: bool = False,
                        step_gemm: str = "f32", **unbuilt) -> List[List[Segment]]:
        """Recordings of any length: wav f32 [B, S] at 16 kHz on the GPU, lens samples per row -> the segments of every row.
        The seek loop of ``transformers``' long-form ``generate`` (``return_timestamps=True``, ``condition_on_prev_tokens=False``,
        temperature 0): every window of ``n_frames`` mel frames is decoded with timestamp tokens, cut into segments at the
        timestamp pairs (``split_segments``), and the row's next window starts where the last complete segment ended.
          * features: once per row over its own samples, 160 * (len // 160) of them, so the clamp at the maximum - 8 is per
            recording; a window is a slice of them, zero-padded in the feature domain.  A row shorter than one window is framed
            as ``generate`` frames it, its samples zero-padded to the window (what the feature extractor does with a short
            recording), and equals ``generate(return_timestamps=True)``;
          * every iteration batches the current windows of the rows that are not finished; a row's result does not depend on
            its batch-mates;
          * ``language`` None: detected per row on the first window;
          * windows decode up to ``max_target_positions`` tokens;
          * ``no_speech_threshold`` and ``logprob_threshold`` (both or neither): a window whose <|nospeech|> probability exceeds
            the first and whose average log-probability falls below the second is skipped whole.
        ``avg_logprob``: greedy, the mean log-probability of the picks among the classes the rules allow (the closing eos
        counts), as ``_retrieve_avg_logprobs`` at temperature 0; beam search, the best hypothesis' own score.  One host read per
        window besides the alive counts.
        ``fallback`` (a ``Fallback``; None: every window is decoded once, as above): ``generate_with_fallback``.  The active
        windows are decoded at ``temperatures[0]``; a row whose compression ratio (of its tokens with the closing eos) exceeds
        ``compression_ratio_threshold`` or whose average log-probability lies below ``logprob_threshold`` is decoded again at the
        next temperature, and only such rows: their cross keys / values are gathered, nothing is encoded again.  A row for which
        the no-speech condition holds is skipped instead (``_need_fallback``).  After the last temperature the last attempt is
        kept.  0 is the greedy or beam decode; a positive temperature samples ONE row per utterance whatever ``beam_size`` is
        (f5e_whisper_sample_pick; ``avg_logprob`` is then the mean T = 1 log-probability of the draws), with the noise keyed by
        ``fallback.seed``, the position, the utterance's key (``row_keys``; None: its index in the call) and the number of sampled
        decodes the utterance has started before, so a row's result does not depend on its batch-mates.  ``logprob_threshold``
        and ``fallback.logprob_threshold`` are one threshold: two different values are refused.  ``Segment.temperature`` is the
        temperature of the attempt that was kept.  One host read per attempt.  ``trace``: a list that receives one dict per
        attempt (row, seek, temperature, compression_ratio, avg_logprob, no_speech_prob, needs_fallback, should_skip; with a
        ``context`` also prompt, the window's decoder input).
        ``context`` (a ``Context``; None: every window starts with its three forced tokens, as above): conditioning on the
        previous windows' text and an initial prompt.  Every window's decoder input is ``window_prompt`` of its row; the rows of
        an iteration are left-padded to a common length (``generate_from_kv(begin=)``) and the prompt goes through
        ``decoder_prefill`` in one pass.  The token bound stays ``max_target_positions`` for prompt and picks together
        (``_set_max_new_tokens_and_length`` grows ``max_length`` by the prompt and caps it there), so a fully conditioned window
        has ``max_target_positions - (max_target_positions // 2 - 1) - 4`` picks left.  With a ``fallback``, a window kept at a
        temperature of 0.5 or more does not condition the next one (``conditions_next_window``).  ``no_speech_prob`` is read
        at <|startoftranscript|>, wherever the prompt puts it.  Deliberately unlike ``transformers``, which decides from row
        0's history whether ANY row of a batch is conditioned, a row is conditioned iff it has previous segments of its own:
        a row equals its own B = 1 run.  Two things keep that true under padding (``_decode_with_context``): a padded row that
        runs into the batch's token bound, which counts its pad columns, is decoded again alone with its own bound, and a
        sampled attempt batches a row only with rows of its own prompt length, since the noise is keyed by the position.
        ``assistant`` (a draft ``Whisper``; ``generate``): every temperature-0 attempt is assisted generation under the timestamp
        rules; sampled attempts of a ``fallback`` take the path without it.  The draft reads the window's features (computed
        once, with this model's front-end) through its own encoder, or with ``assistant_shares_encoder`` this model's encoder
        output.  Segments, seeks and tokens are those of the run without an assistant.
        ``step_graph`` / ``step_gemm`` (``generate_from_kv``): every attempt's picks are replayed from a captured decode step,
        ``beam_size`` 1 only; an attempt with another row count or a sampled one runs on another cached state.  Segments,
        seeks and tokens are those of the eager run."""
        skw = {}
        if self._check_step_graph(step_graph, step_gemm, beam_size, False, assistant, False):
            skw = dict(step_graph=True, step_gemm=step_gemm)
        if assistant is not None:
            self._check_assistant(assistant, num_assistant_tokens, beam_size, False, 0.0)
            self._check_shared_encoder(assistant, assistant_shares_encoder, "transcribe_long")
        for name, value in unbuilt.items():
            off = {"temperature": (None, 0, 0.0, (0.0,), [0.0]), "condition_on_prev_tokens": (None, False), "prompt_ids": (None,),
                   "chunk_length_s": (None,), "stride_length_s": (None,), "return_token_timestamps": (None, False),
                   "graph": (None, False), "compression_ratio_threshold": (None,)}
            if name not in off:
                raise TypeError(f"Whisper.transcribe_long: unknown argument {name!r}")
            if not any(value is v or (not isinstance(value, Tensor) and value == v) for v in off[name]):
                raise _C.F5EError(f"Whisper.transcribe_long: {name} = {value!r} is out of scope (conditioning on previous tokens, "
                                  "prompt_ids, strided chunk merging, word timestamps across windows and a graph-captured step "
                                  "are not built under these names; temperature fallback goes through fallback=Fallback(...), "
                                  "conditioning and prompts through context=Context(...))")
        if fallback is not None and not isinstance(fallback, Fallback):
            raise _C.F5EError(f"Whisper.transcribe_long: fallback = {fallback!r} must be a Fallback or None")
        lp_thr = logprob_threshold                                     # one threshold for the fallback and for the no-speech skip
        if fallback is not None and fallback.logprob_threshold is not None:
            if logprob_threshold is not None and float(logprob_threshold) != float(fallback.logprob_threshold):
                raise _C.F5EError(f"Whisper.transcribe_long: logprob_threshold = {logprob_threshold!r} and "
                                  f"fallback.logprob_threshold = {fallback.logprob_threshold!r} are one threshold; give one value")
            lp_thr = fallback.logprob_threshold
        elif (no_speech_threshold is None) != (logprob_threshold is None):
            raise _C.F5EError("Whisper.transcribe_long: the no-speech skip needs no_speech_threshold and logprob_threshold together")
        if context is not None:
            self._check_context(context)
        cr_thr = None if fallback is None else fallback.compression_ratio_threshold
        temps = (0.0,) if fallback is None else fallback.temperatures
        if sync_every < 1:
            raise _C.F5EError("Whisper.transcribe_long: sync_every < 1")
        if row_keys is not None and isinstance(wav, Tensor) and wav.ndim == 2 and len(row_keys) != wav.shape[0]:
            raise _C.F5EError(f"Whisper.transcribe_long: row_keys has {len(row_keys)} entries for {wav.shape[0]} recordings")
        cfg = self.cfg
        ts_begin, eos, W, M = cfg.timestamp_begin, cfg.eos_token_id, self.n_frames, cfg.num_mel_bins
        wav, lens = self._check_audio(wav, lens, "transcribe_long")
        fd = self._fold()
        B, S = wav.shape
        dev = wav.device
        samples = [S] * B if lens is None else [min(int(v), S) for v in lens.tolist()]
        frames = [max(v // HOP, W) for v in samples]
        if min(samples) < 1:
            raise _C.F5EError(f"Whisper.transcribe_long: an empty recording (lens = {samples})")
        lens_dev = torch.tensor([min(v, f * HOP) for v, f in zip(samples, frames)], dtype=I32).to(dev)
        feats = [ops.whisper_logmel(wav[b:b + 1], lens_dev[b:b + 1], fd["window"], fd["twiddle"], fd["fb"], frames[b])[0]
                 for b in range(B)]
        prompts = None if language is None else self.prompt_ids(language, task, True)
        keys = list(range(B)) if row_keys is None else [int(v) for v in row_keys]
        seek, out, serial = [0] * B, [[] for _ in range(B)], [0] * B
        if context is not None:
            lead = context.prompt_ids
            if lead is not None and context.prompt_condition_type == "first-segment":     # ``_prepare_segments``
                lead = lead[1:] if lead[0] == cfg.prev_sot_token_id else lead
                history = [[list(lead)] for _ in range(B)]
            else:
                history = [[] for _ in range(B)]
            cond, cut = [context.condition_on_prev_tokens] * B, cfg.max_target_positions // 2 - 1
        while True:
            act = [b for b in range(B) if seek[b] < frames[b]]
            if not act:
                return out
            nf = [min(W, frames[b] - seek[b]) for b in act]
            win = torch.zeros(len(act), W, M, dtype=F32, device=dev)
            for i, b in enumerate(act):
                win[i, :nf[i]] = feats[b][seek[b]:seek[b] + nf[i]]
            if assistant is None:
                kv, asst = self.cross_kv(self.encode_features(win)), None
            else:
                enc = self.encode_features(win)
                kv = self.cross_kv(enc)
                asst = (assistant, assistant.cross_kv(enc if assistant_shares_encoder else assistant.encode_features(win)),
                        num_assistant_tokens)
            if prompts is None:                                        # the first iteration: every row is in it, at seek 0
                prompts = self._prompts(kv, None, task, True)
            prompt = prompts[torch.tensor(act, device=dev)] if isinstance(prompts, Tensor) else prompts
            plist = None
            if context is not None:                                    # per row: previous text / prompt + the forced tokens
                if isinstance(prompts, Tensor):
                    prompts = prompts.tolist()                         # the detected languages: one host read per call
                plist = [window_prompt(context, prompts[b] if isinstance(prompts[0], list) else prompts, history[b], cond[b],
                                      cfg.prev_sot_token_id, ts_begin, cut) for b in act]
            n0 = _prompt_len(prompt)
            kept, pend = [None] * len(act), list(range(len(act)))      # per active row: (full, avg, ns, cr, temperature, skip)
            for temp in temps:
                if context is not None:
                    rows = [act[i] for i in pend]
                    fulls, sum_logp, ns_logp = self._decode_with_context(
                        kv, plist, pend, temp, beam_size, sync_every, 0 if fallback is None else fallback.seed,
                        [keys[b] for b in rows], [serial[b] for b in rows], *(() if asst is None else (asst,)), **skw)
                    if temp > 0:
                        for b in rows:
                            serial[b] += 1
                else:
                    sub, sub_prompt, akw = kv, prompt, {}
                    if asst is not None and temp == 0:
                        akw = dict(assistant=asst[:2], num_assistant_tokens=asst[2])
                    if len(pend) < len(act):                           # only the rows that fall back: gathered, not re-encoded
                        idx = torch.tensor(pend, device=dev)
                        sub = [(k[idx], v[idx]) for k, v in kv]
                        sub_prompt = prompt[idx] if isinstance(prompt, Tensor) else prompt
                        if akw:
                            akw["assistant"] = (asst[0], [(k[idx], v[idx]) for k, v in asst[1]])
                    stats = {}
                    if temp > 0:
                        rows = [act[i] for i in pend]
                        tokens, n = self.generate_from_kv(
                            sub, sub_prompt, None, sync_every, 1, 1.0, return_timestamps=True, stats=stats, temperature=temp,
                            seed=fallback.seed, row_key=torch.tensor([keys[b] for b in rows], dtype=I32).to(dev),
                            serial=torch.tensor([serial[b] for b in rows], dtype=I32).to(dev), **skw)[:2]
                        for b in rows:
                            serial[b] += 1
                    else:
                        tokens, n = self.generate_from_kv(sub, sub_prompt, None, sync_every, beam_size, 1.0, return_timestamps=True,
                                                          stats=stats, **akw, **skw)[:2]
                    tokens, n = tokens.tolist(), n.tolist()
                    fulls = [tokens[j][n0:n[j]] for j in range(len(pend))]
                    sum_logp, ns_logp = stats["sum_logp"].tolist(), stats["no_speech_logp"].tolist()
                again = []
                for j, i in enumerate(pend):
                    full = fulls[j]
                    avg, ns = sum_logp[j] / max(len(full), 1), math.exp(ns_logp[j])
                    cr = compression_ratio(full, cfg.vocab_size)
                    skip = no_speech_threshold is not None and avg < lp_thr and ns > no_speech_threshold
                    need = not skip and fallback is not None and ((cr_thr is not None and cr > cr_thr) or
                                                                  (lp_thr is not None and avg < lp_thr))
                    kept[i] = (full, avg, ns, cr, temp, skip)
                    if need:
                        again.append(i)
                    if trace is not None:
                        trace.append(dict(row=act[i], seek=seek[act[i]], temperature=temp, compression_ratio=cr, avg_logprob=avg,
                                          no_speech_prob=ns, needs_fallback=need, should_skip=skip))
                        if context is not None:
                            trace[-1]["prompt"] = plist[i]
                pend = again
                if not pend:
                    break
            for i, b in enumerate(act):
                full, avg, ns, cr, temp, skip = kept[i]
                seq = full[:-1] if full and full[-1] == eos else full
                if context is not None:
                    cond[b] = context.condition_on_prev_tokens and conditions_next_window(temp)
                if not seq or skip:
                    seek[b] += nf[i]
                    continue
                parts, step = split_segments(seq, ts_begin, seek[b], nf[i])
                if step <= 0:
                    raise _C.F5EError(f"Whisper.transcribe_long: the window at frame {seek[b]} of row {b} does not advance")
                out[b].extend(Segment(s0, s1, tok, seek[b], avg, ns, cr, temp) for s0, s1, tok in parts)
                if context is not None:
                    history[b].extend(tok for _, _, tok in parts)
                seek[b] += step

    def _decode_with_context(self, kv, plist, ix, temp, beam_size, sync_every, seed, keys, serial, asst=None, **skw):
        """One attempt of the windows ``ix`` (indices into ``kv`` and ``plist``, the rows' decoder inputs) at ``temp`` ->
        (generated tokens with the closing eos, sum_logp, no_speech_logp) per row of ``ix``, each what the row's own B = 1 run
        gives.  Temperature 0: the rows are left-padded to their longest prompt and decoded together; the bound counts the pad
        columns, so a padded row that was still open when the last step of that shared bound ran (``at_bound``) is decoded again
        alone, with its own bound.  A sampled attempt keys its noise by the position, which padding would shift, so rows are
        batched only with rows of their own prompt length (a batch that falls back with ragged prompts costs one decode per
        length, not one per row).  ``asst`` = (draft, draft_kv, num_assistant_tokens): the temperature-0 decodes are assisted.
        ``skw``: ``step_graph`` / ``step_gemm`` for every decode."""
        eos, dev, res = self.cfg.eos_token_id, kv[0][0].device, {}

        def run(group):
            rows = [plist[i] for i in group]
            width = max(len(r) for r in rows)
            begin = [width - len(r) for r in rows]
            sub, dsub = kv, None if asst is None else asst[1]
            if group != list(range(kv[0][0].shape[0])):                  # gathered, not encoded again
                idx = torch.tensor(group, device=dev)
                sub = [(k[idx], v[idx]) for k, v in kv]
                dsub = None if asst is None else [(k[idx], v[idx]) for k, v in asst[1]]
            kw, st = {}, {}
            if asst is not None and temp == 0:
                kw = dict(assistant=(asst[0], dsub), num_assistant_tokens=asst[2])
            if temp > 0:
                at = [ix.index(i) for i in group]
                kw = dict(temperature=temp, seed=seed, row_key=torch.tensor([keys[j] for j in at], dtype=I32).to(dev),
                          serial=torch.tensor([serial[j] for j in at], dtype=I32).to(dev))
            tokens, n = self.generate_from_kv(sub, [[eos] * pad + r for pad, r in zip(begin, rows)], None, sync_every,
                                              1 if temp > 0 else beam_size, 1.0, return_timestamps=True, stats=st, begin=begin,
                                              prefill=True, **kw, **skw)[:2]
            tokens, n = tokens.tolist(), n.tolist()
            sl, ns, open_ = st["sum_logp"].tolist(), st["no_speech_logp"].tolist(), st["at_bound"].tolist()
            for j, i in enumerate(group):
                res[i] = (tokens[j][width:n[j]], sl[j], ns[j])
            return [i for j, i in enumerate(group) if begin[j] > 0 and open_[j]]

        if temp > 0:
            for length in sorted({len(plist[i]) for i in ix}):
                run([i for i in ix if len(plist[i]) == length])
        else:
            for i in run(list(ix)):
                run([i])
        return [res[i][0] for i in ix], [res[i][1] for i in ix], [res[i][2] for i in ix]

    def _check_context(self, context) -> None:
        """Refusals of ``transcribe_long(context=)`` by name, before any launch."""
        cfg = self.cfg
        if not isinstance(context, Context):
            raise _C.F5EError(f"Whisper.transcribe_long: context = {context!r} must be a Context or None")
        if (context.condition_on_prev_tokens or context.prompt_ids is not None) and cfg.prev_sot_token_id is None:
            raise _C.F5EError("Whisper.transcribe_long: generation_config has no prev_sot_token_id (<|startofprev|>); conditioning "
                              "on previous tokens and prompt_ids need it")
        ids = context.prompt_ids or ()
        if any(not 0 <= t < cfg.vocab_size for t in ids):
            raise _C.F5EError(f"Whisper.transcribe_long: prompt_ids {list(ids)} must be ids in [0, {cfg.vocab_size})")
        cut, cap = cfg.max_target_positions // 2 - 1, cfg.max_target_positions
        longest = len(ids) + 3
        if context.condition_on_prev_tokens:
            longest = max(longest, (len(ids) if context.prompt_condition_type == "all-segments" and ids else 1) + cut + 3)
        if longest >= cap:
            raise _C.F5EError(f"Whisper.transcribe_long: a prompt of {len(ids)} tokens, up to {cut} previous tokens and 3 forced "
                              f"tokens make {longest} positions, which leaves no room below max_target_positions = {cap}")


class WhisperRecognizer:
    """The duck type ``eval_wer.run_asr_wer`` and ``preprocess_ref_audio_text`` take: ``transcribe(wav_or_path, sr) -> str``."""

    def __init__(self, path: str, device="cuda", language: Optional[str] = "en", beam_size: int = 1, long_form: bool = False,
                 fallback: Optional[Fallback] = None, initial_prompt: Optional[str] = None,
                 condition_on_previous_text: bool = False, assistant_dir: Optional[str] = None, num_assistant_tokens: int = 5,
                 assistant_shares_encoder: bool = False, step_graph: bool = False, step_gemm: str = "f32", weights: str = "f32", assistant_weights: Optional[str] = None):
        """``weights``: "f32", "fp16", "bf16" or "auto" (``Whisper.from_pretrained_dir``), for the model and, unless
        ``assistant_weights`` names another mode for it, its assistant (the two need not agree; the transcripts are the model's): a
        16-bit mode halves the weight memory and the bytes of a decode step and gives the fp32 path's transcripts on an fp16
        checkpoint.  ``language``: a name or code, or None / "auto" to detect it per recording.  ``long_form``: ``transcribe`` runs the
        seek loop over the whole recording (``Whisper.transcribe_long``) instead of cutting it to the first chunk.  ``fallback``:
        the temperature fallback of that loop (needs ``long_form``).  ``initial_prompt``: text (a name, a domain word; ``Whisper.get_prompt_ids``, so
        the checkpoint needs merges.txt) given as a "first-segment" prompt: without conditioning it is put in front of EVERY
        window; with it, it leads the first window's previous text and then scrolls out of the cut (``Context``).
        ``condition_on_previous_text``: every window is conditioned on the text of the windows before it.  Both need
        ``long_form``.  ``assistant_dir``: a local directory of a draft model (large-v3-turbo, a distil-whisper checkpoint) for
        assisted generation with ``num_assistant_tokens`` drafts per round: the same transcripts, fewer passes of the large
        decoder; greedy only (``beam_size`` 1).  ``assistant_shares_encoder``: the draft has no encoder of its own to run and
        reads this model's encoder output.  ``step_graph`` / ``step_gemm``: ``transcribe`` and ``transcribe_segments`` replay
        their picks from a captured decode step (``Whisper.generate_from_kv``; ``beam_size`` 1, no assistant): the same
        transcripts; the replay alone is level with the eager step, ``step_gemm="skinny"`` takes 1.7x .. 1.95x off a token at
        the large-v3 / turbo decoder shapes."""
        self._step = {}
        if Whisper._check_step_graph(step_graph, step_gemm, beam_size, False, assistant_dir, False):
            self._step = dict(step_graph=True, step_gemm=step_gemm)
        if fallback is not None and not (long_form and isinstance(fallback, Fallback)):
            raise _C.F5EError("WhisperRecognizer: fallback needs long_form=True and a Fallback record")
        if (initial_prompt is not None or condition_on_previous_text) and not long_form:
            raise _C.F5EError("WhisperRecognizer: initial_prompt and condition_on_previous_text need long_form=True")
        if initial_prompt is not None and not isinstance(initial_prompt, str):
            raise _C.F5EError(f"WhisperRecognizer: initial_prompt = {initial_prompt!r} must be text or None")
        self.fallback = fallback
        self.device = torch.device(device)
        self.language = language
        self.beam_size = int(beam_size)      # the constructor's alone: transcribe() ignores the wenet flag of the same name
        self.long_form = bool(long_form)
        self.model = Whisper.from_pretrained_dir(path, weights=weights).to(self.device)
        if self._lang() is not None:
            self.model.prompt_ids(language)                  # a language the checkpoint does not know fails here, not per file
        elif not self.model.cfg.lang_to_id:
            raise _C.F5EError("WhisperRecognizer: language detection needs lang_to_id in generation_config.json")
        if self.long_form:
            self.model.cfg.timestamp_begin                   # refused by name here, not per file
        self.context = None
        if initial_prompt is not None or condition_on_previous_text:
            ids = None if initial_prompt is None else tuple(self.model.get_prompt_ids(initial_prompt))
            self.context = Context(condition_on_prev_tokens=bool(condition_on_previous_text), prompt_ids=ids)
            self.model._check_context(self.context)          # a prompt that leaves no room fails here, not per file
        self.assistant, self._assist = None, {}
        if assistant_dir is not None:
            self.assistant = Whisper.from_pretrained_dir(assistant_dir, weights=assistant_weights or weights).to(self.device)
            self.model._check_assistant(self.assistant, num_assistant_tokens, self.beam_size, False, 0.0)     # fails here, not per file
            self.model._check_shared_encoder(self.assistant, bool(assistant_shares_encoder),
                                             "transcribe_long" if self.long_form else "generate")
            self._assist = dict(assistant=self.assistant, num_assistant_tokens=int(num_assistant_tokens),
                                assistant_shares_encoder=bool(assistant_shares_encoder))
        self._warned = set()

    def _lang(self) -> Optional[str]:
        return None if self.language is None or str(self.language).lower() == "auto" else self.language

    def _audio(self, audio, sr: Optional[int], cut: bool = True) -> Tensor:
        """A wav path or a wave at ``sr`` -> mono f32 [1, S] at 16 kHz on the device, cut to the chunk (with a warning) unless
        ``cut`` is False."""
        from ..infer import audio as A
        from ..infer.utils_infer import load_wav
        name = audio if isinstance(audio, str) else None
        if isinstance(audio, str):
            audio, sr = load_wav(audio)
        if sr is None:
            raise _C.F5EError("WhisperRecognizer.transcribe: a tensor needs its sample rate")
        audio = torch.as_tensor(audio, dtype=F32)
        if audio.ndim == 1:
            audio = audio.unsqueeze(0)
        if audio.shape[0] > 1:
            audio = audio.mean(0, keepdim=True)
        audio = A.resample_device(audio.to(self.device, F32), int(sr), SAMPLE_RATE)
        limit = HOP * self.model.n_frames
        if cut and audio.shape[-1] > limit:
            if name not in self._warned:
                self._warned.add(name)
                warnings.warn(f"WhisperRecognizer: {name or 'audio'} is {audio.shape[-1] / SAMPLE_RATE:.1f} s long; only the first "
                              f"{limit / SAMPLE_RATE:.0f} s are transcribed (long-form chunking is out of scope)")
            audio = audio[:, :limit]
        return audio.contiguous()

    @torch.no_grad()
    def transcribe(self, audio, sr: Optional[int] = None, mode=None, **ignored) -> str:
        if getattr(self, "long_form", False):
            return "".join(text for _, _, text in self.transcribe_segments(audio, sr)).strip()
        tokens, n = self.model.generate(self._audio(audio, sr), None, self._lang(), beam_size=self.beam_size,
                                        **getattr(self, "_assist", {}), **getattr(self, "_step", {}))
        return self.model.decode_ids(tokens[0, :int(n[0])].tolist()).strip()

    @torch.no_grad()
    def transcribe_segments(self, audio, sr: Optional[int] = None) -> List[Tuple[float, float, str]]:
        """-> [(start_s, end_s, text)] over the whole recording, however long (``Whisper.transcribe_long``)."""
        kw = {} if getattr(self, "fallback", None) is None else dict(fallback=self.fallback)
        if getattr(self, "context", None) is not None:
            kw["context"] = self.context
        kw.update(getattr(self, "_assist", {}))
        kw.update(getattr(self, "_step", {}))
        segs = self.model.transcribe_long(self._audio(audio, sr, cut=False), None, self._lang(), beam_size=self.beam_size, **kw)[0]
        return [(s.start_s, s.end_s, self.model.decode_ids(s.tokens)) for s in segs]

    @torch.no_grad()
    def transcribe_words(self, audio, sr: Optional[int] = None) -> list:
        """-> [WordSpan(word, start_s, end_s)] of the transcript (``ppg.ctc_align.WordSpan``): the decoded hypothesis goes through
        ``token_timestamps(include_last=True)``, so the closing token's time ends the last word.  Words are stripped of the
        punctuation merged into them and of surrounding space; a word of punctuation alone is dropped."""
        from ..ppg.ctc_align import WordSpan
        if self._lang() is None:
            raise _C.F5EError("WhisperRecognizer.transcribe_words: word timestamps need a named language (not 'auto')")
        model, wav = self.model, self._audio(audio, sr)
        kv = model.encode(wav)
        prompt = model.prompt_ids(self.language)
        tokens, n = model.generate_from_kv(kv, prompt, beam_size=self.beam_size)[:2]
        times = model.token_timestamps(kv, tokens, n, model._frames_of(wav, None), len(prompt), include_last=True)
        k = int(n[0])
        spans = []
        for word, start, end in model.words_from_tokens(tokens[0, :k].tolist(), times[0, :k].tolist(), self.language):
            word = word.strip().strip(PREPEND_PUNCTUATIONS + APPEND_PUNCTUATIONS).strip()
            if word:
                spans.append(WordSpan(word, start, end))
        return spans

    def align(self, audio, sr: Optional[int], text: str) -> list:
        """``CTCAligner.align``'s signature: the word spans of the recording, carrying the words of ``text``.  The recording is
        transcribed with word times; ``split_words(text)`` must agree with the transcript's words (case and punctuation
        aside), else ValueError names the first pair that differs: correct the text or give the parts by hand."""
        from ..ppg.ctc_align import WordSpan, split_words

        def key(w):
            return "".join(ch for ch in w.lower() if ch.isalnum())
        spans = [s for span in self.transcribe_words(audio, sr) for s in _per_word(span, split_words) if key(s.word)]
        want = [w for w in split_words(text) if key(w)]
        for i in range(max(len(want), len(spans))):
            a = want[i] if i < len(want) else None
            b = spans[i].word if i < len(spans) else None
            if a is None or b is None or key(a) != key(b):
                raise ValueError(f"WhisperRecognizer.align: the text and the transcript differ at word {i}: {a!r} vs {b!r} "
                                 f"(transcript: {' '.join(s.word for s in spans)!r}); correct the text or give the parts by hand")
        return [WordSpan(w, s.start_s, s.end_s) for w, s in zip(want, spans)]


def _per_word(span, split_words) -> list:
    """A transcript word that ``split_words`` cuts further (every CJK character is a word of its own) shares its span evenly."""
    parts = [w for w in split_words(span.word) if any(ch.isalnum() for ch in w)]
    if len(parts) <= 1:
        return [span]
    step = (span.end_s - span.start_s) / len(parts)
    return [type(span)(w, span.start_s + k * step, span.start_s + (k + 1) * step) for k, w in enumerate(parts)]
