"""Streaming recognition: audio in as it arrives, a partial transcript out after every block.

``StreamingRecognizer`` joins the pieces that exist for whole utterances -- the kaldi fbank kernel, the incremental encoder
(``ConformerEngine.forward_chunk``, the reference's ``BaseEncoder.forward_chunk``), the CTC projection -- to the resumable CTC
prefix beam search (``ops.ctc_beam_chunk``, csrc/ctc_beam.hip).  Per block of samples it runs the fbank on the whole frames
that became available, one ``forward_chunk`` per COMPLETE window of the reference's chunk-by-chunk loop
(``forward_chunk_by_chunk``, wenet/transformer/encoder.py:328-343) and one search call over the new encoder frames; nothing is
recomputed, and nothing is read back until ``partial()`` / ``nbest()`` / ``finish()`` ask.  Because the search is bit for bit
the whole-utterance search on the same logits, ``finish()`` returns what ``ctc_prefix_beam_search(...,
simulate_streaming=True)`` returns on the whole recording whenever the logits' margins hold (the chunk loop and the one-pass
banded encoder differ in rounding only).

One utterance per recogniser: the search kernel is batched, the encoder's chunk path is batch 1.  Host code here: the window
bookkeeping (``ready_windows``, a pure function), the sample / feature remainders and the capacity check."""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import torch

from .. import _C, ops

F32, I32 = torch.float32, torch.int32
Tensor = torch.Tensor

SAMPLE_RATE = 16000
FRAMES_PER_SECOND = 100        # kaldi fbank: 10 ms shift
STREAM_MODES = ("ctc_prefix_beam_search", "attention_rescoring")


def ready_windows(num_frames: int, cur: int, chunk: int, final: bool, rate: int = 2,
                  context: int = 3) -> List[Tuple[int, int]]:
    """The feature windows [start, end) of the reference's loop that can run NOW: ``num_frames`` feature frames of the
    utterance have arrived, the next window starts at ``cur``.  A window is rate (chunk - 1) + context frames at stride rate
    chunk (``rate``: the model's subsampling rate, ``context`` = its right context + 1; the defaults are the 2x front).  Before
    the end of the utterance only complete windows run (what follows cannot change them); with ``final`` the loop's own bound
    applies, a last short window running while at least ``context`` frames remain from its start.  Fed a whole utterance at
    once (cur = 0, final) this is ``range(0, num_frames - context + 1, rate * chunk)`` with ``end = min(cur + window,
    num_frames)``."""
    if chunk < 1:
        raise _C.F5EError(f"streaming: decoding_chunk_size must be positive (got {chunk})")
    window, stride = rate * (chunk - 1) + context, rate * chunk
    out = []
    while cur + window <= num_frames or (final and cur < num_frames - context + 1):
        out.append((cur, min(cur + window, num_frames)))
        cur += stride
    return out


def check_sample_rate(sr) -> None:
    if int(sr) != SAMPLE_RATE:
        raise _C.F5EError(f"streaming: the recogniser takes {SAMPLE_RATE} Hz audio (got {sr}); resampling inside the stream "
                          "is not built")


def check_capacity(fed_frames: int, new_frames: int, max_frames: int, max_seconds: float) -> None:
    """Feature frames: raises before anything is launched when the utterance would run past ``max_seconds``."""
    if fed_frames + new_frames > max_frames:
        raise _C.F5EError(f"streaming: {fed_frames} + {new_frames} feature frames run past max_seconds = {max_seconds} "
                          f"({max_frames} frames); reset() or build the recogniser with a larger max_seconds")


def check_stream_args(beam_size: int, decoding_chunk_size: int, max_seconds: float, vocab: int) -> Tuple[int, int, int]:
    """-> (beam, chunk, max feature frames); caller bugs raise here, on the host."""
    beam, chunk = int(beam_size), int(decoding_chunk_size)
    if not 1 <= beam <= min(16, vocab):
        raise _C.F5EError(f"streaming: beam_size must lie in 1..{min(16, vocab)} (got {beam_size})")
    if not 1 <= chunk <= 16384:
        raise _C.F5EError(f"streaming: decoding_chunk_size must lie in 1..16384 (got {decoding_chunk_size}); a recogniser "
                          "always runs chunk by chunk")
    max_frames = int(float(max_seconds) * FRAMES_PER_SECOND)
    if max_frames < 3:
        raise _C.F5EError(f"streaming: max_seconds = {max_seconds} holds fewer than 3 feature frames")
    return beam, chunk, max_frames


class StreamingRecognizer:
    """Built by ``ConformerPPG.streaming_recognizer`` (or ``CTCAligner.stream``, which adds the detokeniser)."""

    def __init__(self, model, beam_size: int = 10, decoding_chunk_size: int = 16, num_decoding_left_chunks: int = -1,
                 max_seconds: float = 60.0, use_linear: bool = False, detokenize: Optional[Callable] = None):
        from .ppg_model import ConformerEngine, kaldiFbank
        # caller bugs first: they are the same on any device
        self.beam, self.chunk, self.max_frames = check_stream_args(beam_size, decoding_chunk_size, max_seconds,
                                                                   model.vocab_size)
        if not (model.static_chunk_size > 0 or model.use_dynamic_chunk):
            raise _C.F5EError("PPG extractor: streaming needs a chunk-trained model (static_chunk_size > 0 or "
                              "use_dynamic_chunk in encoder_conf)")
        self.model, self.left, self.max_seconds = model, int(num_decoding_left_chunks), float(max_seconds)
        self.use_linear, self.detokenize = bool(use_linear), detokenize
        self.eng = model._require_ctc()
        self.device = self.eng.device
        self.rate, self.context = self.eng.rate, self.eng.context       # the model's subsampling front
        self.T_cap = max(1, ConformerEngine.stream_frames(self.max_frames, self.chunk, self.rate, self.context))
        self.state = ops.ctc_beam_state(1, self.T_cap, self.chunk, self.beam, device=self.device)
        self.fbank = kaldiFbank().eval().to(self.device)
        self.V = self.eng.ctc_w.shape[0]
        self._idle_scores = torch.zeros(1, 1, self.V, device=self.device)        # a readout feeds no frame
        self._counts = {n: torch.tensor([n], dtype=I32, device=self.device) for n in range(self.chunk + 1)}
        self._clear()

    def _clear(self) -> None:
        self.samples = torch.empty(0, device=self.device)       # samples from the start of the next fbank frame on
        self.feats = torch.empty(0, self.eng.idim, device=self.device)     # feature frames from ``cur`` on
        self.cur = 0                  # feature frame at which the next window starts
        self.num_frames = 0           # feature frames of the utterance so far
        self.offset = 0               # encoder frames so far = frames the search has consumed
        self.caches = (None, None, None)
        self.enc: List[Tensor] = []
        self.finished = False

    def reset(self) -> None:
        """Back to the start of an utterance: the search state at the empty prefix, every buffer dropped."""
        self.state.init()
        self._clear()

    # ---- input

    @torch.no_grad()
    def accept_waveform(self, samples) -> int:
        """16 kHz mono f32 samples (host or device, 1-D or [1, n], any length including 0) -> encoder frames added."""
        wav = torch.as_tensor(samples)
        if wav.ndim == 2 and wav.shape[0] == 1:
            wav = wav[0]
        if wav.ndim != 1:
            raise _C.F5EError(f"streaming: accept_waveform takes mono samples [n] or [1, n] (got {tuple(wav.shape)})")
        self._open()
        win, shift = self.fbank.win, self.fbank.shift
        have = self.samples.shape[0] + wav.shape[0]
        k = 1 + (have - win) // shift if have >= win else 0
        check_capacity(self.num_frames, k, self.max_frames, self.max_seconds)
        self.samples = torch.cat((self.samples, wav.to(self.device, F32)))
        if k == 0:
            return 0
        feats, _ = self.fbank(self.samples[None, :(k - 1) * shift + win])
        self.samples = self.samples[k * shift:]
        return self._accept(feats[0])

    @torch.no_grad()
    def accept_features(self, feats) -> int:
        """fbank frames [n, idim] or [1, n, idim] (host or device) -> encoder frames added."""
        feats = torch.as_tensor(feats)
        if feats.ndim == 3 and feats.shape[0] == 1:
            feats = feats[0]
        if feats.ndim != 2 or feats.shape[1] != self.eng.idim:
            raise _C.F5EError(f"streaming: accept_features takes frames [n, {self.eng.idim}] (got {tuple(feats.shape)})")
        self._open()
        check_capacity(self.num_frames, feats.shape[0], self.max_frames, self.max_seconds)
        return self._accept(feats.to(self.device, F32))

    def _open(self) -> None:
        if self.finished:
            raise _C.F5EError("streaming: the utterance is finished; reset() starts the next one")

    def _accept(self, feats: Tensor) -> int:
        self.feats = torch.cat((self.feats, feats))
        self.num_frames += feats.shape[0]
        return self._run(final=False)

    def _run(self, final: bool) -> int:
        """One forward_chunk, one CTC projection and one search call per window that is ready."""
        eng, added, base = self.eng, 0, self.cur
        for a, b in ready_windows(self.num_frames, self.cur, self.chunk, final, self.rate, self.context):
            y, *self.caches = eng.forward_chunk(self.feats[None, a - base:b - base], self.offset, self.chunk * self.left,
                                                *self.caches)
            n = y.shape[1]
            if self.offset + n > self.T_cap:                      # cannot happen below max_frames; never reach the kernel with it
                raise _C.F5EError(f"streaming: {self.offset + n} encoder frames exceed the search state's {self.T_cap}")
            self.enc.append(y)
            ops.ctc_beam_chunk(eng.ctc_logits(eng.head(y)[0] if self.use_linear else y), self._counts[n], self.state,
                               want_result=False)
            self.offset += n
            added += n
            self.cur = a + self.rate * self.chunk
        self.feats = self.feats[self.cur - base:] if self.cur > base else self.feats
        return added

    # ---- output

    @torch.no_grad()
    def nbest(self) -> List[Tuple[Tuple[int, ...], float]]:
        """The n-best list on everything heard so far, best first: one readout launch, one copy to the host."""
        K, ld = self.beam, max(1, self.offset)                    # no prefix is longer than the frames consumed
        buf = torch.empty(K * ld + 2 * K, dtype=I32, device=self.device)
        hyp, n, sc = buf[:K * ld].view(1, K, ld), buf[K * ld:K * ld + K].view(1, K), buf[K * ld + K:].view(F32).view(1, K)
        ops.ctc_beam_chunk(self._idle_scores, self._counts[0], self.state, hyp=hyp, hyp_len=n, score=sc)
        host = buf.cpu()
        hyp_h, n_h = host[:K * ld].view(K, ld), host[K * ld:K * ld + K].tolist()
        sc_h = host[K * ld + K:].view(F32).tolist()
        return [(tuple(int(v) for v in hyp_h[k, :n_h[k]]), float(sc_h[k])) for k in range(K) if n_h[k] >= 0]

    def partial(self) -> Tuple[Tuple[int, ...], float]:
        """(ids, score) of the best prefix so far."""
        return self.nbest()[0]

    def encoder_out(self) -> Tensor:
        """The encoder output so far, [1, T', D]."""
        return torch.cat(self.enc, 1) if self.enc else torch.empty(1, 0, self.eng.dim, device=self.device)

    @torch.no_grad()
    def finish(self, mode: str = "ctc_prefix_beam_search", ctc_weight: float = 0.5, reverse_weight: float = 0.0):
        """The end of the utterance: the last short window runs if at least 3 feature frames remain from its start, then
        ``ctc_prefix_beam_search`` -> the n-best list of (ids, score); ``attention_rescoring`` -> (ids, score) of the entry
        the attention decoder likes best, the existing device decoder on the encoder output kept here.  Samples that do not
        fill a last fbank frame are dropped, as the whole-utterance fbank drops them."""
        if mode not in STREAM_MODES:
            raise _C.F5EError(f"streaming: unknown mode {mode!r} (one of {', '.join(STREAM_MODES)})")
        if mode == "attention_rescoring":
            self.model._require_decoder(reverse_weight)
        if not self.finished:
            self._run(final=True)
            self.finished = True
        nbest = self.nbest()
        if mode == "ctc_prefix_beam_search":
            return nbest
        if not self.enc:
            raise _C.F5EError("streaming: attention_rescoring needs at least 3 feature frames of audio")
        enc = self.encoder_out()
        return self.model._rescore(self.eng, enc, torch.tensor([enc.shape[1]], dtype=I32), [nbest], self.beam,
                                   ctc_weight, reverse_weight)[0]

    # ---- text (``CTCAligner.stream``)

    def _text(self, ids) -> str:
        if self.detokenize is None:
            raise _C.F5EError("streaming: this recogniser has no detokeniser (build it with CTCAligner.stream)")
        return self.detokenize(ids)

    def partial_text(self) -> str:
        return self._text(self.partial()[0])

    def finish_text(self, mode: str = "ctc_prefix_beam_search", ctc_weight: float = 0.5, reverse_weight: float = 0.0) -> str:
        res = self.finish(mode, ctc_weight, reverse_weight)
        return self._text(res[0][0] if mode == "ctc_prefix_beam_search" else res[0])
