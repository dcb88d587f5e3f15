"""Text in, timestamps out: the CTC half of the ASR model (``ConformerPPG(ctc=True)``) as a forced aligner and a greedy
transcriber.  The reference tells the user of ``infer/speech_edit.py`` to install an outside CTC forced aligner and to type
the ``parts_to_edit`` by hand, although its own ASR model carries a CTC head, ``wenet/utils/ctc_util.py::forced_align`` and
``wenet/bin/alignment.py``; this module is those three behind one class, with the search on the device (csrc/ctc.hip).

Host code here: the symbol table, the tokeniser and the frame -> second arithmetic.  ``frames_timestamp`` restates
``get_frames_timestamp`` of wenet/bin/alignment.py (that script cannot be imported -- it pulls in ``textgrid`` and dataset
modules at the top -- so its parity is not pinned by a fixture; tests/test_ctc_cpu.py checks its properties)."""
from __future__ import annotations

from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from .. import _C

FRAME_SHIFT_S = 0.01      # kaldi fbank: 10 ms
SUBSAMPLING = 2           # Conv2dSubsampling2, the `conv2d` front-end: the default where no model says its rate


class WordSpan(NamedTuple):
    word: str
    start_s: float
    end_s: float


def read_symbol_table(path: str) -> Dict[str, int]:
    """``token id`` lines (wenet/utils/file_utils.py::read_symbol_table)."""
    table = {}
    with open(path, "r", encoding="utf8") as fin:
        for line in fin:
            arr = line.strip().split()
            if not arr:
                continue
            if len(arr) != 2:
                raise ValueError(f"{path}: expected `token id`, got {line!r}")
            table[arr[0]] = int(arr[1])
    return table


def _is_cjk(ch: str) -> bool:
    o = ord(ch)
    return (0x4E00 <= o <= 0x9FFF or 0x3400 <= o <= 0x4DBF or 0xF900 <= o <= 0xFAFF or 0x3040 <= o <= 0x30FF
            or 0xAC00 <= o <= 0xD7AF or 0x20000 <= o <= 0x2FA1F)


def split_words(text: str) -> List[str]:
    """Whitespace splits words; every CJK character is its own word."""
    words, cur = [], ""
    for ch in text:
        if ch.isspace() or _is_cjk(ch):
            if cur:
                words.append(cur)
                cur = ""
            if not ch.isspace():
                words.append(ch)
        else:
            cur += ch
    if cur:
        words.append(cur)
    return words


def default_tokenize(text: str, table: Dict[str, int]) -> Tuple[List[str], List[List[int]]]:
    """-> (words, ids per word).  A word becomes its characters, looked up as-is, then lower-cased, then upper-cased, then
    ``<unk>`` if the table has it; characters without an entry are dropped (a word may be left with no ids)."""
    words = split_words(text)
    ids = []
    for w in words:
        row = []
        for ch in w:
            for cand in (ch, ch.lower(), ch.upper(), "<unk>"):
                if cand in table:
                    row.append(table[cand])
                    break
        ids.append(row)
    return words, ids


def frames_timestamp(alignment: Sequence[int], blank: int = 0) -> List[List[int]]:
    """``get_frames_timestamp`` (wenet/bin/alignment.py:55-73): the frame classes cut into one segment per token -- leading
    blanks belong to the following token, the token's own frames follow, trailing blanks join the last segment."""
    alignment = list(alignment)
    out, start, end = [], 0, 0
    while end < len(alignment):
        while end < len(alignment) and alignment[end] == blank:
            end += 1
        if end == len(alignment):
            if not out:
                raise ValueError("frames_timestamp: the alignment holds no token")
            out[-1] += alignment[start:]
            break
        end += 1
        while end < len(alignment) and alignment[end - 1] == alignment[end]:
            end += 1
        out.append(alignment[start:end])
        start = end
    return out


def word_spans(words: Sequence[str], ids: Sequence[Sequence[int]], tok_end: Sequence[int], n_frames: int,
               frame_s: float = FRAME_SHIFT_S * SUBSAMPLING, total_s: Optional[float] = None) -> List[WordSpan]:
    """Token segments in ``frames_timestamp``'s sense from the kernel's ``tok_end`` (segment i = [tok_end[i-1], tok_end[i]),
    the first from frame 0, the last to ``n_frames``) -> one span per word, from the start of its first token's segment to the
    end of its last.  A word with no tokens gets an empty span at its neighbour's edge.  ``total_s`` caps the times (the
    last encoder frame may reach past the audio by part of a window)."""
    n_tok = sum(len(r) for r in ids)
    if n_tok == 0:
        raise ValueError("no character of the text is in the symbol table")
    edges = [0] + [int(e) for e in tok_end[:n_tok]]
    edges[-1] = int(n_frames)
    cap = (lambda t: min(t, total_s)) if total_s is not None else (lambda t: t)
    spans, k, last = [], 0, None
    for w, row in zip(words, ids):
        if row:
            last = (cap(edges[k] * frame_s), cap(edges[k + len(row)] * frame_s))
            spans.append(WordSpan(w, *last))
            k += len(row)
        else:
            spans.append(None)
    # empty words: the end of the word before, or the start of the first word that has tokens
    first = next(s for s in spans if s is not None)
    edge = first.start_s
    for i, (w, s) in enumerate(zip(words, spans)):
        if s is None:
            spans[i] = WordSpan(w, edge, edge)
        else:
            edge = s.end_s
    return spans


DECODE_MODES = ("ctc_greedy_search", "ctc_prefix_beam_search", "attention_rescoring")     # the reference's mode names


class CTCAligner:
    """``align(audio, sr, text)`` -> word-level timestamps; ``transcribe(audio, sr, mode=...)`` -> text (greedy by default;
    ``attention_rescoring`` needs ``decoder=True`` or a model built with its attention decoder); ``score(audio, sr, text)``
    / ``score_batch(waves, sr, text)`` -> log P(text | audio) under the CTC head, the ranking of best-of-N synthesis.
    ``tokenize``: optional ``text -> (words, ids per word)`` in place of ``default_tokenize`` (BPE models bring their own).
    ``model`` / ``symbol_table``: an already built ``ConformerPPG(ctc=True)`` and table instead of the three paths."""

    def __init__(self, ppg_model_path: Optional[str] = None, ppg_config: Optional[str] = None,
                 dict_path: Optional[str] = None, device="cuda", tokenize: Optional[Callable] = None, *, model=None,
                 symbol_table: Optional[Dict[str, int]] = None, decoder: bool = False, asr: bool = False):
        from .ppg_model import build_asr_model, build_ppg_model, kaldiFbank
        self.device = device
        build = build_asr_model if asr else build_ppg_model      # asr: also the 4x / 6x / 8x fronts and layer-norm conv modules
        self.model = model if model is not None else build(ppg_model_path, ppg_config, device, ctc=True, decoder=decoder)
        if not getattr(self.model, "has_ctc", False):
            raise _C.F5EError("CTCAligner: the model was built without its CTC head (ctc=True)")
        self.table = dict(symbol_table) if symbol_table is not None else read_symbol_table(dict_path)
        self.inverse = {v: k for k, v in self.table.items()}
        self.tokenize = tokenize or (lambda text: default_tokenize(text, self.table))
        self.featCal = kaldiFbank().eval()
        # seconds per encoder frame: the fbank shift times the model's subsampling rate (20 ms for the 2x front)
        self.frame_s = FRAME_SHIFT_S * int(getattr(self.model, "subsampling_rate", SUBSAMPLING))

    def _feats(self, audio, sr):
        from ..infer import audio as A
        from ..infer.utils_infer import load_wav
        if isinstance(audio, str):
            audio, sr = load_wav(audio)
        if audio.ndim == 1:
            audio = audio.unsqueeze(0)
        if audio.shape[0] > 1:
            audio = audio.mean(0, keepdim=True)
        secs = audio.shape[-1] / float(sr)
        audio = A.resample_device(audio.to(self.device, torch.float32), sr, 16000)
        feats, feats_len = self.featCal(audio)
        return feats, feats_len.to(self.device), secs

    def _check_decoding(self, decoding_chunk_size: int, simulate_streaming: bool) -> None:
        """The model's check of the streaming parameters for the one utterance handled here, before any feature is computed."""
        self.model._check_decoding(torch.empty(1, 0, 0), decoding_chunk_size, simulate_streaming)

    def _text(self, ids) -> str:
        return "".join(self.inverse.get(int(i), "") for i in ids).replace("▁", " ").strip()

    @torch.no_grad()
    def transcribe(self, audio, sr: Optional[int] = None, mode: str = "ctc_greedy_search", beam_size: int = 10,
                   ctc_weight: float = 0.5, reverse_weight: float = 0.0, *, decoding_chunk_size: int = -1,
                   num_decoding_left_chunks: int = -1, simulate_streaming: bool = False) -> str:
        """``mode``: one of the reference's ``ctc_greedy_search`` (the default), ``ctc_prefix_beam_search`` (the best of the
        n-best at ``beam_size``) and ``attention_rescoring`` (that list re-ranked by the attention decoder).  The three
        keyword-only arguments are the reference's (``ConformerPPG._check_decoding``): by default the encoder sees the whole
        recording; ``decoding_chunk_size > 0`` with ``simulate_streaming=True`` runs it chunk by chunk."""
        stream = dict(decoding_chunk_size=decoding_chunk_size, num_decoding_left_chunks=num_decoding_left_chunks,
                      simulate_streaming=simulate_streaming)
        if mode not in DECODE_MODES:
            raise _C.F5EError(f"CTCAligner.transcribe: unknown mode {mode!r} (one of {', '.join(DECODE_MODES)})")
        if mode == "attention_rescoring" and getattr(self.model, "decoder_type", None) is None:
            raise _C.F5EError("CTCAligner.transcribe: attention_rescoring needs a model built with its attention decoder "
                              "(CTCAligner(decoder=True) / build_ppg_model(decoder=True))")
        self._check_decoding(decoding_chunk_size, simulate_streaming)
        feats, lens, _ = self._feats(audio, sr)
        if mode == "ctc_greedy_search":
            ids = self.model.ctc_greedy_search(feats, lens, pad_id=-1, **stream)[0][0]
        elif mode == "ctc_prefix_beam_search":
            ids = self.model.ctc_prefix_beam_search(feats, lens, beam_size, **stream)[0][0][0]
        else:
            ids = self.model.attention_rescoring(feats, lens, beam_size, ctc_weight=ctc_weight,
                                                 reverse_weight=reverse_weight, **stream)[0][0]
        return self._text(ids)

    @torch.no_grad()
    def recognize(self, audio, sr: Optional[int] = None, beam_size: int = 10, reorder_cache: bool = False, *,
                  decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1,
                  simulate_streaming: bool = False) -> str:
        """The reference's decoding mode ``attention`` (wenet/bin/recognize.py -> ASRModel.recognize): beam search over the
        attention decoder; the ids up to the first eos, detokenised as ``transcribe`` does.  It is a method of its own and
        not a ``transcribe`` mode.  Needs a model built with its attention decoder."""
        if getattr(self.model, "decoder_type", None) is None:
            raise _C.F5EError("CTCAligner.recognize needs a model built with its attention decoder "
                              "(CTCAligner(decoder=True) / build_ppg_model(decoder=True))")
        self._check_decoding(decoding_chunk_size, simulate_streaming)
        feats, lens, _ = self._feats(audio, sr)
        row = self.model.recognize(feats, lens, beam_size, reorder_cache=reorder_cache,
                                   decoding_chunk_size=decoding_chunk_size, num_decoding_left_chunks=num_decoding_left_chunks,
                                   simulate_streaming=simulate_streaming)[0][0].cpu().tolist()
        ids = row[:row.index(self.model.eos)] if self.model.eos in row else row
        return self._text(ids)

    def stream(self, **kw):
        """A ``StreamingRecognizer`` (ppg/streaming_asr.py; the keywords of ``ConformerPPG.streaming_recognizer``) whose
        ``partial_text()`` / ``finish_text()`` detokenise as ``transcribe`` does."""
        rec = self.model.streaming_recognizer(**kw)
        rec.detokenize = self._text
        return rec

    def transcribe_stream(self, chunks, sr: int = 16000, mode: str = "ctc_prefix_beam_search", ctc_weight: float = 0.5,
                          reverse_weight: float = 0.0, **kw):
        """A generator over ``chunks``, an iterable of 16 kHz mono sample blocks: the partial text after every block, then
        the final text (``mode``: ``ctc_prefix_beam_search`` or ``attention_rescoring``).  ``kw``: the keywords of
        ``stream``.  The arguments are checked, and the recogniser is built, when this is called, not at the first
        ``next``."""
        from .streaming_asr import STREAM_MODES, check_sample_rate
        check_sample_rate(sr)
        if mode not in STREAM_MODES:
            raise _C.F5EError(f"CTCAligner.transcribe_stream: unknown mode {mode!r} (one of {', '.join(STREAM_MODES)})")
        rec = self.stream(**kw)

        def run():
            for block in chunks:
                rec.accept_waveform(block)
                yield rec.partial_text()
            yield rec.finish_text(mode, ctc_weight, reverse_weight)
        return run()

    @torch.no_grad()
    def align(self, audio, sr: Optional[int], text: str) -> List[WordSpan]:
        words, ids = self.tokenize(text)
        labels = [i for row in ids for i in row]
        if not labels:
            raise ValueError("CTCAligner.align: no character of the text is in the symbol table")
        feats, lens, secs = self._feats(audio, sr)
        al = self.model.ctc_forced_align(feats, lens, [labels])       # host ids and lengths: validated there (F5EError)
        if int(al.align[0, 0]) < 0:                                   # the kernel's "no path" row: never build spans from it
            raise _C.F5EError("CTCAligner.align: the text has no CTC path through this recording")
        return word_spans(words, ids, al.tok_end[0].cpu().tolist(), int(al.frame_lens[0]), frame_s=self.frame_s,
                          total_s=secs)

    def warm(self) -> None:
        """Build what the first call would build lazily (the model's engine, the fbank's device buffers), on the calling
        thread: worker threads that share this object then find it ready."""
        self.model.engine()
        if self.featCal.window.device.type != "cuda":
            self.featCal.to(self.device)

    def _labels(self, text: str, name: str) -> List[int]:
        labels = [i for row in self.tokenize(text)[1] for i in row]
        if not labels:
            raise ValueError(f"CTCAligner.{name}: no character of the text is in the symbol table")
        return labels

    @torch.no_grad()
    def score(self, audio, sr: Optional[int], text: str, use_linear: bool = False) -> float:
        """log P(text | audio) in nats: the sum over ALL CTC paths of the text's tokens (``ConformerPPG.ctc_loss`` negated;
        ``align`` gives the best single path).  -inf when the text has no path through the recording.  ``use_linear`` as in
        ``ConformerPPG.ctc_greedy_search``: False scores what the reference decodes with, True what the CTC head was
        trained on."""
        labels = self._labels(text, "score")
        feats, lens, _ = self._feats(audio, sr)
        logits, frame_lens, _ = self.model._ctc_scores(feats, lens, use_linear)
        return float(self._logp(logits, frame_lens, labels)[0])

    def _logp(self, logits, frame_lens, labels: List[int]) -> torch.Tensor:
        from .. import ops
        N = logits.shape[0]
        lab = torch.tensor([labels], dtype=torch.int32, device=logits.device).expand(N, -1).contiguous()
        l_len = torch.full((N,), len(labels), dtype=torch.int32, device=logits.device)
        return ops.ctc_loss(logits, lab, frame_lens, l_len, blank=0)

    @torch.no_grad()
    def score_batch(self, waves: torch.Tensor, sr: int, text: str, use_linear: bool = False) -> torch.Tensor:
        """``score`` for N waveforms of one length against ONE text: waves f32 [N, n] on the device -> log-likelihoods f32
        [N] on the device (nothing is copied to the host: the caller decides when to wait).  One pass: device resampler,
        fbank, the encoder at batch N, f5e_ctc_loss.  This method is the scorer protocol of
        ``infer.utils_infer.infer_batch_process(best_of=N, scorer=...)``: any object that has it can rank candidates."""
        from ..infer import audio as A
        if not (torch.is_tensor(waves) and waves.ndim == 2 and waves.is_cuda):
            raise _C.F5EError("CTCAligner.score_batch: waves must be a GPU tensor [N, n]; there is no CPU path")
        labels = self._labels(text, "score_batch")
        audio = A.resample_device(waves.to(torch.float32), sr, 16000)
        feats, _ = self.featCal(audio)                                # equal lengths: every row has all the frames
        lens = torch.full((feats.shape[0],), feats.shape[1], dtype=torch.int64)   # host values, as the encoder wants them
        logits, frame_lens, _ = self.model._ctc_scores(feats, lens, use_linear)
        return self._logp(logits, frame_lens, labels)
