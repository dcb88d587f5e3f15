"""Callers of the hot path (mirror of reference infer/utils_infer.py): checkpoint/model/vocoder loading and
``infer_process`` / ``infer_batch_process`` with the reference's argument names, defaults and duration / RMS /
cross-fade rules.  Everything between ``model_obj.sample`` and ``vocoder.decode`` runs on libf5e_hip.so; what is left
here is host glue (text chunking, wav I/O, numpy cross-fade) exactly as in the reference.  ``infer_vc_process`` is the
voice-conversion counterpart (PPG models, ``sample_vc``), which the reference only offers as an eval driver.

Resampling and the pydub-style silence clipping live in ``infer/audio.py``.  The Whisper ASR fallback of
``preprocess_ref_audio_text`` is opt-in: hand it a ``transcriber`` (``eval.whisper.WhisperRecognizer``); without one an empty
``ref_text`` is an error.  Not rebuilt (out of scope): HF-hub downloads (no network).  Chinese g2p needs the optional ``jieba`` + ``pypinyin`` packages;
the ASCII path is self-contained.
"""
from __future__ import annotations

import hashlib
import math
import os
import re
import tempfile
import wave
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Tuple

import numpy as np
import torch

from ..model import CFM
from ..model.utils import get_tokenizer
from ..vocoder import Vocos, load_vocos
from ..vocoder_bigvgan import load_bigvgan
from . import audio as A

# ----------------------------------------- defaults (reference infer/utils_infer.py:49-62)
device = "cuda" if torch.cuda.is_available() else "cpu"
target_sample_rate = 24000
n_mel_channels = 100
hop_length = 256
win_length = 1024
n_fft = 1024
mel_spec_type = "vocos"
target_rms = 0.1
cross_fade_duration = 0.15
ode_method = "euler"
nfe_step = 32
cfg_strength = 2.0
sway_sampling_coef = -1.0
speed = 1.0
fix_duration = None

_DEFAULT_VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "examples", "vocab.txt")


# ----------------------------------------- text front-end

def chunk_text(text: str, max_chars: int = 135) -> List[str]:
    """Sentence-wise greedy packing into chunks of at most ``max_chars`` UTF-8 bytes (reference utils_infer.py:70-97):
    split after ``;:,.!?`` followed by whitespace, or after a full-width ``；：，。！？``; a sentence ending in a
    single-byte character gets a trailing space when appended."""
    pieces = re.split(r"(?<=[;:,.!?])\s+|(?<=[；：，。！？])", text)
    chunks: List[str] = []
    cur = ""
    for sent in pieces:
        add = sent + " " if sent and len(sent[-1].encode("utf-8")) == 1 else sent
        if len(cur.encode("utf-8")) + len(sent.encode("utf-8")) <= max_chars:
            cur += add
        else:
            if cur:
                chunks.append(cur.strip())
            cur = add
    if cur:
        chunks.append(cur.strip())
    return chunks


_ASCII_TOKEN = re.compile(r"[A-Za-z0-9]+|.", re.DOTALL)
_OOV_TRANS = str.maketrans({";": ",", "“": '"', "”": '"', "‘": "'", "’": "'"})


def convert_char_to_pinyin(text_list: List[str], polyphone: bool = True) -> List[List[str]]:
    """Character/pinyin tokeniser (reference model/utils.py:270-311).  For single-byte text jieba yields alphanumeric
    runs and single other characters; that segmentation is restated here, so ASCII needs no third-party package.
    Text with multi-byte characters defers to jieba + pypinyin when they are installed."""
    out = []
    for text in text_list:
        text = text.translate(_OOV_TRANS)
        if all(ord(c) < 128 for c in text):
            chars: List[str] = []
            for seg in _ASCII_TOKEN.findall(text):
                if chars and len(seg) > 1 and chars[-1] not in " :'\"":
                    chars.append(" ")
                chars.extend(seg)
            out.append(chars)
            continue
        try:
            import jieba
            from pypinyin import Style, lazy_pinyin
        except ImportError as e:  # pragma: no cover - optional dependency
            raise RuntimeError("non-ASCII text needs the optional jieba + pypinyin packages (SURVEY f1)") from e
        chars = []
        for seg in jieba.cut(text):
            nb = len(seg.encode("utf-8"))
            if nb == len(seg):
                if chars and nb > 1 and chars[-1] not in " :'\"":
                    chars.append(" ")
                chars.extend(seg)
            elif polyphone and nb == 3 * len(seg):
                py = lazy_pinyin(seg, style=Style.TONE3, tone_sandhi=True)
                for i, c in enumerate(seg):
                    if "㄀" <= c <= "鿿":
                        chars.append(" ")
                    chars.append(py[i])
            else:
                for c in seg:
                    if ord(c) < 256:
                        chars.extend(c)
                    elif "㄀" <= c <= "鿿":
                        chars.append(" ")
                        chars.extend(lazy_pinyin(c, style=Style.TONE3, tone_sandhi=True))
                    else:
                        chars.append(c)
        out.append(chars)
    return out


# ----------------------------------------- loading (reference utils_infer.py:101-271)

def load_vocoder(vocoder_name="vocos", is_local=False, local_path="", device=device, hf_cache_dir=None):
    if vocoder_name not in ("vocos", "bigvgan"):
        raise NotImplementedError(f"unknown vocoder {vocoder_name!r} (vocos / bigvgan)")
    if not is_local:
        raise RuntimeError(f"no network access: pass is_local=True and local_path=<{vocoder_name} checkpoint directory>")
    if vocoder_name == "bigvgan":   # config.json + bigvgan_generator.pt (reference utils_infer.py:125-138)
        return load_bigvgan(local_path, device)
    return load_vocos(local_path, device)


def load_checkpoint(model, ckpt_path: str, device: str, dtype=None, use_ema=True):
    """EMA prefix strip, bookkeeping/legacy key drops and strict load as in reference utils_infer.py:185-227.
    The module keeps fp32 master weights whatever ``dtype`` says: the HIP engine makes its own bf16 repack (the
    reference's fp16 cast would degrade the RoPE / time tables)."""
    ckpt_type = ckpt_path.split(".")[-1]
    if ckpt_type == "safetensors":
        from safetensors.torch import load_file
        checkpoint = load_file(ckpt_path, device="cpu")
    else:
        checkpoint = torch.load(ckpt_path, map_location="cpu", weights_only=True)
    if use_ema:
        if ckpt_type == "safetensors":
            checkpoint = {"ema_model_state_dict": checkpoint}
        state = {k.replace("ema_model.", ""): v for k, v in checkpoint["ema_model_state_dict"].items()
                 if k not in ("initted", "step")}
        for legacy in ("mel_spec.mel_stft.mel_scale.fb", "mel_spec.mel_stft.spectrogram.window"):
            state.pop(legacy, None)
    else:
        if ckpt_type == "safetensors":
            checkpoint = {"model_state_dict": checkpoint}
        state = checkpoint["model_state_dict"]
    model.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in state.items()})
    return model.to(device)


def load_model(model_cls, model_cfg, ckpt_path, mel_spec_type=mel_spec_type, vocab_file="", ode_method=ode_method,
               use_ema=True, device=device, ppg_config=None, cb_config=None):
    """``ppg_config`` / ``cb_config``: (backbone dict, CFM dict) pairs of a PPG / codebook model, as
    ``train.parse_cfg.parse_model_yaml`` splits them (``infer_cli.load_model_config``); the reference's load_model has no
    way to build such a model.  None = the plain model, exactly as before."""
    if vocab_file == "":
        vocab_file = _DEFAULT_VOCAB
    vocab_char_map, vocab_size = get_tokenizer(vocab_file)
    dit_kw, cfm_kw = {}, {}
    for name, pair in (("ppg_config", ppg_config), ("cb_config", cb_config)):
        if pair is not None:
            dit_kw[name], cfm_kw[name] = pair
    model = CFM(
        transformer=model_cls(**model_cfg, text_num_embeds=vocab_size, mel_dim=n_mel_channels, **dit_kw),
        mel_spec_kwargs=dict(n_fft=n_fft, hop_length=hop_length, win_length=win_length,
                             n_mel_channels=n_mel_channels, target_sample_rate=target_sample_rate,
                             mel_spec_type=mel_spec_type),
        odeint_kwargs=dict(method=ode_method), vocab_char_map=vocab_char_map, **cfm_kw).to(device)
    if ckpt_path:
        model = load_checkpoint(model, ckpt_path, device, use_ema=use_ema)
    return model


# ----------------------------------------- audio I/O (stdlib wave instead of torchaudio/soundfile)

def load_wav(path: str) -> Tuple[torch.Tensor, int]:
    """PCM16 / PCM32 / float32 RIFF -> (float32 [channels, n], sample_rate)."""
    with wave.open(path, "rb") as w:
        nch, sw, sr, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(n)
    if sw == 2:
        data = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif sw == 4:
        data = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    else:
        raise ValueError(f"unsupported sample width {sw}")
    return torch.from_numpy(data.reshape(-1, nch).T.copy()), sr


def save_wav(path: str, audio: np.ndarray, sr: int) -> None:
    pcm = np.clip(np.asarray(audio, dtype=np.float64), -1.0, 1.0)
    pcm = (pcm * 32767.0).round().astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.tobytes())


def _read_segment(path: str) -> A.Segment:
    wav, sr = load_wav(path)
    return A.Segment.from_float(wav.numpy(), sr)


def _write_segment(path: str, seg: A.Segment) -> None:
    with wave.open(path, "wb") as w:
        w.setnchannels(seg.pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(seg.rate)
        w.writeframes(np.ascontiguousarray(seg.pcm, dtype="<i2").tobytes())


_ref_audio_cache = {}


def preprocess_ref_audio_text(ref_audio_orig, ref_text, clip_short=True, show_info=print, transcriber=None):
    """Reference infer/utils_infer.py:293-352: clip the clip to <= 12 s at silences, strip silent edges, add 50 ms of
    silence, write a temporary wav; make ref_text end in ". ".  Returns (wav path, ref_text).  ``transcriber``: anything with
    ``transcribe(wav_path) -> str`` (an ``eval.whisper.WhisperRecognizer``); with one, an empty ``ref_text`` is replaced by
    the transcript of the clipped prompt, as the reference does with whisper-large-v3-turbo (:148-179, :341)."""
    show_info("Converting audio...")
    seg = A.clip_reference(_read_segment(ref_audio_orig), clip_short=clip_short, note=show_info)
    with tempfile.NamedTemporaryFile(delete=False, suffix=".wav") as f:
        ref_audio = f.name
    _write_segment(ref_audio, seg)
    with open(ref_audio, "rb") as fh:
        audio_hash = hashlib.md5(fh.read()).hexdigest()
    if not ref_text.strip():
        if audio_hash in _ref_audio_cache:
            show_info("Using cached reference text...")
            ref_text = _ref_audio_cache[audio_hash]
        elif transcriber is not None:
            show_info("No reference text provided, transcribing reference audio...")
            _ref_audio_cache[audio_hash] = ref_text = transcriber.transcribe(ref_audio).strip()
        else:
            raise ValueError("ref_text is empty: the reference falls back to Whisper ASR here (utils_infer.py:341), "
                             "which is outside this build; pass the transcript of the reference audio")
    else:
        show_info("Using custom reference text...")
    if not ref_text.endswith(". ") and not ref_text.endswith("\u3002"):
        ref_text += " " if ref_text.endswith(".") else ". "
    return ref_audio, ref_text


def remove_silence_for_generated_wav(filename):
    """Reference infer/utils_infer.py:567-575."""
    _write_segment(filename, A.strip_generated_silence(_read_segment(filename)))


def cross_fade_concat(waves: List[np.ndarray], cross_fade_duration: float, sr: int = target_sample_rate) -> np.ndarray:
    """Linear cross-fade between consecutive chunk waves (reference utils_infer.py:520-556)."""
    if cross_fade_duration <= 0:
        return np.concatenate(waves)
    final = waves[0]
    for nxt in waves[1:]:
        n = min(int(cross_fade_duration * sr), len(final), len(nxt))
        if n <= 0:
            final = np.concatenate([final, nxt])
            continue
        mix = final[-n:] * np.linspace(1, 0, n) + nxt[:n] * np.linspace(0, 1, n)
        final = np.concatenate([final[:-n], mix, nxt[n:]])
    return final


# ----------------------------------------- inference drivers (reference utils_infer.py:367-565)

def plan_batch(ref_audio_len: int, ref_text: str, gen_text: str, speed_: float, fix_duration_) -> Tuple[int, float]:
    """Duration heuristic of process_batch (reference utils_infer.py:455-471) -> (duration in frames, speed used)."""
    local_speed = 0.3 if len(gen_text.encode("utf-8")) < 10 else speed_
    if fix_duration_ is not None:
        return int(fix_duration_ * target_sample_rate / hop_length), local_speed
    ref_text_len = len(ref_text.encode("utf-8"))
    gen_text_len = len(gen_text.encode("utf-8"))
    return ref_audio_len + int(ref_audio_len / ref_text_len * gen_text_len / local_speed), local_speed


def pick_best(scores) -> int:
    """Index of the first maximum among the finite scores; NaN and -inf rank last; 0 when no score is finite."""
    best, at = None, 0
    for i, v in enumerate(scores):
        if math.isfinite(v) and (best is None or v > best):
            best, at = v, i
    return at


def infer_batch_process(ref_audio, ref_text, gen_text_batches, model_obj, vocoder, mel_spec_type="vocos", progress=None,
                        target_rms=0.1, cross_fade_duration=0.15, nfe_step=32, cfg_strength=2.0,
                        sway_sampling_coef=-1, speed=1, fix_duration=None, device=None, streaming=False,
                        chunk_size=2048, mode="cfg", alpha_spk=2.5, alpha_txt=3.0, best_of=1, scorer=None, seed=None,
                        report=None):
    """Generator like the reference's: yields (final_wave, sample_rate, combined_spectrogram) or, when streaming,
    (chunk, sample_rate) pieces.  mode "tts" (PPG / codebook models): ``sample_tts`` with alpha_spk / alpha_txt in place
    of ``sample`` with cfg_strength (reference eval_infer_batch_tts.py:203-214).

    Best-of-N (beyond the reference; off by default): ``best_of=N`` draws N candidates per text chunk, each its own batch-1
    call with its own seed (one batch would be N copies: the sampler seeds every batch item alike), scores the N waveforms
    in ONE ``scorer.score_batch(stack [N, n], 24000, gen_text)`` call against the chunk's own text (``ppg.ctc_align.
    CTCAligner`` is such a scorer: log P(text | audio) under the ASR model's CTC head) and keeps the first maximum; NaN and
    -inf rank last, and candidate 0 stays when no score is finite.  ``seed``: candidate i of chunk c runs with seed + c *
    best_of + i; None draws the seeds from the global CPU generator on the calling thread, in submission order.
    ``report``: a list that receives one dict per chunk, {"seeds", "scores", "chosen"}."""
    if mode not in ("cfg", "tts"):
        raise ValueError(f"infer_batch_process: mode {mode!r} (cfg / tts; voice conversion is infer_vc_process)")
    best_of = int(best_of)
    if best_of < 1:
        raise ValueError(f"infer_batch_process: best_of must be at least 1 (got {best_of})")
    if best_of > 1 and (scorer is None or not hasattr(scorer, "score_batch")):
        raise ValueError("infer_batch_process: best_of > 1 needs a scorer with score_batch(waves, sr, text) "
                         "(ppg.ctc_align.CTCAligner)")
    audio, sr = ref_audio
    if audio.shape[0] > 1:
        audio = torch.mean(audio, dim=0, keepdim=True)
    rms = torch.sqrt(torch.mean(torch.square(audio)))
    if rms < target_rms:
        audio = audio * target_rms / rms
    if sr != target_sample_rate:
        audio = A.resample(audio, sr, target_sample_rate)
    audio = audio.to(device)
    if len(ref_text[-1].encode("utf-8")) == 1:
        ref_text = ref_text + " "

    def process_batch(gen_text, seed=None):
        """Queues one chunk on the GPU and returns DEVICE tensors: nothing here waits for the GPU, so the host prep of
        the next chunk overlaps this chunk's ODE loop; the caller copies to the host afterwards."""
        text_list = convert_char_to_pinyin([ref_text + gen_text])
        ref_audio_len = audio.shape[-1] // hop_length
        duration, _ = plan_batch(ref_audio_len, ref_text, gen_text, speed, fix_duration)
        with torch.inference_mode():
            if mode == "tts":
                generated, _traj = model_obj.sample_tts(cond=audio, text=text_list, duration=duration, steps=nfe_step,
                                                        alpha_spk=alpha_spk, alpha_txt=alpha_txt,
                                                        sway_sampling_coef=sway_sampling_coef, seed=seed)
            else:
                generated, _traj = model_obj.sample(cond=audio, text=text_list, duration=duration, steps=nfe_step,
                                                    cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef,
                                                    seed=seed)
            del _traj
            generated = generated.to(torch.float32)[:, ref_audio_len:, :].permute(0, 2, 1)
            # reference utils_infer.py:488-491: Vocos.decode -> [b, n], BigVGAN's forward -> [b, 1, n]
            wave_ = vocoder.decode(generated) if mel_spec_type == "vocos" else vocoder(generated)
            if rms < target_rms:
                wave_ = wave_ * rms / target_rms
            return wave_, generated

    def to_host(res):
        wave_, generated = res
        return wave_.squeeze().cpu().numpy(), generated[0].cpu().numpy()

    def draw_seed():
        return int(torch.randint(0, 2 ** 31 - 1, (1,)).item())

    def best_of_n(gen_text, seeds):
        """N candidates of one chunk, one scorer call, the first maximum -> (what ``process_batch`` returns for the winner,
        the chunk's report entry)."""
        cands = [process_batch(gen_text, seed=s) for s in seeds]
        stack = torch.stack([w.reshape(-1) for w, _ in cands]).to(torch.float32)
        scores = [float(v) for v in torch.as_tensor(scorer.score_batch(stack, target_sample_rate, gen_text)).reshape(-1).tolist()]
        chosen = pick_best(scores)
        return cands[chosen], {"seeds": list(seeds), "scores": scores, "chosen": chosen}

    # plain: the call that always existed, process_batch(gen_text) with the sampler's own noise draw; otherwise every
    # candidate's seed is fixed here, on the calling thread, before any chunk runs
    plain = best_of == 1 and seed is None
    if not plain:
        chunk_seeds = [[seed + c * best_of + i if seed is not None else draw_seed() for i in range(best_of)]
                       for c in range(len(gen_text_batches))]

    def run_chunk(c):
        """-> (chunk c on the host, its report entry or None); callable from a worker thread: it touches no shared state."""
        if plain:
            return to_host(process_batch(gen_text_batches[c])), None
        if best_of == 1:
            return (to_host(process_batch(gen_text_batches[c], seed=chunk_seeds[c][0])),
                    {"seeds": list(chunk_seeds[c]), "scores": [], "chosen": 0})
        res, entry = best_of_n(gen_text_batches[c], chunk_seeds[c])
        return to_host(res), entry

    def note(entry):
        """The report grows on the calling thread, in chunk order."""
        if report is not None and entry is not None:
            report.append(entry)

    if streaming:
        for c in range(len(gen_text_batches)):
            (w, _), entry = run_chunk(c)
            note(entry)
            for j in range(0, len(w), chunk_size):
                yield w[j: j + chunk_size], target_sample_rate
        return
    # The reference submits process_batch to a ThreadPoolExecutor (utils_infer.py:511), but process_batch is a generator
    # function there: submit() only creates the generator, and the chunks then run ONE AT A TIME, in order, in the consumer
    # loop (`next(result)`, :514-518).  Default here = the same order on the calling thread, so with seed=None the noise
    # of chunk i is the i-th draw from the global CPU generator exactly as in the reference (reproducible under
    # torch.manual_seed); the GPU still overlaps chunks with the host because nothing above waits for it.
    # F5E_INFER_WORKERS=k (2..4) opts into k host threads, each on its own stream (the engine keeps
    # per-call buffers private per thread): more throughput on one GPU, and a per-chunk seed drawn in submission order on
    # this thread keeps the result independent of thread timing (a different noise stream than the serial default).
    workers = max(1, min(4, int(os.environ.get("F5E_INFER_WORKERS", "1"))))
    if workers == 1 or len(gen_text_batches) < 2:
        if plain:
            results = [to_host(r) for r in [process_batch(g) for g in gen_text_batches]]
        else:
            results = []
            for c in range(len(gen_text_batches)):
                res, entry = run_chunk(c)
                results.append(res)
                note(entry)
    else:
        # one work item per chunk, candidates included; a plain call draws its per-chunk seed here as it always did
        work = [(g, draw_seed()) for g in gen_text_batches] if plain else list(range(len(gen_text_batches)))
        import threading
        tls = threading.local()
        main_stream = torch.cuda.current_stream()
        if best_of > 1 and hasattr(scorer, "warm"):
            scorer.warm()                                  # build its engine once, here, not once per worker that gets there first

        def on_own_stream(a):
            # the samplers run on the caller's current stream: every worker brings its own, ordered behind this thread's
            if not hasattr(tls, "stream"):
                tls.stream = torch.cuda.Stream()
                tls.stream.wait_stream(main_stream)
            with torch.cuda.stream(tls.stream):
                return (to_host(process_batch(*a)), None) if plain else run_chunk(a)

        with ThreadPoolExecutor(max_workers=workers) as ex:
            done = list(ex.map(on_own_stream, work))       # in submission order, whichever worker finished first
        results = [res for res, _ in done]
        for _, entry in done:
            note(entry)
    waves = [r[0] for r in results]
    specs = [r[1] for r in results]
    if waves:
        yield cross_fade_concat(waves, cross_fade_duration), target_sample_rate, np.concatenate(specs, axis=1)
    else:
        yield None, target_sample_rate, None


def infer_process(ref_audio, ref_text, gen_text, model_obj, vocoder, mel_spec_type=mel_spec_type, show_info=print,
                  progress=None, target_rms=target_rms, cross_fade_duration=cross_fade_duration, nfe_step=nfe_step,
                  cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, speed=speed,
                  fix_duration=fix_duration, device=device, mode="cfg", alpha_spk=2.5, alpha_txt=3.0, best_of=1,
                  scorer=None, seed=None, report=None):
    audio, sr = load_wav(ref_audio)
    secs = audio.shape[-1] / sr
    max_chars = int(len(ref_text.encode("utf-8")) / secs * (22 - secs))
    gen_text_batches = chunk_text(gen_text, max_chars=max_chars)
    show_info(f"Generating audio in {len(gen_text_batches)} batches...")
    return next(infer_batch_process((audio, sr), ref_text, gen_text_batches, model_obj, vocoder,
                                    mel_spec_type=mel_spec_type, progress=progress, target_rms=target_rms,
                                    cross_fade_duration=cross_fade_duration, nfe_step=nfe_step,
                                    cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, speed=speed,
                                    fix_duration=fix_duration, device=device, mode=mode, alpha_spk=alpha_spk,
                                    alpha_txt=alpha_txt, best_of=best_of, scorer=scorer, seed=seed, report=report))


# ----------------------------------------- voice conversion (reference eval_infer_batch_vc.py:214-238, utils_eval.py:284-336)

max_total_secs = 22.0      # prompt + converted piece per sample_vc call: the budget infer_process gives a text chunk


def plan_vc_chunks(n_samples: int, sr: int, ref_secs: float, silences=(), max_total_secs: float = max_total_secs
                   ) -> List[Tuple[int, int]]:
    """Split a source of ``n_samples`` at ``sr`` into consecutive [start, end) pieces of at most
    ``max_total_secs - ref_secs`` seconds (the reference clamps prompt + source at 4096 frames and silently truncates).
    A piece that has to end before the source does is cut at the midpoint of the longest silence inside the last third of
    its window (``silences``: [start_ms, end_ms] pairs of ``audio.detect_silence``; the part of a silence inside that third
    is what counts), and at the window's end when there is none.  Pure host arithmetic."""
    budget = float(max_total_secs) - float(ref_secs)
    if budget < 1.0:
        raise ValueError(f"voice conversion: a {ref_secs:.2f} s prompt leaves {budget:.2f} s of the {max_total_secs:.1f} s "
                         "budget for the source; at least 1 s is needed (use a shorter prompt)")
    max_len = int(budget * sr)
    spans = [(int(a * sr / 1000.0), int(b * sr / 1000.0)) for a, b in silences]
    pieces, start = [], 0
    while n_samples - start > max_len:
        lo, hi = start + max_len - max_len // 3, start + max_len
        best = None
        for a, b in spans:
            a, b = max(a, lo), min(b, hi)
            if b > a and (best is None or b - a > best[1] - best[0]):
                best = (a, b)
        cut = (best[0] + best[1]) // 2 if best is not None else hi
        pieces.append((start, cut))
        start = cut
    if n_samples > start or not pieces:
        pieces.append((start, n_samples))
    return pieces


def _mono(audio: torch.Tensor) -> torch.Tensor:
    if audio.ndim == 1:
        audio = audio.unsqueeze(0)
    return torch.mean(audio, dim=0, keepdim=True) if audio.shape[0] > 1 else audio


def infer_vc_batch_process(ref_audio, source_audio, pieces, model_obj, vocoder, ppg_front, mel_spec_type="vocos",
                           target_rms=0.1, cross_fade_duration=0.15, nfe_step=32, alpha_spk=2.5, alpha_ppg=3.0,
                           sway_sampling_coef=-1, speed=1.0, seed=None, device=None):
    """Generator (one item, like ``infer_batch_process``): converts the ``pieces`` ([start, end) sample ranges) of
    ``source_audio`` = (wave [channels, n], rate) to the voice of ``ref_audio`` = (wave, rate), in order and with the same
    prompt, and yields (joined wave, 24000, joined mel [100, frames]).

    Per piece, what eval_infer_batch.py --mode vc does per utterance: prompt mel at 24 kHz (RMS-raised to ``target_rms``
    when quieter, undone after the vocoder), the PPG of [prompt ; piece] at 16 kHz (both from their own rates, unscaled),
    total = ref_len + int(n24_piece / hop / speed), ``sample_vc``, the frames after the prompt through the vocoder.  The
    audio goes to the device once; every rate conversion is ``audio.resample_device``."""
    audio, sr = ref_audio
    source, src_sr = source_audio
    audio, source = _mono(audio), _mono(source)
    rms = torch.sqrt(torch.mean(torch.square(audio)))
    quiet = bool(rms < target_rms)
    audio, source = audio.to(device, torch.float32), source.to(device, torch.float32)
    rms = rms.to(device)
    with torch.inference_mode():
        scaled = audio * target_rms / rms if quiet else audio
        audio24 = A.resample_device(scaled, sr, target_sample_rate)
        ref_len = audio24.shape[-1] // hop_length
        ref_mel = model_obj.mel_spec(audio24).permute(0, 2, 1)[:, :ref_len]
        prompt16 = A.resample_device(audio, sr, 16000)

    def process_piece(start, end):
        with torch.inference_mode():
            piece = source[:, start:end]
            full16 = torch.cat([prompt16, A.resample_device(piece, src_sr, 16000)], dim=1)
            ppg, _len = ppg_front.audio_to_ppg(full16, 16000)
            orig, new, _w, _t = A.resample_plan(src_sr, target_sample_rate)
            n24 = -(-new * (end - start) // orig)        # the resampler's output length for this piece
            total = ref_len + int(n24 / hop_length / speed)
            if total - ref_len < 2:                      # under two frames (a 20 ms tail after a cut): nothing to vocode
                return None
            generated, _traj = model_obj.sample_vc(cond=ref_mel, ppg=ppg.to(device), duration=torch.tensor([total]),
                                                   steps=nfe_step, alpha_spk=alpha_spk, alpha_ppg=alpha_ppg,
                                                   sway_sampling_coef=sway_sampling_coef, seed=seed)
            del _traj
            generated = generated.to(torch.float32)[:, ref_len:total, :].permute(0, 2, 1)
            wave_ = vocoder.decode(generated) if mel_spec_type == "vocos" else vocoder(generated)
            if quiet:
                wave_ = wave_ * rms / target_rms
            return wave_, generated

    # queued piece after piece on the caller's stream; the host copies come after the last piece is queued
    results = [r for r in (process_piece(a, b) for a, b in pieces) if r is not None]
    results = [(w.squeeze().cpu().numpy(), g[0].cpu().numpy()) for w, g in results]
    if results:
        yield (cross_fade_concat([r[0] for r in results], cross_fade_duration), target_sample_rate,
               np.concatenate([r[1] for r in results], axis=1))
    else:
        yield None, target_sample_rate, None


def infer_vc_process(ref_audio, source_audio, model_obj, vocoder, ppg_front, mel_spec_type=mel_spec_type,
                     show_info=print, target_rms=target_rms, cross_fade_duration=cross_fade_duration, nfe_step=nfe_step,
                     alpha_spk=2.5, alpha_ppg=3.0, sway_sampling_coef=sway_sampling_coef, speed=speed, seed=None,
                     max_total_secs=max_total_secs, device=device):
    """Voice conversion: the content of ``source_audio`` in the voice of ``ref_audio`` (wav paths, or (wave [channels, n],
    rate) pairs) -> (wave, 24000, mel), as ``infer_process`` returns them.  ``ppg_front``: any object with
    ``audio_to_ppg(audio [1, n] on the device, 16000) -> (ppg, len)`` (``ppg.PPGModelWapper``).  A source longer than
    ``max_total_secs`` minus the prompt is converted in pieces cut at silences (``plan_vc_chunks``) and cross-faded."""
    audio, sr = load_wav(ref_audio) if isinstance(ref_audio, str) else ref_audio
    source, src_sr = load_wav(source_audio) if isinstance(source_audio, str) else source_audio
    n = source.shape[-1]
    ref_secs = audio.shape[-1] / sr
    silences = []
    if n > int((max_total_secs - ref_secs) * src_sr) >= src_sr:      # only a source that needs cutting is searched
        seg = A.Segment.from_float(_mono(source).cpu().numpy(), src_sr)
        silences = A.detect_silence(seg, min_silence_len=100, silence_thresh=-40, seek_step=10)
    pieces = plan_vc_chunks(n, src_sr, ref_secs, silences, max_total_secs)
    show_info(f"Converting audio in {len(pieces)} pieces...")
    return next(infer_vc_batch_process((audio, sr), (source, src_sr), pieces, model_obj, vocoder, ppg_front,
                                       mel_spec_type=mel_spec_type, target_rms=target_rms,
                                       cross_fade_duration=cross_fade_duration, nfe_step=nfe_step, alpha_spk=alpha_spk,
                                       alpha_ppg=alpha_ppg, sway_sampling_coef=sway_sampling_coef, speed=speed, seed=seed,
                                       device=device))
