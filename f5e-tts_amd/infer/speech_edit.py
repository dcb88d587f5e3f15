"""Speech editing (mirror of reference infer/speech_edit.py): re-synthesise chosen spans of a recording through
``CFM.sample(edit_mask=...)`` and keep the rest of it.  The reference is a script with its settings typed in at the top and
``parts_to_edit`` measured by hand with an outside forced aligner; here the recipe is a function, the settings are flags and
the parts can come from the project's own aligner (``ppg.ctc_align.CTCAligner``: the ASR model's CTC head, searched on the
device) by diffing the word lists of the original and the target text.

``plan_edit`` is the reference's audio / mask assembly (speech_edit.py:141-160) as pure host arithmetic; ``diff_parts`` maps
aligned words to parts; ``speech_edit_process`` is the script's body (:131-201)."""
from __future__ import annotations

import argparse
import difflib
import os
from typing import List, Optional, Sequence, Tuple

import torch

from . import utils_infer as U


def plan_edit(n_samples: int, sr: int, hop_length: int, parts_to_edit: Sequence[Sequence[float]],
              fix_duration: Optional[Sequence[float]] = None) -> Tuple[List[Tuple[str, int, int]], List[bool]]:
    """The reference's loop (speech_edit.py:141-160) on numbers instead of tensors -> (pieces, edit_mask).

    pieces: ("keep", a, b) = samples [a, b) of the recording (Python slice rules, as ``audio[:, a:b]``), ("zeros", 0, n) = n
    zero samples for a part to generate, in output order.  edit_mask: one bool per mel frame, True = keep the recording:
    per part ``round((start - offset) / hop)`` True frames and ``round(part_dur / hop)`` False frames, then True up to
    ``n // hop + 1`` frames of the assembled audio (a negative pad truncates, as F.pad does).  ``fix_duration`` gives a
    duration per part in seconds; None keeps every part's own."""
    fix = list(fix_duration) if fix_duration is not None else None
    if fix is not None and len(fix) < len(parts_to_edit):
        raise ValueError(f"fix_duration has {len(fix)} entries for {len(parts_to_edit)} parts")
    pieces: List[Tuple[str, int, int]] = []
    mask: List[bool] = []
    offset, total = 0, 0

    def keep(a: int, b: int) -> int:
        a, b = min(max(a, 0), n_samples), min(max(b, 0), n_samples)
        pieces.append(("keep", a, max(a, b)))
        return max(0, b - a)

    for start, end in parts_to_edit:
        part_dur = (end - start) if fix is None else fix.pop(0)
        part_dur = part_dur * sr
        start = start * sr
        total += keep(round(offset), round(start))
        pieces.append(("zeros", 0, round(part_dur)))
        total += round(part_dur)
        mask += [True] * round((start - offset) / hop_length) + [False] * round(part_dur / hop_length)
        offset = end * sr
    total += keep(round(offset), n_samples)
    want = total // hop_length + 1
    mask = mask[:want] + [True] * (want - len(mask))
    return pieces, mask


def assemble(audio: torch.Tensor, pieces) -> torch.Tensor:
    """audio [1, n] -> the recording with every part to edit replaced by its run of zeros."""
    parts = [audio[:, a:b] if kind == "keep" else audio.new_zeros(1, b) for kind, a, b in pieces]
    return torch.cat(parts, dim=-1)


def diff_parts(spans, target_words: Sequence[str], fix_duration: Optional[Sequence[float]] = None):
    """Word spans of the ORIGINAL text (``WordSpan(word, start_s, end_s)``) and the word list of the target -> (parts,
    fix_duration).  Every non-equal opcode of ``difflib.SequenceMatcher`` over the two word lists is one part, from the start
    of its first original word to the end of its last.  A pure insertion has no original words: it becomes an empty part at
    the edge between its neighbours and needs a ``fix_duration`` (else ValueError)."""
    origin = [s.word for s in spans]
    ops = [op for op in difflib.SequenceMatcher(a=origin, b=list(target_words), autojunk=False).get_opcodes()
           if op[0] != "equal"]
    if fix_duration is not None and len(fix_duration) != len(ops):
        raise ValueError(f"fix_duration has {len(fix_duration)} entries, the texts differ in {len(ops)} places")
    parts = []
    for tag, i1, i2, _j1, _j2 in ops:
        if tag == "insert":
            if fix_duration is None:
                raise ValueError("the target text inserts words where the original has none: give fix_duration "
                                 "(seconds per edited part)")
            edge = spans[i1].start_s if i1 < len(spans) else spans[-1].end_s
            parts.append([edge, edge])
        else:
            parts.append([spans[i1].start_s, spans[i2 - 1].end_s])
    return parts, (list(fix_duration) if fix_duration is not None else None)


def speech_edit_process(audio_to_edit, origin_text: str, target_text: str, model_obj, vocoder, parts_to_edit=None,
                        fix_duration=None, aligner=None, mel_spec_type=U.mel_spec_type, nfe_step=U.nfe_step,
                        cfg_strength=U.cfg_strength, sway_sampling_coef=U.sway_sampling_coef, seed=None,
                        target_rms=U.target_rms, device=None):
    """``audio_to_edit``: a wav path or (wave [channels, n], rate) -> (wave f32 [n'] on the host, 24000, mel [100, frames]).
    ``parts_to_edit``: [[start_s, end_s], ...] of the recording, in order; None = derive them with ``aligner``
    (``align(audio, sr, text) -> [WordSpan]``) from the difference between ``origin_text`` and ``target_text``."""
    audio, sr = U.load_wav(audio_to_edit) if isinstance(audio_to_edit, str) else audio_to_edit
    device = device or next(model_obj.parameters()).device
    audio = U._mono(audio)
    if parts_to_edit is None:
        if aligner is None:
            raise ValueError("speech_edit_process needs parts_to_edit or an aligner to find them")
        from ..ppg.ctc_align import split_words
        spans = aligner.align(audio, sr, origin_text)
        parts_to_edit, fix_duration = diff_parts(spans, split_words(target_text), fix_duration)
    rms = torch.sqrt(torch.mean(torch.square(audio)))
    quiet = bool(rms < target_rms)
    audio = audio.to(device, torch.float32)
    rms = rms.to(device)
    hop = U.hop_length
    with torch.inference_mode():
        if quiet:
            audio = audio * target_rms / rms
        audio = U.A.resample_device(audio, sr, U.target_sample_rate)
        pieces, mask = plan_edit(audio.shape[-1], U.target_sample_rate, hop, parts_to_edit, fix_duration)
        audio = assemble(audio, pieces)
        edit_mask = torch.tensor([mask], dtype=torch.bool, device=device)
        text_list = U.convert_char_to_pinyin([target_text])
        duration = audio.shape[-1] // hop
        generated, _traj = model_obj.sample(cond=audio, text=text_list, duration=duration, steps=nfe_step,
                                            cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, seed=seed,
                                            edit_mask=edit_mask)
        del _traj
        mel = generated.to(torch.float32).permute(0, 2, 1)
        wave_ = vocoder.decode(mel) if mel_spec_type == "vocos" else vocoder(mel)
        if quiet:
            wave_ = wave_ * rms / target_rms
    return wave_.squeeze().cpu().numpy(), U.target_sample_rate, mel[0].cpu().numpy()


def _pairs(text: str) -> List[List[float]]:
    return [[float(v) for v in item.split("-")] for item in text.split(",") if item.strip()]


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python3 -m f5e_tts_amd.infer.speech_edit",
                                description="Re-synthesise parts of a recording (speech editing).")
    p.add_argument("--audio", type=str, required=True, help="The recording to edit")
    p.add_argument("--origin_text", type=str, required=True, help="What the recording says")
    p.add_argument("--target_text", type=str, required=True, help="What it should say")
    p.add_argument("--parts", type=str, default="", help='Spans to replace, in seconds: "1.42-2.44,4.04-4.9" '
                                                         "(default: found by aligning --origin_text with --asr_model)")
    p.add_argument("--fix_duration", type=str, default="", help='Seconds per replaced span: "1.2,1" (default: the span\'s own)')
    p.add_argument("--asr_model", type=str, help="ASR checkpoint with a CTC head (the PPG extractor's model)")
    p.add_argument("--asr_config", type=str, help="Its train.yaml")
    p.add_argument("--asr_dict", type=str, help="Its symbol table (`token id` lines)")
    p.add_argument("--whisper_dir", type=str, help="A local Whisper model directory: find the spans from its word timestamps "
                                                   "instead (needs alignment_heads in its generation_config.json)")
    p.add_argument("--whisper_language", type=str, default="en", help="The recording's language, for --whisper_dir")
    p.add_argument("--whisper_beam", type=int, default=1, help="Beam size of the --whisper_dir transcription (1: greedy)")
    p.add_argument("--whisper_weights", type=str, choices=("f32", "fp16", "bf16", "auto"), default="f32",
                   help="The type the --whisper_dir model's matrices are held in on the device (fp16 / bf16: half the memory; auto: "
                        "the type the checkpoint stores)")
    p.add_argument("-m", "--model", type=str, default="F5TTS_v1_Base", help="The model name")
    p.add_argument("-mc", "--model_cfg", type=str, default="", help="The path to the model config file .yaml")
    p.add_argument("-p", "--ckpt_file", type=str, required=True, help="The path to model checkpoint .pt/.safetensors")
    p.add_argument("-v", "--vocab_file", type=str, default="", help="The path to vocab file .txt")
    p.add_argument("--vocoder_name", type=str, choices=["vocos", "bigvgan"], default=U.mel_spec_type)
    p.add_argument("--vocoder_local_path", type=str, default="", help="The vocoder's directory")
    p.add_argument("--nfe_step", type=int, default=U.nfe_step)
    p.add_argument("--cfg_strength", type=float, default=U.cfg_strength)
    p.add_argument("--sway_sampling_coef", type=float, default=U.sway_sampling_coef)
    p.add_argument("--target_rms", type=float, default=U.target_rms)
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--device", type=str, default=U.device)
    p.add_argument("-o", "--output", type=str, default="tests/speech_edit_out.wav", help="The wav to write")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    parts = _pairs(args.parts) if args.parts else None
    if parts is not None and any(len(p) != 2 for p in parts):
        raise SystemExit('--parts: "start-end,start-end" in seconds')
    fix = [float(v) for v in args.fix_duration.split(",") if v.strip()] if args.fix_duration else None
    wenet = bool(args.asr_model and args.asr_config and args.asr_dict)
    if wenet and args.whisper_dir:
        raise SystemExit("give one aligner: --asr_model / --asr_config / --asr_dict, or --whisper_dir")
    if parts is None and not wenet and not args.whisper_dir:
        raise SystemExit("give --parts, or --asr_model / --asr_config / --asr_dict (or --whisper_dir) to find them")
    from ..model import DiT
    from .infer_cli import DEFAULT_VOCODER_PATH, load_arch
    vocoder = U.load_vocoder(args.vocoder_name, is_local=True,
                             local_path=args.vocoder_local_path or DEFAULT_VOCODER_PATH[args.vocoder_name],
                             device=args.device)
    model = U.load_model(DiT, load_arch(args.model, args.model_cfg), args.ckpt_file, mel_spec_type=args.vocoder_name,
                         vocab_file=args.vocab_file, device=args.device)
    aligner = None
    if parts is None and wenet:
        from ..ppg.ctc_align import CTCAligner
        aligner = CTCAligner(args.asr_model, args.asr_config, args.asr_dict, args.device, asr=True)
    elif parts is None:
        from ..eval.whisper import WhisperRecognizer
        aligner = WhisperRecognizer(args.whisper_dir, args.device, args.whisper_language, args.whisper_beam,
                                    **({} if args.whisper_weights == "f32" else dict(weights=args.whisper_weights)))
    wave, sr, _mel = speech_edit_process(args.audio, args.origin_text, args.target_text, model, vocoder,
                                         parts_to_edit=parts, fix_duration=fix, aligner=aligner,
                                         mel_spec_type=args.vocoder_name, nfe_step=args.nfe_step,
                                         cfg_strength=args.cfg_strength, sway_sampling_coef=args.sway_sampling_coef,
                                         seed=args.seed, target_rms=args.target_rms, device=args.device)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    U.save_wav(args.output, wave, sr)
    print(args.output)


if __name__ == "__main__":
    main()
