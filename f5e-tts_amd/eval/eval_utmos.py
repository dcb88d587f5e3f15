"""UTMOS driver: mirror of reference eval/eval_utmos.py, with the predictor of ``eval/utmos.py`` on the device.  Every file under
``--audio_dir`` with the extension ``--ext`` (searched recursively, in sorted order so that the output is stable) is read with
the project's stdlib wav reader, mixed down to mono, moved to the device and scored at its own sample rate (the predictor
resamples to 16 kHz there).  Written: ``<audio_dir>/_utmos_results.jsonl`` in the reference's format -- one ``{"wav": stem,
"utmos": score}`` line per file, a blank line, ``UTMOS: <mean, 4 decimals>``; an empty directory gives a mean of 0.

The checkpoint is a LOCAL file (``--utmos_ckpt``, a state dict of ``UTMOS22Strong`` / the published predictor); nothing is ever
fetched.

    python -m f5e_tts_amd.eval.eval_utmos --audio_dir gen/ --ext wav --utmos_ckpt utmos22_strong.pth
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path
from typing import List, Optional

import torch


def load_predictor(ckpt: Optional[str], device):
    if not ckpt:
        raise SystemExit("eval_utmos: --utmos_ckpt is required: a local state dict of the utmos22_strong predictor (nothing is "
                         "fetched)")
    from .utmos import UTMOS22Strong
    state = torch.load(ckpt, weights_only=True, map_location="cpu")
    state = state.get("state_dict", state) if isinstance(state, dict) else state
    return UTMOS22Strong.from_checkpoint(state).to(device)


def audio_files(audio_dir: str, ext: str) -> List[Path]:
    return sorted(Path(audio_dir).rglob(f"*.{ext}"))


def run_utmos(audio_dir: str, ext: str, predictor, device="cuda", batch: int = 1) -> float:
    """Scores every ``*.ext`` file under ``audio_dir`` with ``predictor`` (anything callable as ``predictor(wave [B, S] on
    ``device``, sr) -> scores [B]``), writes ``_utmos_results.jsonl`` there and returns the mean (0 without files).  ``batch`` > 1
    scores that many files of one sample rate per call when the predictor offers ``predict`` (ragged rows equal their own
    B = 1 run); the reference's one file per call is the default."""
    from ..infer.utils_infer import load_wav
    paths = audio_files(audio_dir, ext)
    result_path = Path(audio_dir) / "_utmos_results.jsonl"
    scores, pending = [], []                                  # pending: 16 kHz waves waiting for a full batch

    def flush():
        if pending:
            n = [int(w.numel()) for w in pending]
            rows = torch.zeros(len(pending), max(n))
            for b, w in enumerate(pending):
                rows[b, :n[b]] = w
            scores.extend(float(v) for v in predictor.predict(rows.to(device), n))
            pending.clear()

    for path in paths:
        wav, sr = load_wav(str(path))
        wav = wav.mean(0)                                     # mono: the mean of the channels
        if batch > 1 and sr == 16000 and hasattr(predictor, "predict"):
            pending.append(wav)
            if len(pending) == batch:
                flush()
        else:
            flush()                                           # keeps the scores in the order of the files
            scores.append(float(predictor(wav.to(device)[None], sr)[0]))
    flush()
    with open(result_path, "w", encoding="utf-8") as f:
        for path, score in zip(paths, scores):
            f.write(json.dumps({"wav": str(path.stem), "utmos": score}, ensure_ascii=False) + "\n")
        avg = sum(scores) / len(paths) if paths else 0
        f.write(f"\nUTMOS: {avg:.4f}\n")
    print(f"UTMOS: {avg:.4f}")
    print(f"UTMOS results saved to {result_path}")
    return float(avg)


def main(argv=None, predictor=None) -> float:
    ap = argparse.ArgumentParser(description="UTMOS of every audio file under a directory (utmos22_strong on the device)")
    ap.add_argument("--audio_dir", required=True, help="searched recursively")
    ap.add_argument("--ext", default="wav", help="audio extension (RIFF wav files)")
    ap.add_argument("--utmos_ckpt", default=None, help="local state dict of the utmos22_strong predictor (required; nothing is "
                                                       "fetched)")
    ap.add_argument("--batch", type=int, default=1, help="files per call (16 kHz files only; 1 = the reference's loop)")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if predictor is None:
        predictor = load_predictor(args.utmos_ckpt, args.device)
    return run_utmos(args.audio_dir, args.ext, predictor, args.device, args.batch)


if __name__ == "__main__":
    main()
