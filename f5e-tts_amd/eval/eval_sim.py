"""Speaker-similarity (SIM) driver: mirror of reference eval/utils_eval.py::run_sim (714-753), from two wav files to a cosine:
the WavLM-large upstream of ``eval/wavlm.py`` and the ECAPA-TDNN head of ``eval/ecapa_tdnn.py``, both loaded from the one
checkpoint.  Every wav is read, moved to the device and resampled to 16 kHz there; the generated / prompt pair of an utterance
goes through ONE ragged batch of two rows; SIM is the cosine of the two embeddings.  ``--dump_feats DIR`` keeps the hidden
states of every recording as ``DIR/<stem>.npy`` (f32 [L, T, feat_dim]); ``--feat_dir DIR`` reads such files instead of running
the upstream (the route from before the upstream existed, unchanged).

    python -m f5e_tts_amd.eval.eval_sim --metalst meta.lst --gen_wav_dir gen/ --ckpt wavlm_large_finetune.pth
"""
from __future__ import annotations

import argparse
import json
import os
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch


def get_test_set(metalst: str, gen_wav_dir: str) -> List[Tuple[str, str, str]]:
    """``get_seed_tts_test`` (utils_eval.py:400-418) without the split over GPUs: lines ``utt|prompt_text|prompt_wav|gt_text``
    (a fifth field is ignored); utterances without a generated wav are skipped; a relative prompt path is relative to the
    list.  -> [(gen_wav, prompt_wav, truth)]."""
    rows = []
    with open(metalst) as f:
        for line in f:
            parts = line.strip().split("|")
            if len(parts) not in (4, 5):
                continue
            utt, _, prompt_wav, gt_text = parts[:4]
            gen_wav = os.path.join(gen_wav_dir, utt + ".wav")
            if not os.path.exists(gen_wav):
                continue
            if not os.path.isabs(prompt_wav):
                prompt_wav = os.path.join(os.path.dirname(metalst), prompt_wav)
            rows.append((gen_wav, prompt_wav, gt_text))
    return rows


def load_model(ckpt: str, device):
    """``ECAPA_TDNN_SMALL(feat_dim=1024)`` with ``state_dict["model"]`` loaded ``strict=False`` (utils_eval.py:718-720)."""
    from .ecapa_tdnn import ECAPA_TDNN_SMALL
    model = ECAPA_TDNN_SMALL(feat_dim=1024)
    state = torch.load(ckpt, weights_only=True, map_location="cpu")
    missing, _ = model.load_state_dict(state["model"], strict=False)
    if missing:
        raise RuntimeError(f"{ckpt}: the checkpoint lacks {len(missing)} keys of the ECAPA-TDNN head, e.g. {missing[:3]}")
    return model.to(device).eval()


def load_upstream(ckpt: str, device):
    """The WavLM-large upstream from the ``feature_extract.model.*`` keys of the same checkpoint."""
    from .wavlm import WavLM
    state = torch.load(ckpt, weights_only=True, map_location="cpu")
    return WavLM.from_sim_checkpoint(state["model"]).to(device).eval()


def _wav16k(path: str, device) -> torch.Tensor:
    """The first channel of a wav file at 16 kHz, on ``device`` (resampled there when it is a GPU)."""
    from ..infer import audio
    from ..infer.utils_infer import load_wav
    wav, sr = load_wav(path)
    wav = wav[0].to(device)
    return (audio.resample_device if wav.is_cuda else audio.resample)(wav, sr, 16000)


def _features(feat_dir: str, wav: str) -> np.ndarray:
    path = os.path.join(feat_dir, Path(wav).stem + ".npy")
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path}: no precomputed WavLM hidden states for {wav} (drop --feat_dir to run the upstream on the audio)")
    hs = np.load(path)
    if hs.ndim != 3:
        raise ValueError(f"{path}: expected [L, T, feat_dim], got {hs.shape}")
    return hs.astype(np.float32, copy=False)


def run_sim(test_set: Sequence[Tuple[str, str, str]], ckpt: Optional[str], feat_dir: Optional[str] = None, device="cuda",
            model=None, upstream=None, dump_feats: Optional[str] = None) -> List[dict]:
    """-> [{"wav": stem of the generated wav, "sim": cosine}] in the order of ``test_set``.  ``model``: an encoder already
    built (anything callable as ``model(hidden_states [L, 2, T, F], lengths) -> [2, emb]``); otherwise ``ckpt`` is loaded.
    ``feat_dir``: read precomputed hidden states.  Without it the audio goes through ``upstream`` (anything callable as
    ``upstream([wav_a, wav_b]) -> {"hidden_states": [L tensors [2, T, F]], "lengths": frames [2]}``; by default the WavLM of
    ``ckpt``), and ``dump_feats`` names a directory that receives ``<stem>.npy`` per recording."""
    if model is None:
        model = load_model(ckpt, device)
    results = []
    if feat_dir is None:
        if upstream is None:
            if not ckpt:
                raise ValueError("run_sim: the audio route needs an upstream or the checkpoint to load it from (or a feat_dir)")
            upstream = load_upstream(ckpt, device)
        if dump_feats:
            os.makedirs(dump_feats, exist_ok=True)
        for gen_wav, prompt_wav, _truth in test_set:
            feats = upstream([_wav16k(gen_wav, device), _wav16k(prompt_wav, device)])
            hs, frames = torch.stack(list(feats["hidden_states"])), feats["lengths"]
            emb = model(hs, frames)
            sim = torch.nn.functional.cosine_similarity(emb[0:1], emb[1:2])[0].item()
            results.append({"wav": Path(gen_wav).stem, "sim": sim})
            if dump_feats:
                for row, wav in enumerate((gen_wav, prompt_wav)):
                    np.save(os.path.join(dump_feats, Path(wav).stem + ".npy"), hs[:, row, :int(frames[row])].cpu().numpy())
        return results
    for gen_wav, prompt_wav, _truth in test_set:
        a, b = _features(feat_dir, gen_wav), _features(feat_dir, prompt_wav)
        if a.shape[0] != b.shape[0] or a.shape[2] != b.shape[2]:
            raise ValueError(f"{gen_wav} / {prompt_wav}: hidden states disagree in layers or width: {a.shape} vs {b.shape}")
        T = max(a.shape[1], b.shape[1])
        pair = np.zeros((a.shape[0], 2, T, a.shape[2]), np.float32)
        pair[:, 0, :a.shape[1]], pair[:, 1, :b.shape[1]] = a, b
        emb = model(torch.from_numpy(pair).to(device), [a.shape[1], b.shape[1]])
        sim = torch.nn.functional.cosine_similarity(emb[0:1], emb[1:2])[0].item()
        results.append({"wav": Path(gen_wav).stem, "sim": sim})
    return results


def main(argv=None, model=None, upstream=None) -> float:
    ap = argparse.ArgumentParser(description="speaker similarity of generated wavs against their prompts (WavLM-large "
                                             "upstream + ECAPA-TDNN head)")
    ap.add_argument("--metalst", required=True, help="utt|prompt_text|prompt_wav|gt_text per line")
    ap.add_argument("--gen_wav_dir", required=True)
    ap.add_argument("--feat_dir", default=None, help="read <stem>.npy per wav (f32 [L, T, feat_dim] hidden states of 16 kHz "
                                                     "audio) instead of running the upstream on the audio")
    ap.add_argument("--dump_feats", default=None, help="audio route: write the hidden states of every wav here as <stem>.npy")
    ap.add_argument("--ckpt", required=model is None, help="wavlm_large_finetune.pth (its 'model' entry is loaded)")
    ap.add_argument("--out", default=None, help="per-utterance JSON (default: <gen_wav_dir>/_sim_results.json)")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    test_set = get_test_set(args.metalst, args.gen_wav_dir)
    if not test_set:
        raise SystemExit(f"{args.metalst}: no utterance has a generated wav under {args.gen_wav_dir}")
    if args.feat_dir and args.dump_feats:
        raise SystemExit("--dump_feats belongs to the audio route; it cannot be combined with --feat_dir")
    results = run_sim(test_set, args.ckpt, args.feat_dir, args.device, model=model, upstream=upstream,
                      dump_feats=args.dump_feats)
    sim = float(np.mean([r["sim"] for r in results]))
    out = args.out or os.path.join(args.gen_wav_dir, "_sim_results.json")
    with open(out, "w") as f:
        json.dump(results, f, indent=1)
    print(f"SIM: {sim:.5f} over {len(results)} utterances -> {out}")
    return sim


if __name__ == "__main__":
    main()
