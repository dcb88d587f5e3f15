"""Speaker-similarity (SIM) driver: mirror of reference eval/utils_eval.py::run_sim (714-753) on the ECAPA-TDNN head of
``eval/ecapa_tdnn.py``.  The WavLM-large upstream is not built here, so the hidden states of every recording are read from
``feat_dir/<stem>.npy`` (f32 [L, T, feat_dim], extracted from 16 kHz audio: resampling belongs to the extraction) -- as
``eval_infer_batch --ppg_dir`` took precomputed PPGs before the extractor existed.  The generated / prompt pair of an
utterance goes through ONE ragged batch of two rows; SIM is the cosine of the two embeddings.

    python -m f5e_tts_amd.eval.eval_sim --metalst meta.lst --gen_wav_dir gen/ --feat_dir feats/ --ckpt wavlm_large_finetune.pth
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


def _features(feat_dir: str, wav: str) -> np.ndarray:
    path = os.path.join(feat_dir, Path(wav).stem + ".npy")
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path}: no precomputed WavLM hidden states for {wav} (the upstream is not built here)")
    hs = np.load(path)
    if hs.ndim != 3:
        raise ValueError(f"{path}: expected [L, T, feat_dim], got {hs.shape}")
    return hs.astype(np.float32, copy=False)


def run_sim(test_set: Sequence[Tuple[str, str, str]], ckpt: Optional[str], feat_dir: str, device="cuda", model=None) -> List[dict]:
    """-> [{"wav": stem of the generated wav, "sim": cosine}] in the order of ``test_set``.  ``model``: an encoder already
    built (anything callable as ``model(hidden_states [L, 2, T, F], lengths) -> [2, emb]``); otherwise ``ckpt`` is loaded."""
    if model is None:
        model = load_model(ckpt, device)
    results = []
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


def main(argv=None, model=None) -> float:
    ap = argparse.ArgumentParser(description="speaker similarity of generated wavs against their prompts (ECAPA-TDNN head "
                                             "on precomputed WavLM hidden states)")
    ap.add_argument("--metalst", required=True, help="utt|prompt_text|prompt_wav|gt_text per line")
    ap.add_argument("--gen_wav_dir", required=True)
    ap.add_argument("--feat_dir", required=True, help="<stem>.npy per wav: f32 [L, T, feat_dim] hidden states (16 kHz audio)")
    ap.add_argument("--ckpt", required=model is None, help="wavlm_large_finetune.pth (its 'model' entry is loaded)")
    ap.add_argument("--out", default=None, help="per-utterance JSON (default: <gen_wav_dir>/_sim_results.json)")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    test_set = get_test_set(args.metalst, args.gen_wav_dir)
    if not test_set:
        raise SystemExit(f"{args.metalst}: no utterance has a generated wav under {args.gen_wav_dir}")
    results = run_sim(test_set, args.ckpt, args.feat_dir, args.device, model=model)
    sim = float(np.mean([r["sim"] for r in results]))
    out = args.out or os.path.join(args.gen_wav_dir, "_sim_results.json")
    with open(out, "w") as f:
        json.dump(results, f, indent=1)
    print(f"SIM: {sim:.5f} over {len(results)} utterances -> {out}")
    return sim


if __name__ == "__main__":
    main()
