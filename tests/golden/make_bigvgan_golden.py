"""Generates tests/golden/bigvgan_mel.npz: the reference's ``get_bigvgan_mel_spectrogram`` (model/modules.py:30-72) on
seeded waves, which pins the BigVGAN front-end's padding, framing, magnitude epsilon and log to the reference code.

Usage (build container only; the reference never travels to the GPU box):
    python tests/golden/make_bigvgan_golden.py /root/reference

librosa is not installed: ``librosa.filters.mel`` is shimmed with the in-tree slaney restatement
(``f5e_tts_amd.engine.slaney_mel_filterbank``), so the filter values themselves stay "parity unpinned"."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)


def main(ref_root: str):
    import make_golden as MG
    from f5e_tts_amd.engine import slaney_mel_filterbank
    from tools import synth as SY

    modules = MG.load_reference(ref_root)[0]

    def mel_shim(sr, n_fft, n_mels, fmin=0.0, fmax=None, **kw):
        return slaney_mel_filterbank(n_fft, n_mels, sr, fmin, fmax).t().numpy()

    modules.librosa_mel_fn = mel_shim
    out = {}
    for tag, frames, extra, batch, seed in (("a", 64, 0, 2, 2024), ("b", 37, 131, 1, 7)):
        wav = SY.synthetic_ref_wave(frames, seed=seed, batch=batch)
        if extra:
            wav = torch.cat([wav, wav[:, :extra].flip(1)], 1)
        mel = modules.get_bigvgan_mel_spectrogram(wav)
        out[f"{tag}_wav"] = wav.numpy().astype(np.float32)
        out[f"{tag}_mel"] = mel.numpy().astype(np.float32)
        print(tag, tuple(wav.shape), "->", tuple(mel.shape))
    np.savez_compressed(os.path.join(HERE, "bigvgan_mel.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
