"""Generates tests/golden/mmdit_*.npz: the reference's ``MMDiT.forward`` (model/backbones/mmdit.py:147-188, built from
MMDiTBlock and JointAttnProcessor, model/modules.py:510-604, 647-718) on two small seeded configurations, for every
(drop_audio_cond, drop_text) pair.  They pin tests/mmdit_ref.py and the MMDiT mirror's state_dict layout.

Usage (build container only; the reference never travels to the GPU box):
    python tests/golden/make_mmdit_golden.py /root/reference

The parameters are rounded to fp16-representable values BEFORE the reference runs and stored as float16 (exact), which
keeps each file under the repository's size limit; tests widen them to fp32.  Buffers (rotary inv_freq) stay fp32."""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

# tag -> (constructor arguments, batch, audio frames, text tokens, seed)
CASES = {
    "b1": (dict(dim=64, depth=3, heads=2, dim_head=64, ff_mult=1, mel_dim=20, text_num_embeds=30,
                text_mask_padding=True, qk_norm=None), 1, 40, 9, 1100),
    "b2_rms": (dict(dim=64, depth=3, heads=2, dim_head=64, ff_mult=1, mel_dim=20, text_num_embeds=30,
                    text_mask_padding=False, qk_norm="rms_norm"), 2, 48, 13, 1200),
}


def main(ref_root: str):
    import make_golden as MG

    MG.load_reference(ref_root)
    mmdit_mod = importlib.import_module("f5_tts.model.backbones.mmdit")
    for tag, (arch, b, n, nt, seed) in CASES.items():
        torch.manual_seed(seed)
        m = mmdit_mod.MMDiT(**arch).eval()
        MG._unzero(m, seed + 1)
        g = torch.Generator().manual_seed(seed + 2)
        for p in m.parameters():
            p.data.copy_(p.data.half().float())
        x, cond = torch.randn(b, n, arch["mel_dim"], generator=g), torch.randn(b, n, arch["mel_dim"], generator=g)
        text = torch.randint(0, arch["text_num_embeds"], (b, nt), generator=g)
        mask = None
        if b > 1:
            text[1, nt - 4:] = -1
            mask = torch.arange(n)[None] < torch.tensor([n, n - 11])[:, None]
        time = torch.tensor(0.37)
        out = {"x": x, "cond": cond, "text": text, "mask": mask, "time": time}
        with torch.no_grad():
            for da in (False, True):
                for dt in (False, True):
                    out[f"pred_a{int(da)}_t{int(dt)}"] = m(x, cond, text, time, drop_audio_cond=da, drop_text=dt,
                                                           mask=mask)
        params = dict(m.named_parameters())
        out.update({"w/" + k: v.half() if k in params else v for k, v in m.state_dict().items()})
        path = os.path.join(HERE, f"mmdit_{tag}.npz")
        np.savez_compressed(path, **MG._np(out))
        print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
