"""Generates tests/golden/mas_paths.npz and tests/golden/mas_dit.npz from the reference's own monotonic alignment search
(durpred/monotonic_align: ``maximum_path`` over the numba loop ``maximum_path_jit``, which make_golden's pass-through
numba shim runs as plain Python on float32 arrays) and its ``DiT.align_text_ppg`` / ``DiT.calc_align_loss``
(model/backbones/dit.py:309-360).  They pin tests/mas_ref.py, csrc/mas.hip and the DiT / CFM alignment methods.

Usage (build container only; the reference never travels to the GPU box):
    python tests/golden/make_mas_golden.py /root/reference

mas_paths.npz: seeded matrices ``logp_<i>`` f32 [B, Ty, Tx], lengths ``ty_<i>`` / ``tx_<i>`` and the reference's dense paths
``path_<i>`` (uint8).  mas_dit.npz: a small codebook + PPG DiT (dimensions the HIP engine accepts; only the text_embed.*,
ppg_embed.* and quantizer.* tensors, which is all the alignment reads, rounded to fp16-representable values BEFORE the
reference runs and stored as float16), its inputs, the reference's two embeddings, ``attn`` and the loss value.

Before anything is written the script asserts that no stored discrete decision is fragile: every path survives uniform
noise of +-1e-3 on its matrix (5 draws), and every quantizer row of the DiT case has a top-1 / top-2 logit gap above 1e-3.
A tolerance in a test can then never hide a flipped decision.  If a seed fails, pick another; do not loosen the check."""
from __future__ import annotations

import importlib
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

NOISE, DRAWS, GAP = 1e-3, 5, 1e-3

# (B, Ty, Tx, t_y, t_x, seed): ragged batches, t_x = 1, t_x = t_y, t_y < Ty, Tx off the 32 / 64 grid
PATH_CASES = [
    (3, 160, 50, [160, 121, 77], [50, 33, 50], 4101),
    (2, 256, 96, [256, 200], [96, 1], 4200),
    (2, 70, 70, [70, 45], [70, 45], 4300),
    (1, 200, 67, [150], [67], 4400),
]

DIT_ARCH = dict(dim=256, depth=1, heads=4, dim_head=64, ff_mult=1, mel_dim=20, text_num_embeds=30, text_dim=256,
                conv_layers=1, text_mask_padding=False)
DIT_PPG = dict(use_ppg=True, ppg_dim=32, use_transformer=False, transformer_config=dict(), use_cross_mask=False,
               cross_mask_config=dict())
DIT_CB = dict(use_codebook=True, num_vars=20, temp_start=2, temp_stop=0.5, temp_decay=0.999995, groups=2,
              combine_groups=False, weight_proj_depth=1, weight_proj_factor=1, use_perplex_loss=False,
              perplex_loss_config=dict(), use_align_loss=True, align_loss_config=dict(align_loss_weight=0.5))
DIT_SEED, DIT_B, DIT_N, DIT_NT = 5110, 2, 48, 13
DIT_TEXT_LEN, DIT_PPG_LEN = [13, 9], [48, 37]
KEPT = ("text_embed.", "ppg_embed.", "quantizer.")


def ref_path(mono, logp: torch.Tensor, ty, tx) -> torch.Tensor:
    """The reference's maximum_path on [B, Ty, Tx] with the mask its callers build (outer product of the two length masks)."""
    B, Ty, Tx = logp.shape
    my = torch.arange(Ty)[None, :] < torch.as_tensor(ty)[:, None]
    mx = torch.arange(Tx)[None, :] < torch.as_tensor(tx)[:, None]
    mask = (my[:, :, None] & mx[:, None, :]).float()
    return mono.maximum_path(logp.clone(), mask)


def assert_stable(mono, logp, ty, tx, path, seed):
    g = torch.Generator().manual_seed(seed)
    for d in range(DRAWS):
        noisy = logp + (torch.rand(logp.shape, generator=g) * 2 - 1) * NOISE
        assert torch.equal(ref_path(mono, noisy, ty, tx), path), f"path flips under +-{NOISE} noise (draw {d}): new seed"


def make_paths(mono):
    out = {}
    for i, (B, Ty, Tx, ty, tx, seed) in enumerate(PATH_CASES):
        g = torch.Generator().manual_seed(seed)
        logp = torch.randn(B, Ty, Tx, generator=g) * 3.0 - 4.0
        keep = logp.clone()
        path = ref_path(mono, logp, ty, tx)
        assert torch.equal(logp, keep)
        for b in range(B):   # a monotonic path: one token per frame below t_y, every token used, nothing outside
            assert path[b, :ty[b]].sum(-1).eq(1).all() and path[b, ty[b]:].sum() == 0 and path[b, :, tx[b]:].sum() == 0
            assert path[b, :ty[b], :tx[b]].sum(0).ge(1).all()
        assert_stable(mono, logp, ty, tx, path, seed + 1)
        out[f"logp_{i}"], out[f"path_{i}"] = logp, path.to(torch.uint8)
        out[f"ty_{i}"], out[f"tx_{i}"] = np.asarray(ty, np.int32), np.asarray(tx, np.int32)
    out["n_cases"] = np.asarray(len(PATH_CASES))
    return out


def make_dit(MG, dit_mod, mono):
    torch.manual_seed(DIT_SEED)
    m = dit_mod.DiT(**DIT_ARCH, ppg_config=DIT_PPG, cb_config=DIT_CB)
    MG._unzero(m, DIT_SEED + 1)
    m.eval()
    for name, p in m.named_parameters():
        if name.startswith(KEPT):
            p.data.copy_(p.data.half().float())
    g = torch.Generator().manual_seed(DIT_SEED + 2)
    text = torch.randint(0, DIT_ARCH["text_num_embeds"], (DIT_B, DIT_NT), generator=g)
    for b, n in enumerate(DIT_TEXT_LEN):
        text[b, n:] = -1
    ppg = torch.randn(DIT_B, DIT_N, DIT_PPG["ppg_dim"], generator=g)
    text_len, ppg_len = torch.tensor(DIT_TEXT_LEN), torch.tensor(DIT_PPG_LEN)
    with torch.no_grad():
        text_embed = m.text_embed(text, DIT_B, DIT_N)
        ppg_embed = m.ppg_embed(ppg, DIT_N)
        attn = m.align_text_ppg(text_embed, text_len, ppg_embed, ppg_len)
        loss = m.calc_align_loss(attn, text_embed, text_len, ppg_embed)
        # fragility checks: the likelihood matrix restated (dit.py:320-325), searched under noise; the quantizer's logit gaps
        d = text_embed.shape[-1]
        neg_cent = (-0.5 * math.log(2 * math.pi) * d - 0.5 * (ppg_embed ** 2).sum(-1)[:, :, None]
                    + torch.einsum("btd,bsd->bts", ppg_embed, text_embed) - 0.5 * (text_embed ** 2).sum(-1)[:, None, :])
        path = attn.transpose(1, 2)
        assert torch.equal(ref_path(mono, neg_cent, DIT_PPG_LEN, DIT_TEXT_LEN), path)
        assert_stable(mono, neg_cent, DIT_PPG_LEN, DIT_TEXT_LEN, path, DIT_SEED + 3)
        for e in (text_embed, ppg_embed):
            logits = m.quantizer.weight_proj(e.reshape(-1, d)).view(-1, DIT_CB["groups"], DIT_CB["num_vars"])
            top = logits.topk(2, dim=-1).values
            assert float((top[..., 0] - top[..., 1]).min()) > GAP, "quantizer logit gap below the bound: new seed"
    assert float(loss) > 0
    out = {"text": text, "ppg": ppg, "text_len": text_len, "ppg_len": ppg_len, "text_embed": text_embed,
           "ppg_embed": ppg_embed, "attn": attn.to(torch.uint8), "loss": loss,
           "align_loss_weight": np.asarray(DIT_CB["align_loss_config"]["align_loss_weight"])}
    params = dict(m.named_parameters())
    out.update({"w/" + k: (v.half() if k in params else v) for k, v in m.state_dict().items() if k.startswith(KEPT)})
    return out


def main(ref_root: str):
    import make_golden as MG

    _, dit_mod, _, _ = MG.load_reference(ref_root)
    mono = importlib.import_module("f5_tts.durpred.monotonic_align")
    for name, arrays in (("mas_paths.npz", make_paths(mono)), ("mas_dit.npz", make_dit(MG, dit_mod, mono))):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **MG._np(arrays))
        print("wrote", path, os.path.getsize(path) // 1024, "KiB")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
