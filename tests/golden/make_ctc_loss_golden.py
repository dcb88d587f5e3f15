"""Generates tests/golden/ctc_loss.npz from the reference's own ``CTC`` module (ppg/wenet/transformer/ctc.py), imported
where it lies: ``CTC.forward`` (ctc_lo, log_softmax, torch.nn.CTCLoss(reduction="sum"), batch-size average) on small random
inputs, and the per-utterance losses of the same module built with ``reduce=False``.  It pins tests/ctc_loss_ref.py,
f5e_ctc_loss and ``ConformerPPG.ctc_loss``.

Usage (where the reference checkout is; it never travels to the GPU machine):
    python tests/golden/make_ctc_loss_golden.py <reference root>

Cases: batch sizes 1 and 3, D = 16, V = 12, T <= 40; ``ys_pad`` is padded with -1 as the reference's collate does.  One
utterance carries an adjacent repeat.  Stored per case i: hs_pad_<i>, hlens_<i>, ys_pad_<i>, ys_lens_<i>, loss_<i> (the value of
``CTC.forward``), per_utt_<i>; shared: ctc_lo_weight, ctc_lo_bias."""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ctc_loss_ref as LR  # noqa: E402

D, V = 16, 12
CASES = [  # (frame lengths, label rows)
    ([33], [[3, 5, 5, 2, 9, 4]]),
    ([40, 27, 19], [[1, 7, 7, 7, 2, 11, 4, 6], [10, 3], [5, 8, 1, 1, 9]]),
]


def load_ctc(ref_root: str):
    path = os.path.join(ref_root, "src", "f5_tts", "ppg", "wenet", "transformer", "ctc.py")
    spec = importlib.util.spec_from_file_location("reference_ctc", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CTC


def main(ref_root: str):
    CTC = load_ctc(ref_root)
    torch.manual_seed(9101)
    summed, per = CTC(V, D).eval(), CTC(V, D, reduce=False).eval()
    with torch.no_grad():
        summed.ctc_lo.weight.mul_(4.0)           # logits of a few units: frames that prefer some classes
        per.load_state_dict(summed.state_dict())
    out = {"ctc_lo_weight": summed.ctc_lo.weight.detach().numpy(), "ctc_lo_bias": summed.ctc_lo.bias.detach().numpy(),
           "n_cases": np.asarray(len(CASES))}
    g = torch.Generator().manual_seed(9102)
    for i, (hl, rows) in enumerate(CASES):
        B, T, L = len(hl), max(hl), max(len(r) for r in rows)
        hs = torch.randn(B, T, D, generator=g)
        ys = torch.full((B, L), -1, dtype=torch.long)
        for b, r in enumerate(rows):
            ys[b, :len(r)] = torch.tensor(r)
        hlens, ylens = torch.tensor(hl), torch.tensor([len(r) for r in rows])
        with torch.no_grad():
            total = summed(hs, hlens, ys, ylens)
            each = per(hs, hlens, ys, ylens) * B          # forward divides by the batch size whatever the reduction
            logits = summed.ctc_lo(hs)
        assert torch.isfinite(each).all() and abs(float(each.sum() / B - total)) < 1e-4 * float(total)
        mine = -LR.loss(logits.numpy().astype(np.float64), ys.numpy(), hl, ylens.numpy(), dtype=np.float64)
        assert np.allclose(mine, each.numpy(), rtol=1e-5), (mine, each)
        out.update({f"hs_pad_{i}": hs.numpy(), f"hlens_{i}": np.asarray(hl, np.int32), f"ys_pad_{i}": ys.numpy().astype(np.int32),
                    f"ys_lens_{i}": ylens.numpy().astype(np.int32), f"loss_{i}": np.asarray(float(total), np.float32),
                    f"per_utt_{i}": each.numpy().astype(np.float32)})
        print(f"case {i}: B={B} T={T} L={L} CTC.forward {float(total):.5f} per utterance {each.numpy()}")
    path = os.path.join(HERE, "ctc_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main(sys.argv[1])
