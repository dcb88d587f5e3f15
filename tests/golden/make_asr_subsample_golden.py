"""Fixtures for the recogniser's 4x / 6x / 8x subsampling fronts and the layer-norm convolution module, from the reference's
own classes: ``init_asr_model`` (ppg/asr_model.py:814-859) with ``input_layer: conv2d4 / conv2d6 / conv2d8``
(``Conv2dSubsampling4 / 6 / 8``, ppg/wenet/transformer/subsampling.py:121-280) and ``cnn_module_norm: layer_norm``
(convolution.py:63-69, 122-128).

Usage (where the reference checkout is at hand; it is never needed to run the tests):
    python tests/golden/make_asr_subsample_golden.py <reference checkout>

One file per rate, ``asr_subsample_{4,6,8}.npz``.  A reduced conformer (``tests/asr_subsample_ref.fixture_config``: 64-d,
4 heads, 2 blocks, kernel 7, ``use_dynamic_chunk: true``, GlobalCMVN; 4x with ``cnn_module_norm: layer_norm``, 6x and 8x with
``batch_norm``, 8x ``causal``), seeded parameters rounded to fp16-representable values BEFORE the reference runs and stored
as float16 (exact); tests widen them to fp32.  Per file:

    w/<state_dict key>           encoder.*, ctc.* of the reference model
    feats_one [1, 101, 80]       one utterance (101 is no multiple of 4, 6 or 8)
    feats_pair [2, 77, 80], lens_pair = (77, context): a ragged batch whose second row has the MINIMUM length (7 / 11 / 15)
    embed_/enc_/logp_{one,pair}  ``encoder.embed`` output, encoder output (full context), ``ctc.log_softmax`` of it
    mask_pair [2, T']            the subsampled pad mask
    cbc                          ``forward_chunk_by_chunk(feats_one, 4, 2)``
    step{0,1}_{y,sub,att<i>,cnn<i>}   two consecutive ``forward_chunk`` calls on the loop's first two windows (offset 0 / 4,
                                 required_cache_size 4 * 2)"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]      # repository root, tests/, here

from asr_subsample_ref import RATES, RIGHT_CONTEXT, fixture_config     # noqa: E402
from make_ppg_stream_golden import load_reference_ppg                  # noqa: E402


def build_model(asr, cmvn_mod, rate):
    torch.manual_seed(6100 + rate)
    model = asr.init_asr_model(fixture_config(rate))
    g = torch.Generator().manual_seed(6200 + rate)
    mean, istd = torch.randn(80, generator=g), 0.5 + torch.rand(80, generator=g)
    model.encoder.global_cmvn = cmvn_mod.GlobalCMVN(mean.half().float(), istd.half().float())
    with torch.no_grad():
        for _, p in model.named_parameters():
            if p.ndim == 1:          # norm affines, biases: away from their 1 / 0 defaults
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        for name, b in model.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.1 * torch.randn(b.shape, generator=g))
            if name.endswith("running_var"):
                b.copy_(1.0 + 0.2 * torch.rand(b.shape, generator=g))
        for t in list(model.parameters()) + [b for n, b in model.named_buffers() if "running" in n]:
            t.copy_(t.half().float())
    return model.eval()


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    asr, cmvn_mod = load_reference_ppg(sys.argv[1])
    keep = ("encoder.embed.", "encoder.encoders.", "encoder.after_norm.", "encoder.global_cmvn.", "ctc.")
    for rate in RATES:
        model = build_model(asr, cmvn_mod, rate)
        context = RIGHT_CONTEXT[rate] + 1
        assert model.encoder.embed.subsampling_rate == rate and model.encoder.embed.right_context + 1 == context
        g = torch.Generator().manual_seed(6300 + rate)
        feats_one = (4.0 * torch.randn(1, 101, 80, generator=g) + 8.0).half().float()
        feats_pair = (4.0 * torch.randn(2, 77, 80, generator=g) + 8.0).half().float()
        feats_pair[1, context:] = 0.0
        lens_pair = torch.tensor([77, context])
        sd = {k: v for k, v in model.state_dict().items() if k.startswith(keep) and "concat_linear" not in k
              and "num_batches_tracked" not in k and "linear_xs_embs" not in k}
        out = {"w/" + k: v.half().numpy() for k, v in sd.items()}
        for k, v in sd.items():
            assert torch.equal(v.half().float(), v), k
        out.update(feats_one=feats_one.half().numpy(), feats_pair=feats_pair.half().numpy(), lens_pair=lens_pair.numpy())
        enc_ = model.encoder
        with torch.no_grad():
            for tag, feats, lens in (("one", feats_one, torch.tensor([101])), ("pair", feats_pair, lens_pair)):
                masks = (torch.arange(feats.shape[1])[None, :] < lens[:, None]).unsqueeze(1)
                emb, _, m2 = enc_.embed(enc_.global_cmvn(feats), masks)
                enc, m3 = enc_(feats, lens, None, decoding_chunk_size=-1)
                assert torch.equal(m2, m3)
                out["embed_" + tag], out["enc_" + tag] = emb.numpy(), enc.numpy()
                out["logp_" + tag] = model.ctc.log_softmax(enc).numpy()
            out["mask_pair"] = m3[:, 0].numpy()
            cbc, _ = enc_.forward_chunk_by_chunk(feats_one, 4, 2)
            out["cbc"] = cbc.numpy()
            window, stride = 3 * rate + context, 4 * rate
            cache = (None, None, None)
            for step, (cur, offset) in enumerate(((0, 0), (stride, 4))):
                y, sub, att, cnn = enc_.forward_chunk(feats_one[:, cur:cur + window], offset, 4 * 2, *cache)
                cache = (sub, att, cnn)
                out[f"step{step}_y"], out[f"step{step}_sub"] = y.numpy(), sub.numpy()
                for i, (a_, c_) in enumerate(zip(att, cnn)):
                    out[f"step{step}_att{i}"], out[f"step{step}_cnn{i}"] = a_.numpy(), c_.numpy()
        path = os.path.join(HERE, f"asr_subsample_{rate}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path) // 1024, "KiB",
              {k: v.shape for k, v in out.items() if not k.startswith("w/") and "step" not in k})


if __name__ == "__main__":
    main()
