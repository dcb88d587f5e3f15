"""Fixtures for the chunk-by-chunk (streaming) mode of the PPG extractor, from the reference's own classes:
``ASRModel.extract(stream=True)`` (ppg/asr_model.py:222-244 -> ``BaseEncoder.forward_chunk_by_chunk(speech, 16, 17)``,
ppg/wenet/transformer/encoder.py:210-355) and two consecutive ``forward_chunk`` calls with their caches.

Usage (where the reference checkout is at hand; it is never needed to run the tests):
    python tests/golden/make_ppg_stream_golden.py <reference checkout>

A reduced encoder as in ``make_golden.py ppg`` (64-d, 4 heads, 2 blocks, kernel 15, seeded parameters and BatchNorm
buffers, GlobalCMVN), ``use_dynamic_chunk: true``, for ``causal`` false and true.  The SAME parameters serve both settings
(``causal`` only changes the padding of the depthwise convolution).  Parameters and features are rounded to
fp16-representable values BEFORE the reference runs and stored as float16 (exact), which keeps every file under the
repository's size limit; tests widen them to fp32.

    ppg_stream_common.npz     w/<state_dict key>, feats_long [1, 645, 80] (322 frames = 20 chunks + 2), feats_short [1, 75, 80]
    ppg_stream_causal{0,1}.npz  ppg_/logits_{long,short} of extract(stream=True); step{0,1}_{y,sub,att<i>,cnn<i>} of two
                              forward_chunk calls on feats_long (offset 0 / 16, required_cache_size 16 * 17);
                              causal1 also full_ppg_long / full_logits_long / full_ppg_pair / full_logits_pair of
                              extract(stream=False) (one utterance; a ragged batch of two, lens_pair)

The script also prints the check of the one-pass formulation the HIP path uses: the reference's
``encoder(feats, lens, None, decoding_chunk_size=16, num_decoding_left_chunks=17)`` against its chunk-by-chunk loop."""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference_ppg(ref_root):
    """The import recipe of ``make_golden.make_ppg_case``: the reference's ppg package without its heavy siblings."""
    src = os.path.join(ref_root, "src", "f5_tts")
    if "f5_tts" not in sys.modules or not hasattr(sys.modules["f5_tts"], "__path__"):
        pkg = types.ModuleType("f5_tts")
        pkg.__path__ = [src]
        sys.modules["f5_tts"] = pkg
    pk = types.ModuleType("f5_tts.ppg")
    pk.__path__ = [os.path.join(src, "ppg")]
    sys.modules["f5_tts.ppg"] = pk
    for name in ("torchaudio", "torchaudio.transforms", "torchaudio.compliance", "torchaudio.compliance.kaldi"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["torchaudio"].transforms = sys.modules["torchaudio.transforms"]
    sys.modules["torchaudio"].compliance = sys.modules["torchaudio.compliance"]
    sys.modules["torchaudio.compliance"].kaldi = sys.modules["torchaudio.compliance.kaldi"]
    asr = importlib.import_module("f5_tts.ppg.asr_model")
    cmvn_mod = importlib.import_module("f5_tts.ppg.wenet.transformer.cmvn")
    return asr, cmvn_mod


def build_model(asr, cmvn_mod, causal):
    cfg = dict(cmvn_file=None, is_json_cmvn=True, input_dim=80, output_dim=40, encoder="conformer", decoder="transformer",
               encoder_conf=dict(output_size=64, attention_heads=4, linear_units=128, num_blocks=2, cnn_module_kernel=15,
                                 use_dynamic_chunk=True, causal=causal),
               decoder_conf=dict(attention_heads=4, linear_units=64, num_blocks=1),
               model_conf=dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False, sv_conf=dict(use_sv=False)))
    torch.manual_seed(5151)
    model = asr.init_asr_model(cfg)
    g = torch.Generator().manual_seed(5152)
    mean, istd = torch.randn(80, generator=g), 0.5 + torch.rand(80, generator=g)
    model.encoder.global_cmvn = cmvn_mod.GlobalCMVN(mean.half().float(), istd.half().float())
    with torch.no_grad():
        for _, p in model.named_parameters():
            if p.ndim == 1:          # LayerNorm / BatchNorm affine, biases: away from their 1 / 0 defaults
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        for name, b in model.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.1 * torch.randn(b.shape, generator=g))
            if name.endswith("running_var"):
                b.copy_(1.0 + 0.2 * torch.rand(b.shape, generator=g))
        for t in list(model.parameters()) + [b for n, b in model.named_buffers() if "running" in n]:
            t.copy_(t.half().float())
    return model.eval()


def rel(a, b):
    return float((a - b).norm() / b.norm())


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    ref = sys.argv[1]
    asr, cmvn_mod = load_reference_ppg(ref)
    g = torch.Generator().manual_seed(5153)
    feats_long = (4.0 * torch.randn(1, 645, 80, generator=g) + 8.0).half().float()
    feats_short = (4.0 * torch.randn(1, 75, 80, generator=g) + 8.0).half().float()
    feats_pair = torch.cat([feats_long[:, :101], feats_short.new_zeros(1, 101, 80)], 0)
    feats_pair[1, :75] = feats_short[0]
    lens_pair = torch.tensor([101, 75])
    keep = ("encoder.embed.", "encoder.encoders.", "encoder.after_norm.", "encoder.global_cmvn.", "linear.", "ce.fc.")
    common = None
    for causal in (False, True):
        model = build_model(asr, cmvn_mod, causal)
        sd = {k: v for k, v in model.state_dict().items() if k.startswith(keep) and "concat_linear" not in k
              and "num_batches_tracked" not in k}
        if common is None:
            common = {"w/" + k: v.half().numpy() for k, v in sd.items()}
            for k, v in sd.items():
                assert torch.equal(v.half().float(), v), k
            common.update(feats_long=feats_long.half().numpy(), feats_short=feats_short.half().numpy())
            path = os.path.join(HERE, "ppg_stream_common.npz")
            np.savez_compressed(path, **common)
            print("wrote", path, os.path.getsize(path) // 1024, "KiB")
        else:
            for k, v in sd.items():
                assert np.array_equal(common["w/" + k], v.half().numpy()), k      # one weight set serves both settings
        out = {}
        with torch.no_grad():
            for tag, feats in (("long", feats_long), ("short", feats_short)):
                n = feats.shape[1]
                ppg, logits = model.extract(feats, torch.tensor([n]), stream=True)
                out["ppg_" + tag], out["logits_" + tag] = ppg.numpy(), logits.numpy()
                one, _ = model.encoder(feats, torch.tensor([n]), None, decoding_chunk_size=16, num_decoding_left_chunks=17)
                full, _ = model.encoder(feats, torch.tensor([n]), None, decoding_chunk_size=-1)
                print("causal=%d T=%d: stream frames %d (full-context %d); one-pass banded encoder vs loop rel L2 %.2e; "
                      "full context vs loop %.2e" % (causal, n, ppg.shape[1], full.shape[1],
                                                     rel(model.linear(one), ppg), rel(model.linear(full), ppg)))
            cache = (None, None, None)
            for step, (cur, offset) in enumerate(((0, 0), (32, 16))):
                y, sub, att, cnn = model.encoder.forward_chunk(feats_long[:, cur:cur + 33], offset, 16 * 17, *cache)
                cache = (sub, att, cnn)
                out[f"step{step}_y"], out[f"step{step}_sub"] = y.numpy(), sub.numpy()
                for i, (a_, c_) in enumerate(zip(att, cnn)):
                    out[f"step{step}_att{i}"], out[f"step{step}_cnn{i}"] = a_.numpy(), c_.numpy()
            if causal:
                p1, l1 = model.extract(feats_long, torch.tensor([645]), stream=False)
                p2, l2 = model.extract(feats_pair, lens_pair, stream=False)
                out.update(full_ppg_long=p1.numpy(), full_logits_long=l1.numpy(), full_ppg_pair=p2.numpy(),
                           full_logits_pair=l2.numpy(), feats_pair=feats_pair.half().numpy(), lens_pair=lens_pair.numpy())
        path = os.path.join(HERE, f"ppg_stream_causal{int(causal)}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path) // 1024, "KiB", {k: v.shape for k, v in out.items() if "step" not in k})


if __name__ == "__main__":
    main()
