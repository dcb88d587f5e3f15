"""Makes tests/golden/wavlm.npz from ``transformers.WavLMModel`` (5.15.0 when this was run), built from a config with seeded
random weights -- nothing is downloaded.  A tiny model of the WavLM-large STRUCTURE: layer-norm extractor with the real kernels and
strides, stable (pre-) layer norm, 128-tap / 16-group positional conv, gated relative-position bias with 320 buckets.

Stored: the HF-named weights (``w/<name>``), the input waves (raw; they are normalised here as s3prl does before the call:
``F.layer_norm`` over each row's valid samples, zeros beyond) and all 4 hidden states of every case:
  S = 400 (one frame), 23457 (73 frames, exact buckets only), 40000 (124 frames: |rel| >= 80 reaches the log buckets) and the
  padded pair (40000, 23457) with its attention mask (row 1 is stored up to its 73 valid frames).
To keep the file under the 1 MiB limit of a committed file the weights are rounded to bf16-representable values and the waves to
multiples of 2^-15 (16-bit PCM) BEFORE the model runs: both are still exact float32 inputs, they only compress better.

    python tests/golden/make_wavlm_golden.py
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

SEED = 20260
CASES = (400, 23457, 40000)


def hf_config():
    from transformers import WavLMConfig
    return WavLMConfig(
        hidden_size=64, num_hidden_layers=3, num_attention_heads=4, intermediate_size=128, conv_dim=(32,) * 7,
        conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), feat_extract_norm="layer", do_stable_layer_norm=True,
        num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, num_buckets=320, max_bucket_distance=800,
        hidden_dropout=0.0, activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0,
        layerdrop=0.0, mask_time_prob=0.0, mask_feature_prob=0.0, vocab_size=32)


def build_model():
    from transformers import WavLMModel
    torch.manual_seed(SEED)
    model = WavLMModel(hf_config()).eval()
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        for name, p in model.named_parameters():          # no gate, bias or norm may be trivial
            if "gru_rel_pos" in name:
                p.add_(0.3 * torch.randn(p.shape, generator=g))
            elif "rel_attn_embed" in name:
                p.add_(torch.randn(p.shape, generator=g))
            elif "layer_norm" in name:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        for p in model.parameters():
            p.copy_(p.bfloat16().float())
    return model


def normalise(wav, n):
    out = torch.zeros_like(wav)
    out[:n] = F.layer_norm(wav[:n], (n,), eps=1e-5)
    return out


def main():
    model = build_model()
    g = torch.Generator().manual_seed(SEED + 2)
    out = {"w/" + k: v.detach().numpy() for k, v in model.state_dict().items()}
    waves = {}
    with torch.no_grad():
        for S in CASES:
            t = torch.arange(S) / 16000.0
            w = 0.2 * torch.randn(S, generator=g) + 0.3 * torch.sin(2 * np.pi * (110.0 + S % 97) * t) * (1 + 0.5 * torch.sin(2 * np.pi * 3 * t))
            waves[S] = w = torch.round(w.clamp(-0.999, 0.999) * 32768) / 32768
            out[f"wav_{S}"] = w.numpy()
            hs = model(normalise(w, S)[None], output_hidden_states=True).hidden_states
            out[f"hs_{S}"] = torch.stack(hs)[:, 0].numpy()
        a, b = waves[40000], waves[23457]
        pair = torch.stack([normalise(a, 40000), normalise(F.pad(b, (0, 40000 - 23457)), 23457)])
        mask = torch.zeros(2, 40000, dtype=torch.long)
        mask[0], mask[1, :23457] = 1, 1
        hs = torch.stack(model(pair, attention_mask=mask, output_hidden_states=True).hidden_states)
        frames = model._get_feat_extract_output_lengths(torch.tensor([40000, 23457])).tolist()
        out["pair_frames"] = np.array(frames, np.int32)
        out["hs_pair_0"], out["hs_pair_1"] = hs[:, 0, :frames[0]].numpy(), hs[:, 1, :frames[1]].numpy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wavlm.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items() if not k.startswith("w/")})


if __name__ == "__main__":
    main()
