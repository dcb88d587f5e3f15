"""Makes tests/golden/utmos.npz from ``transformers.Wav2Vec2Model`` (5.15.0 when this was run) and ``torch.nn.LSTM``, built from a
config with seeded random weights -- nothing is downloaded.  A tiny model of the utmos22_strong STRUCTURE: group-norm feature
extractor with the real kernels and strides, post-LayerNorm encoder, 128-tap / 16-group positional conv; every frame joined with a
domain and a judge embedding; one bidirectional LSTM layer; Linear - ReLU - Linear; score = 2 * mean over frames + 3.

Stored: the weights (``w/wav2vec2.<HF name>``, ``w/domain_emb``, ``w/judge_emb``, ``w/blstm.*``, ``w/projection.{0,2}.*``), the
raw input waves (no waveform normalisation in this family) and per case the last hidden state, the BiLSTM output, the per-frame
scores and the utterance score:  S = 400 (one frame), 23457 (73 frames), 40000 (124 frames).
To keep the file under the 1 MiB limit of a committed file the weights are rounded to bf16-representable values and the waves to
multiples of 2^-15 (16-bit PCM) BEFORE the model runs: both are still exact float32 inputs, they only compress better.

A dead head would pass anything, so the script asserts that the per-frame scores of the two long cases have a standard deviation of
at least 0.05 and that no BiLSTM output is saturated (|h| < 0.99); HEAD_GAIN scales the projection's initialisation to get there.

    python tests/golden/make_utmos_golden.py
"""
import os

import numpy as np
import torch

SEED = 20261
CASES = (400, 23457, 40000)
D, EMB, H, P = 64, 16, 32, 128
HEAD_GAIN = 3.0


def hf_config():
    from transformers import Wav2Vec2Config
    return Wav2Vec2Config(
        hidden_size=D, num_hidden_layers=3, num_attention_heads=4, intermediate_size=128, conv_dim=(32,) * 7,
        conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), conv_bias=False, feat_extract_norm="group",
        do_stable_layer_norm=False, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16,
        hidden_dropout=0.0, activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0,
        layerdrop=0.0, mask_time_prob=0.0, mask_feature_prob=0.0, vocab_size=32)


def build_model():
    from transformers import Wav2Vec2Model
    torch.manual_seed(SEED)
    up = Wav2Vec2Model(hf_config()).eval()
    blstm = torch.nn.LSTM(D + 2 * EMB, H, batch_first=True, bidirectional=True)
    proj = torch.nn.Sequential(torch.nn.Linear(2 * H, P), torch.nn.ReLU(), torch.nn.Linear(P, 1))
    domain, judge = torch.randn(1, EMB), torch.randn(1, EMB)
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        for name, p in up.named_parameters():             # no norm may be trivial (the group norm of layer 0 is a layer_norm there)
            if "layer_norm" in name:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        for p in proj.parameters():
            p.mul_(HEAD_GAIN)
        for p in list(up.parameters()) + list(blstm.parameters()) + list(proj.parameters()) + [domain, judge]:
            p.copy_(p.bfloat16().float())
    return up, blstm.eval(), proj.eval(), domain, judge


def main():
    up, blstm, proj, domain, judge = build_model()
    g = torch.Generator().manual_seed(SEED + 2)
    out = {"w/wav2vec2." + k: v.detach().numpy() for k, v in up.state_dict().items()}
    out.update({"w/blstm." + k: v.detach().numpy() for k, v in blstm.state_dict().items()})
    out.update({"w/projection." + k: v.detach().numpy() for k, v in proj.state_dict().items()})
    out["w/domain_emb"], out["w/judge_emb"] = domain.numpy(), judge.numpy()
    with torch.no_grad():
        for S in CASES:
            t = torch.arange(S) / 16000.0
            w = 0.2 * torch.randn(S, generator=g) + 0.3 * torch.sin(2 * np.pi * (110.0 + S % 97) * t) * (1 + 0.5 * torch.sin(2 * np.pi * 3 * t))
            w = torch.round(w.clamp(-0.999, 0.999) * 32768) / 32768
            hidden = up(w[None]).last_hidden_state                                        # [1, T, D]
            T = hidden.shape[1]
            x = torch.cat([hidden, domain.expand(1, T, -1), judge.expand(1, T, -1)], -1)
            h, _ = blstm(x)
            frame = proj(h)[0, :, 0]
            out[f"wav_{S}"], out[f"hidden_{S}"], out[f"blstm_{S}"] = w.numpy(), hidden[0].numpy(), h[0].numpy()
            out[f"frame_{S}"], out[f"score_{S}"] = frame.numpy(), np.float32(frame.mean() * 2 + 3)
            print(f"S={S}: T={T} frame-score std {float(frame.std()) if T > 1 else 0:.3f} max |h| {float(h.abs().max()):.3f} "
                  f"score {float(out[f'score_{S}']):.4f}")
            assert float(h.abs().max()) < 0.99, "a saturated BiLSTM output"
            assert T == 1 or float(frame.std()) >= 0.05, "a dead head: scale HEAD_GAIN"
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "utmos.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items() if not k.startswith("w/")})
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
