"""Plain-torch restatement of the WavLM upstream (f5e_tts_amd/eval/wavlm.py, csrc/wavlm.hip, f5e_relbias_attn_f32): dtype-generic
(the dtype of the weights decides), fairseq / s3prl parameter names, channels-last.  Pinned by tests/golden/wavlm.npz, which
comes from ``transformers.WavLMModel`` (tests/test_wavlm_cpu.py); the GPU tests compare kernels against it in float64.

A ragged batch is DEFINED row by row: row b is the B = 1 run on its first ``lengths[b]`` samples, zero beyond its frames."""
import torch
import torch.nn.functional as F

from f5e_tts_amd.eval.wavlm import frame_counts, relative_bucket


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def wav_norm(wav, lengths=None):
    """[B, S] -> normalised over each row's valid samples (biased variance, eps 1e-5), zero beyond."""
    out = torch.zeros_like(wav)
    for b in range(wav.shape[0]):
        n = wav.shape[1] if lengths is None else int(lengths[b])
        if n > 0:
            out[b, :n] = F.layer_norm(wav[b, :n], (n,), eps=1e-5)
    return out


def gelu(x):
    return F.gelu(x)


def conv_ln_gelu(x, w, bias, g, beta, stride, eps=1e-5):
    """x [B, T, Cin] channels-last, w [C, Cin, k] -> [B, T', C]."""
    y = F.conv1d(x.transpose(1, 2), w, bias, stride=stride).transpose(1, 2)
    return gelu(F.layer_norm(y, (y.shape[-1],), g, beta, eps))


def extractor(sd, cfg, wn):
    x = wn[:, :, None]
    for i, s in enumerate(cfg.conv_stride):
        p = f"feature_extractor.conv_layers.{i}."
        x = conv_ln_gelu(x, sd[p + "0.weight"], sd.get(p + "0.bias"), sd[p + "2.1.weight"], sd[p + "2.1.bias"], s, cfg.layer_norm_eps)
    return x


def fold_wn(g, v):
    return v * (g / v.norm(dim=(0, 1), keepdim=True))


def posconv(x, w, bias, groups, frames=None):
    """x [B, T, D] -> x + GELU(conv(x) + bias) with frames outside [0, frames[b]) read as zero, zero beyond frames[b]."""
    B, T, D = x.shape
    out = torch.zeros_like(x)
    for b in range(B):
        n = T if frames is None else int(frames[b])
        if n > 0:
            xb = x[b:b + 1, :n]
            y = F.conv1d(xb.transpose(1, 2), w, bias, padding=w.shape[2] // 2, groups=groups)
            y = y[:, :, :n] if w.shape[2] % 2 == 0 else y
            out[b, :n] = (xb + gelu(y.transpose(1, 2)))[0]
    return out


def gate(xn, w_gate, b_gate, const, H):
    """xn [B, T, D] (normed layer input) -> [B, H, T]."""
    B, T, D = xn.shape
    p = F.linear(xn.view(B, T, H, D // H).permute(0, 2, 1, 3), w_gate, b_gate)       # [B, H, T, 8]
    p = p.view(B, H, T, 2, 4).sum(-1)
    a, b = torch.sigmoid(p).unbind(-1)
    return a * (b * const.view(1, H, 1) - 1.0) + 2.0


def compute_bias(rel_embed, T, num_buckets=320, max_distance=800):
    """rel_embed [num_buckets, H] -> [H, T, T] exactly as the published module builds it (the [T, T] grid of j - i)."""
    rel = torch.arange(T, dtype=torch.long)[None, :] - torch.arange(T, dtype=torch.long)[:, None]
    return rel_embed[relative_bucket(rel, num_buckets, max_distance)].permute(2, 0, 1)


def relbias_attention(q, k, v, g, bias, H, scale, kv_len=None):
    """q, k, v [B, T, D]; g [B, H, T]; bias [H, T, T] -> [B, T, D]; keys j < kv_len[b]; queries at or beyond it give zeros."""
    B, T, D = q.shape
    dk = D // H
    out = torch.zeros_like(q)
    for b in range(B):
        n = T if kv_len is None else int(kv_len[b])
        if n < 1:
            continue
        qb, kb, vb = (t[b, :n].view(n, H, dk).transpose(0, 1) for t in (q, k, v))
        s = qb @ kb.transpose(1, 2) * scale + g[b, :, :n, None] * bias[:, :n, :n].to(q.dtype)
        out[b, :n] = (torch.softmax(s, -1) @ vb).transpose(0, 1).reshape(n, D)
    return out


def encoder_layer(sd, cfg, i, x, bias, frames=None):
    p = f"encoder.layers.{i}."
    D, H, eps = cfg.encoder_embed_dim, cfg.encoder_attention_heads, cfg.layer_norm_eps
    xn = F.layer_norm(x, (D,), sd[p + "self_attn_layer_norm.weight"], sd[p + "self_attn_layer_norm.bias"], eps)
    q, k, v = (F.linear(xn, sd[p + f"self_attn.{n}_proj.weight"], sd[p + f"self_attn.{n}_proj.bias"]) for n in "qkv")
    g = gate(xn, sd[p + "self_attn.grep_linear.weight"], sd[p + "self_attn.grep_linear.bias"], sd[p + "self_attn.grep_a"].reshape(-1), H)
    a = relbias_attention(q, k, v, g, bias, H, (D // H) ** -0.5, frames)
    x = x + F.linear(a, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"])
    xn = F.layer_norm(x, (D,), sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"], eps)
    return x + F.linear(gelu(F.linear(xn, sd[p + "fc1.weight"], sd[p + "fc1.bias"])), sd[p + "fc2.weight"], sd[p + "fc2.bias"])


def forward_one(sd, cfg, wav):
    """wav [1, S] -> list of L + 1 hidden states [1, T, D]."""
    C, D = cfg.conv_dim[-1], cfg.encoder_embed_dim
    x = extractor(sd, cfg, wav_norm(wav))
    x = F.layer_norm(x, (C,), sd["layer_norm.weight"], sd["layer_norm.bias"], cfg.layer_norm_eps)
    x = F.linear(x, sd["post_extract_proj.weight"], sd["post_extract_proj.bias"])
    w = fold_wn(sd["encoder.pos_conv.0.weight_g"], sd["encoder.pos_conv.0.weight_v"])
    x = posconv(x, w, sd["encoder.pos_conv.0.bias"], cfg.conv_pos_groups)
    bias = compute_bias(sd["encoder.layers.0.self_attn.relative_attention_bias.weight"], x.shape[1], cfg.num_buckets,
                        cfg.max_distance)
    hs = []
    for i in range(cfg.encoder_layers):
        hs.append(x)
        x = encoder_layer(sd, cfg, i, x, bias)
    hs.append(F.layer_norm(x, (D,), sd["encoder.layer_norm.weight"], sd["encoder.layer_norm.bias"], cfg.layer_norm_eps))
    return hs


def forward(sd, cfg, wav, lengths=None):
    """wav [B, S] -> (hs [L + 1, B, T, D] zero beyond each row's frames, frames list)."""
    B, S = wav.shape
    lengths = [S] * B if lengths is None else [int(v) for v in lengths]
    frames = [frame_counts(n, cfg)[-1] for n in lengths]
    T = frame_counts(S, cfg)[-1]
    out = torch.zeros(cfg.encoder_layers + 1, B, T, cfg.encoder_embed_dim, dtype=wav.dtype, device=wav.device)
    for b in range(B):
        hs = forward_one(sd, cfg, wav[b:b + 1, :lengths[b]])
        out[:, b, :frames[b]] = torch.stack(hs)[:, 0]
    return out, frames


def rel_l2(a, b):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
