"""Plain-torch restatement of the UTMOS predictor (f5e_tts_amd/eval/wav2vec2.py, eval/utmos.py, csrc/utmos.hip): dtype-generic
(the dtype of the weights decides), the module's own parameter names, channels-last.  Pinned by tests/golden/utmos.npz, which comes
from ``transformers.Wav2Vec2Model`` and ``torch.nn.LSTM`` (tests/test_utmos_cpu.py); the GPU tests compare kernels against it in
float64.

A ragged batch is DEFINED row by row: row b is the B = 1 run on its first ``lengths[b]`` samples (frames), zero beyond."""
import torch
import torch.nn.functional as F

from wavlm_ref import cast, fold_wn, gelu, posconv, rel_l2  # noqa: F401  (re-exported for the tests)

from f5e_tts_amd.eval.wavlm import frame_counts


def conv0_gn(wav, w, bias, g, beta, lengths=None, eps=1e-5):
    """wav [B, S], w [C, 1, 10] -> [B, T0, C]: conv (stride 5), every channel normalised over the row's own frames (biased
    variance), affine, GELU; zero beyond a row's frames."""
    B, S = wav.shape
    C = w.shape[0]
    out = wav.new_zeros(B, (S - 10) // 5 + 1, C)
    for b in range(B):
        n = S if lengths is None else int(lengths[b])
        if n >= 10:
            y = F.conv1d(wav[b:b + 1, None, :n], w, bias, stride=5)                    # [1, C, T0_b]
            # F.group_norm(y, C, g, beta, eps), written out: torch refuses it for a single frame
            yn = (y - y.mean(2, keepdim=True)) / torch.sqrt(y.var(2, unbiased=False, keepdim=True) + eps)
            out[b, :y.shape[2]] = gelu(yn * g[None, :, None] + beta[None, :, None])[0].t()
    return out


def extractor(sd, cfg, wav):
    """wav [1, S] -> [1, T, C]."""
    p = "feature_extractor.conv_layers."
    x = conv0_gn(wav, sd[p + "0.0.weight"], sd.get(p + "0.0.bias"), sd[p + "0.2.weight"], sd[p + "0.2.bias"], None, cfg.layer_norm_eps)
    for i in range(1, len(cfg.conv_stride)):
        y = F.conv1d(x.transpose(1, 2), sd[p + f"{i}.0.weight"], sd.get(p + f"{i}.0.bias"), stride=cfg.conv_stride[i])
        x = gelu(y).transpose(1, 2)
    return x


def attention(q, k, v, H, scale):
    """q, k, v [1, T, D] -> [1, T, D], plain softmax attention."""
    _, T, D = q.shape
    qh, kh, vh = (t[0].view(T, H, D // H).transpose(0, 1) for t in (q, k, v))
    return (torch.softmax(qh @ kh.transpose(1, 2) * scale, -1) @ vh).transpose(0, 1).reshape(1, T, D)


def encoder_layer(sd, cfg, i, x):
    p = f"encoder.layers.{i}."
    D, H, eps = cfg.encoder_embed_dim, cfg.encoder_attention_heads, cfg.layer_norm_eps
    q, k, v = (F.linear(x, sd[p + f"self_attn.{n}_proj.weight"], sd[p + f"self_attn.{n}_proj.bias"]) for n in "qkv")
    a = attention(q, k, v, H, (D // H) ** -0.5)
    x = x + F.linear(a, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"])
    x = F.layer_norm(x, (D,), sd[p + "self_attn_layer_norm.weight"], sd[p + "self_attn_layer_norm.bias"], eps)
    x = x + F.linear(gelu(F.linear(x, sd[p + "fc1.weight"], sd[p + "fc1.bias"])), sd[p + "fc2.weight"], sd[p + "fc2.bias"])
    return F.layer_norm(x, (D,), sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"], eps)


def wav2vec2_one(sd, cfg, wav):
    """wav [1, S] (raw) -> last hidden state [1, T, D]; ``sd``: the upstream's own names."""
    C, D, eps = cfg.conv_dim[-1], cfg.encoder_embed_dim, cfg.layer_norm_eps
    x = extractor(sd, cfg, wav)
    x = F.layer_norm(x, (C,), sd["layer_norm.weight"], sd["layer_norm.bias"], eps)
    x = F.linear(x, sd["post_extract_proj.weight"], sd["post_extract_proj.bias"])
    x = posconv(x, fold_wn(sd["encoder.pos_conv.0.weight_g"], sd["encoder.pos_conv.0.weight_v"]), sd["encoder.pos_conv.0.bias"],
                cfg.conv_pos_groups)
    x = F.layer_norm(x, (D,), sd["encoder.layer_norm.weight"], sd["encoder.layer_norm.bias"], eps)
    for i in range(cfg.encoder_layers):
        x = encoder_layer(sd, cfg, i, x)
    return x


def lstm_recurrence(xg, w_hh, lengths=None):
    """The hand loop.  xg [B, T, ND * 4 H] = x W_ih^T + b_ih + b_hh per direction (columns d 4 H + gate H + unit, gates i, f, g, o),
    w_hh [ND, 4 H, H] -> [B, T, ND H], zero initial state, packed-sequence semantics: direction 1 of row b starts at frame
    lengths[b] - 1; zero at and beyond lengths[b]."""
    B, T, _ = xg.shape
    ND, _, H = w_hh.shape
    out = xg.new_zeros(B, T, ND * H)
    for b in range(B):
        n = T if lengths is None else int(lengths[b])
        for d in range(ND):
            h, c = xg.new_zeros(H), xg.new_zeros(H)
            for t in (range(n) if d == 0 else range(n - 1, -1, -1)):
                i, f, g, o = (xg[b, t, d * 4 * H:(d + 1) * 4 * H] + w_hh[d] @ h).view(4, H)
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                h = torch.sigmoid(o) * torch.tanh(c)
                out[b, t, d * H:(d + 1) * H] = h
    return out


def lstm(x, sd, prefix="blstm.", lengths=None, bidirectional=True):
    """``nn.LSTM(batch_first=True)`` on x [B, T, In] with the parameters ``prefix + weight_ih_l0[_reverse]`` ... of ``sd``."""
    xg, w_hh = [], []
    for sfx in (("", "_reverse") if bidirectional else ("",)):
        xg.append(F.linear(x, sd[prefix + "weight_ih_l0" + sfx], sd[prefix + "bias_ih_l0" + sfx] + sd[prefix + "bias_hh_l0" + sfx]))
        w_hh.append(sd[prefix + "weight_hh_l0" + sfx])
    return lstm_recurrence(torch.cat(xg, -1), torch.stack(w_hh), lengths)


def head(sd, hidden, frames=None):
    """hidden [B, T, D] -> (blstm [B, T, 2 H], frame scores [B, T], scores [B]); zero beyond frames[b]."""
    B, T, _ = hidden.shape
    cond = torch.cat([sd["domain_emb"][0], sd["judge_emb"][0]]).expand(B, T, -1)
    h = lstm(torch.cat([hidden, cond], -1), sd, lengths=frames)
    y = F.linear(torch.relu(F.linear(h, sd["projection.0.weight"], sd["projection.0.bias"])), sd["projection.2.weight"],
                 sd["projection.2.bias"])[..., 0]
    n = torch.tensor([T] * B if frames is None else [int(v) for v in frames])
    y = y * (torch.arange(T)[None] < n[:, None]).to(y.dtype)
    return h, y, y.sum(1) / n.to(y.dtype) * 2.0 + 3.0


def predict(sd, cfg, wav, lengths=None):
    """wav [B, S] -> dict(hidden [B, T, D], blstm, frame_scores [B, T], scores [B], frames list), every row its own B = 1 run."""
    B, S = wav.shape
    lengths = [S] * B if lengths is None else [int(v) for v in lengths]
    frames = [frame_counts(n, cfg)[-1] for n in lengths]
    T = frame_counts(S, cfg)[-1]
    up = {k[len("wav2vec2."):]: v for k, v in sd.items() if k.startswith("wav2vec2.")}
    hidden = wav.new_zeros(B, T, cfg.encoder_embed_dim)
    for b in range(B):
        hidden[b, :frames[b]] = wav2vec2_one(up, cfg, wav[b:b + 1, :lengths[b]])[0]
    h, y, s = head(sd, hidden, frames)
    return dict(hidden=hidden, blstm=h, frame_scores=y, scores=s, frames=frames)
