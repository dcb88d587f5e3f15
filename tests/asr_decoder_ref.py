"""torch fp64 restatement of the attention decoder of the ASR model (reference ppg/wenet/transformer/decoder.py:86-135,
decoder_layer.py:58-137, attention.py:79-111, pre-norm, concat_after False) and of the rescoring sum of
``ASRModel.attention_rescoring`` (ppg/asr_model.py:628-677).  Pinned against the reference's own outputs by
tests/golden/asr_decoder_*.npz (tests/golden/make_ctc_beam_golden.py); the GPU tests compare the device decoder to it."""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64


def _w(weights, key):
    v = weights[key]
    return (v if torch.is_tensor(v) else torch.from_numpy(v)).to(F64)


def pos_table(n, d):
    pe = torch.zeros(n, d, dtype=F64)
    pos = torch.arange(0, n, dtype=F64).unsqueeze(1)
    div = torch.exp(torch.arange(0, d, 2, dtype=F64) * -(math.log(10000.0) / d))
    pe[:, 0::2], pe[:, 1::2] = torch.sin(pos * div), torch.cos(pos * div)
    return pe


def attention(w, pre, q_in, kv_in, mask, heads):
    """MultiHeadedAttention.forward: q_in [N, Tq, D], kv_in [N, Tk, D], mask bool [N, Tq or 1, Tk] (True = visible)."""
    lin = lambda n, x: F.linear(x, _w(w, pre + f"linear_{n}.weight"), _w(w, pre + f"linear_{n}.bias"))   # noqa: E731
    N, Tq, D = q_in.shape
    dk = D // heads
    split = lambda x: x.view(N, -1, heads, dk).transpose(1, 2)                                             # noqa: E731
    q, k, v = split(lin("q", q_in)), split(lin("k", kv_in)), split(lin("v", kv_in))
    scores = q @ k.transpose(-2, -1) / math.sqrt(dk)
    hide = ~mask.unsqueeze(1)
    attn = torch.softmax(scores.masked_fill(hide, -float("inf")), dim=-1).masked_fill(hide, 0.0)
    return lin("out", (attn @ v).transpose(1, 2).reshape(N, Tq, D))


def decoder_forward(w, pre, memory, ys_in, ys_len, heads, mem_len=None):
    """TransformerDecoder.forward: w = state dict (numpy or torch), pre = "decoder." / "decoder.left_decoder." / ...;
    memory [N, T, D] (or [1, T, D], shared), ys_in long [N, U1], ys_len [N] -> logits f64 [N, U1, V]."""
    ys_in, ys_len = torch.as_tensor(ys_in).long(), torch.as_tensor(ys_len).long()
    N, U1 = ys_in.shape
    memory = torch.as_tensor(memory).to(F64).expand(N, -1, -1)
    T, D = memory.shape[1:]
    pad = torch.arange(U1)[None, :] < ys_len[:, None]                                   # [N, U1]
    tgt_mask = pad[:, None, :] & torch.tril(torch.ones(U1, U1, dtype=torch.bool))[None]
    mem_mask = torch.ones(N, 1, T, dtype=torch.bool) if mem_len is None else \
        (torch.arange(T)[None, :] < torch.as_tensor(mem_len).long()[:, None])[:, None, :]
    ln = lambda n, x: F.layer_norm(x, (D,), _w(w, n + ".weight"), _w(w, n + ".bias"), 1e-5)               # noqa: E731
    x = _w(w, pre + "embed.0.weight")[ys_in] * math.sqrt(D) + pos_table(U1, D)[None]
    i = 0
    while f"{pre}decoders.{i}.norm1.weight" in w:
        p = f"{pre}decoders.{i}."
        h = ln(p + "norm1", x)
        x = x + attention(w, p + "self_attn.", h, h, tgt_mask, heads)
        x = x + attention(w, p + "src_attn.", ln(p + "norm2", x), memory, mem_mask, heads)
        h = ln(p + "norm3", x)
        h = F.linear(torch.relu(F.linear(h, _w(w, p + "feed_forward.w_1.weight"), _w(w, p + "feed_forward.w_1.bias"))),
                     _w(w, p + "feed_forward.w_2.weight"), _w(w, p + "feed_forward.w_2.bias"))
        x = x + h
        i += 1
    x = ln(pre + "after_norm", x)
    return F.linear(x, _w(w, pre + "output_layer.weight"), _w(w, pre + "output_layer.bias"))


def inputs(hyps, sos, eos):
    """n-best ids -> (ys_in, r_ys_in long [N, U + 1]: sos + hyp / reversed hyp, eos-padded; lens [N] = len + 1)."""
    U1 = max(len(h) for h in hyps) + 1
    ys, r_ys = torch.full((len(hyps), U1), eos), torch.full((len(hyps), U1), eos)
    ys[:, 0] = r_ys[:, 0] = sos
    for i, h in enumerate(hyps):
        if len(h):
            ys[i, 1:len(h) + 1] = torch.tensor(h)
            r_ys[i, 1:len(h) + 1] = torch.tensor(h[::-1])
    return ys, r_ys, torch.tensor([len(h) + 1 for h in hyps])


def rescoring_scores(hyps, ctc_scores, logp, r_logp, eos, ctc_weight=0.0, reverse_weight=0.0):
    """The reference's double loop on log-softmaxed decoder outputs [N, U + 1, V] -> list of per-hypothesis scores."""
    out = []
    for i, h in enumerate(hyps):
        score = sum(float(logp[i][j][w]) for j, w in enumerate(h)) + float(logp[i][len(h)][eos])
        if reverse_weight > 0:
            r = sum(float(r_logp[i][len(h) - j - 1][w]) for j, w in enumerate(h)) + float(r_logp[i][len(h)][eos])
            score = score * (1 - reverse_weight) + r * reverse_weight
        out.append(score + ctc_scores[i] * ctc_weight)
    return out


def winner(scores):
    """The first maximum, as the reference's ``if score > best_score``."""
    best, best_i = -float("inf"), 0
    for i, s in enumerate(scores):
        if s > best:
            best, best_i = s, i
    return best_i
