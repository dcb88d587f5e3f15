"""fp32 restatement of ``MMDiT.forward`` (reference model/backbones/mmdit.py:147-188, MMDiTBlock and JointAttnProcessor of
model/modules.py:510-604, 647-718) on a plain state dict, that the MMDiT tests compare the HIP path with.  Test code only:
the product never imports it.  Built from the oracle's per-op restatements (time embedding, ConvPositionEmbedding, RoPE,
RMSNorm)."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from oracle import f5e_oracle as O


def text_embedding(sd, text: torch.Tensor, drop_text: bool, mask_padding: bool) -> torch.Tensor:
    """mmdit.py TextEmbedding: ids + 1, embedding + freqs_cis[min(pos, 1023)], filler positions zeroed; no ConvNeXt, the
    text keeps its own length."""
    ids = text.long() + 1
    keep = ids != 0
    if drop_text:
        ids = torch.zeros_like(ids)
    table = sd["text_embed.text_embed.weight"]
    h = table[ids]
    nt = ids.shape[1]
    pos = O.text_pos_table(table.shape[1], 1024)[torch.clamp(torch.arange(nt), max=1023)]
    h = h + pos[None]
    if mask_padding:
        h = h.masked_fill(~keep.unsqueeze(-1), 0.0)
    return h


def audio_embedding(sd, x: torch.Tensor, cond: torch.Tensor, drop_audio_cond: bool) -> torch.Tensor:
    if drop_audio_cond:
        cond = torch.zeros_like(cond)
    h = F.linear(torch.cat((x, cond), dim=-1), sd["audio_embed.linear.weight"], sd["audio_embed.linear.bias"])
    return O.conv_pos_embedding(sd, "audio_embed.conv_pos_embed.", h) + h


def _heads(t: torch.Tensor, heads: int) -> torch.Tensor:
    b, n, inner = t.shape
    return t.view(b, n, heads, inner // heads).transpose(1, 2)


def joint_attention(sd, p: str, x, c, heads: int, mask: Optional[torch.Tensor], fx, fc, context_pre_only: bool):
    """JointAttnProcessor.__call__: both streams project, norm and rotate separately, attend over the concatenated keys
    (audio keys masked past the mask, text keys never), and split again."""
    def proj(h, sfx):
        return [_heads(F.linear(h, sd[f"{p}to_{n}{sfx}.weight"], sd[f"{p}to_{n}{sfx}.bias"]), heads) for n in "qkv"]

    q, k, v = proj(x, "")
    qc, kc, vc = proj(c, "_c")
    if p + "q_norm.weight" in sd:
        q, k = O.rms_norm(q, sd[p + "q_norm.weight"]), O.rms_norm(k, sd[p + "k_norm.weight"])
        qc, kc = O.rms_norm(qc, sd[p + "c_q_norm.weight"]), O.rms_norm(kc, sd[p + "c_k_norm.weight"])
    q, k = O.apply_rope(q, fx), O.apply_rope(k, fx)
    qc, kc = O.apply_rope(qc, fc), O.apply_rope(kc, fc)
    qa, ka, va = torch.cat([q, qc], 2), torch.cat([k, kc], 2), torch.cat([v, vc], 2)
    s = qa @ ka.transpose(-1, -2) * (q.shape[-1] ** -0.5)
    if mask is not None:
        km = F.pad(mask, (0, c.shape[1]), value=True)
        s = s.masked_fill(~km[:, None, None, :], float("-inf"))
    o = torch.softmax(s, -1) @ va
    b, n = x.shape[:2]
    o = o.transpose(1, 2).reshape(b, -1, o.shape[1] * o.shape[-1])
    ox, oc = o[:, :n], o[:, n:]
    ox = F.linear(ox, sd[p + "to_out.0.weight"], sd[p + "to_out.0.bias"])
    oc = None if context_pre_only else F.linear(oc, sd[p + "to_out_c.weight"], sd[p + "to_out_c.bias"])
    if mask is not None:
        ox = ox.masked_fill(~mask.unsqueeze(-1), 0.0)
    return ox, oc


def _ff(sd, p, h):
    h = F.gelu(F.linear(h, sd[p + "ff.0.0.weight"], sd[p + "ff.0.0.bias"]), approximate="tanh")
    return F.linear(h, sd[p + "ff.2.weight"], sd[p + "ff.2.bias"])


def _ln(h):
    return F.layer_norm(h, (h.shape[-1],), eps=1e-6)


def mmdit_block(sd, p: str, x, c, t, heads: int, mask, fx, fc, context_pre_only: bool):
    """MMDiTBlock.forward -> (c or None, x)."""
    ec = F.linear(F.silu(t), sd[p + "attn_norm_c.linear.weight"], sd[p + "attn_norm_c.linear.bias"])
    if context_pre_only:
        scale, shift = torch.chunk(ec, 2, dim=1)             # AdaLayerNorm_Final: (scale, shift)
        norm_c = _ln(c) * (1 + scale[:, None]) + shift[:, None]
    else:
        c_shift_msa, c_scale_msa, c_gate_msa, c_shift_mlp, c_scale_mlp, c_gate_mlp = torch.chunk(ec, 6, dim=1)
        norm_c = _ln(c) * (1 + c_scale_msa[:, None]) + c_shift_msa[:, None]
    ex = F.linear(F.silu(t), sd[p + "attn_norm_x.linear.weight"], sd[p + "attn_norm_x.linear.bias"])
    shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = torch.chunk(ex, 6, dim=1)
    norm_x = _ln(x) * (1 + scale_msa[:, None]) + shift_msa[:, None]
    ax, ac = joint_attention(sd, p + "attn.", norm_x, norm_c, heads, mask, fx, fc, context_pre_only)
    if context_pre_only:
        c = None
    else:
        c = c + c_gate_msa.unsqueeze(1) * ac
        h = _ln(c) * (1 + c_scale_mlp[:, None]) + c_shift_mlp[:, None]
        c = c + c_gate_mlp.unsqueeze(1) * _ff(sd, p + "ff_c.", h)
    x = x + gate_msa.unsqueeze(1) * ax
    h = _ln(x) * (1 + scale_mlp[:, None]) + shift_mlp[:, None]
    x = x + gate_mlp.unsqueeze(1) * _ff(sd, p + "ff_x.", h)
    return c, x


def mmdit_forward(sd, heads: int, x, cond, text, time, drop_audio_cond: bool, drop_text: bool,
                  mask: Optional[torch.Tensor] = None, text_mask_padding: bool = True) -> torch.Tensor:
    """MMDiT.forward: x, cond [b, n, mel]; text int [b, nt] (-1 = padding); time 0-dim or [b] -> [b, n, mel]."""
    sd = {k: v.float() if v.is_floating_point() else v for k, v in sd.items()}
    b = x.shape[0]
    if time.ndim == 0:
        time = time.repeat(b)
    t = O.time_embedding(sd, time.float())
    c = text_embedding(sd, text, drop_text, text_mask_padding)
    x = audio_embedding(sd, x.float(), cond.float(), drop_audio_cond)
    inv = sd["rotary_embed.inv_freq"]
    fx, fc = O.rope_freqs(x.shape[1], inv_freq=inv), O.rope_freqs(text.shape[1], inv_freq=inv)
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("transformer_blocks."))
    for i in range(depth):
        c, x = mmdit_block(sd, f"transformer_blocks.{i}.", x, c, t, heads, mask, fx, fc, i == depth - 1)
    e = F.linear(F.silu(t), sd["norm_out.linear.weight"], sd["norm_out.linear.bias"])
    scale, shift = torch.chunk(e, 2, dim=1)
    x = _ln(x) * (1 + scale[:, None]) + shift[:, None]
    return F.linear(x, sd["proj_out.weight"], sd["proj_out.bias"])
