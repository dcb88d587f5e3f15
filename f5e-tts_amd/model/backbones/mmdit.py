"""MMDiT mirror (reference model/backbones/mmdit.py): constructor signature, exact ``state_dict`` keys and the inference
``forward`` (audio stream x and text stream c through joint-attention blocks) on libf5e_hip.so.

Like UNetT, MMDiT is not on the sampled path: the reference's samplers only ever call ``transformer.sample``, which exists
on DiT alone.  It is built from the DiT block kernels (AdaLN LayerNorm, QKV + RoPE GEMM, gated residual GEMM,
feed-forward) run once per stream, plus f5e_joint_attn for the attention over the concatenated audio and text keys."""
from __future__ import annotations

import math

import torch
from torch import nn

from ... import _C, ops
from ...engine import text_pos_table
from ..modules import AdaLayerNorm_Final, ConvPositionEmbedding, MMDiTBlock, TimestepEmbedding
from .dit import RotaryEmbedding

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32


class TextEmbedding(nn.Module):
    """reference mmdit.py TextEmbedding: no ConvNeXt; sinusoidal positions clamped to precompute_max_pos - 1; the text
    keeps its own length (no padding to the audio length)."""

    def __init__(self, out_dim, text_num_embeds, mask_padding=True):
        super().__init__()
        self.text_embed = nn.Embedding(text_num_embeds + 1, out_dim)  # index 0 = filler token
        self.mask_padding = mask_padding
        self.precompute_max_pos = 1024
        self.register_buffer("freqs_cis", text_pos_table(out_dim, self.precompute_max_pos), persistent=False)


class AudioEmbedding(nn.Module):
    """reference mmdit.py AudioEmbedding: Linear(2 mel -> dim) of (x, cond), then ConvPositionEmbedding + residual."""

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.linear = nn.Linear(2 * in_dim, out_dim)
        self.conv_pos_embed = ConvPositionEmbedding(out_dim)


class MMDiT(nn.Module):
    def __init__(self, *, dim, depth=8, heads=8, dim_head=64, dropout=0.1, ff_mult=4, mel_dim=100, text_num_embeds=256,
                 text_mask_padding=True, qk_norm=None):
        super().__init__()
        self.time_embed = TimestepEmbedding(dim)
        self.text_embed = TextEmbedding(dim, text_num_embeds, mask_padding=text_mask_padding)
        self.text_cond, self.text_uncond = None, None  # text cache
        self.audio_embed = AudioEmbedding(mel_dim, dim)
        self.rotary_embed = RotaryEmbedding(dim_head)
        self.dim, self.depth = dim, depth
        self.transformer_blocks = nn.ModuleList(
            [MMDiTBlock(dim=dim, heads=heads, dim_head=dim_head, dropout=dropout, ff_mult=ff_mult,
                        context_pre_only=i == depth - 1, qk_norm=qk_norm) for i in range(depth)])
        self.norm_out = AdaLayerNorm_Final(dim)  # final modulation
        self.proj_out = nn.Linear(dim, mel_dim)
        self.initialize_weights()

    def initialize_weights(self):
        """AdaLN-zero init (reference mmdit.py:124-136)."""
        for block in self.transformer_blocks:
            nn.init.constant_(block.attn_norm_x.linear.weight, 0)
            nn.init.constant_(block.attn_norm_x.linear.bias, 0)
            nn.init.constant_(block.attn_norm_c.linear.weight, 0)
            nn.init.constant_(block.attn_norm_c.linear.bias, 0)
        nn.init.constant_(self.norm_out.linear.weight, 0)
        nn.init.constant_(self.norm_out.linear.bias, 0)
        nn.init.constant_(self.proj_out.weight, 0)
        nn.init.constant_(self.proj_out.bias, 0)

    def clear_cache(self):
        self.text_cond, self.text_uncond = None, None

    # ------------------------------------------------------------------ HIP forward

    def _packed(self):
        tensors = list(self.parameters()) + list(self.buffers())
        dv = tensors[0].device
        sig = tuple((t.data_ptr(), t._version) for t in tensors) + (str(dv),)
        if getattr(self, "_pack", None) is None or self._pack[0] != sig:
            if dv.type != "cuda":
                raise _C.F5EError(f"MMDiT lives on {dv}: move it to the GPU (there is no CPU path)")
            f = lambda t: t.detach().to(dv, F32).contiguous()  # noqa: E731

            def qkv(a, sfx):
                return (torch.cat([f(getattr(a, f"to_{n}{sfx}").weight) for n in "qkv"], 0).to(BF),
                        torch.cat([f(getattr(a, f"to_{n}{sfx}").bias) for n in "qkv"], 0))

            def ff(m):
                return f(m.ff[0][0].weight).to(BF), f(m.ff[0][0].bias), f(m.ff[2].weight).to(BF), f(m.ff[2].bias)

            blocks = []
            for blk in self.transformer_blocks:
                a = blk.attn
                L = dict(last=blk.context_pre_only,
                         ada_x=(f(blk.attn_norm_x.linear.weight), f(blk.attn_norm_x.linear.bias)),
                         ada_c=(f(blk.attn_norm_c.linear.weight), f(blk.attn_norm_c.linear.bias)),
                         qkv_x=qkv(a, ""), qkv_c=qkv(a, "_c"),
                         norm_x=(f(a.q_norm.weight), f(a.k_norm.weight)) if a.q_norm is not None else (None, None),
                         norm_c=(f(a.c_q_norm.weight), f(a.c_k_norm.weight)) if a.c_q_norm is not None else (None, None),
                         out_x=(f(a.to_out[0].weight).to(BF), f(a.to_out[0].bias)), ff_x=ff(blk.ff_x))
                if not blk.context_pre_only:
                    L.update(out_c=(f(a.to_out_c.weight).to(BF), f(a.to_out_c.bias)), ff_c=ff(blk.ff_c))
                blocks.append(L)
            tm = self.time_embed.time_mlp
            half = 128
            cp = self.audio_embed.conv_pos_embed.conv1d
            self._pack = (sig, dict(
                sinus_freqs=torch.exp(torch.arange(half).float() * -(math.log(10000) / (half - 1))).to(dv),
                tm=(f(tm[0].weight), f(tm[0].bias), f(tm[2].weight), f(tm[2].bias)),
                text_table=f(self.text_embed.text_embed.weight), text_pos=f(self.text_embed.freqs_cis),
                w_in=f(self.audio_embed.linear.weight), b_in=f(self.audio_embed.linear.bias),
                cp=[(ops.pack_convpos_weight(f(cp[j].weight), 16), f(cp[j].bias)) for j in (0, 2)],
                inv_freq=f(self.rotary_embed.inv_freq), blocks=blocks,
                final=(f(self.norm_out.linear.weight), f(self.norm_out.linear.bias)),
                w_proj=f(self.proj_out.weight).to(BF), b_proj=f(self.proj_out.bias)))
        return self._pack[1]

    def _text_embed(self, P, text, drop_text):
        """TextEmbedding.forward (reference mmdit.py:38-61) -> f32 [b * nt, dim]."""
        dv = P["text_table"].device
        if text.device.type == "cpu" and text.numel():
            hi, lo = int(text.max()), int(text.min())
            if hi + 1 >= P["text_table"].shape[0] or lo < -1:   # nn.Embedding raises IndexError here
                raise IndexError(f"index out of range in self: token id {hi if lo >= -1 else lo} with text_num_embeds = "
                                 f"{P['text_table'].shape[0] - 1}")
        ids = text.to(dv).long() + 1
        keep = (ids != 0).to(F32).contiguous() if self.text_embed.mask_padding else None   # taken before the drop
        if drop_text:
            ids = torch.zeros_like(ids)
        B, nt = ids.shape
        out = torch.empty(B, nt, self.dim, device=dv)
        ops.text_gather(ids.to(I32).contiguous(), P["text_table"], P["text_pos"], keep, out)
        return out.view(B * nt, self.dim)

    @torch.no_grad()
    def forward(self, x, cond, text, time, drop_audio_cond, drop_text, mask=None, cache=False):
        """reference mmdit.py:147-188.  x, cond [b, n, mel]; text int [b, nt] (-1 = padding); time 0-dim or [b];
        mask bool [b, n] (lens_to_mask form) or None -> [b, n, mel] f32."""
        D = self.dim
        blk0 = self.transformer_blocks[0]
        H = blk0.attn.heads
        if D % 256 or D > 2048:
            raise _C.F5EError(f"MMDiT.forward: the LayerNorm kernel takes dim % 256 == 0 and dim <= 2048 (got {D})")
        if blk0.attn.inner_dim != 64 * H:
            raise _C.F5EError("MMDiT.forward: the attention kernels are built for dim_head = 64")
        P = self._packed()
        dv = P["text_table"].device
        B, N, mel = x.shape
        nt = text.shape[1]
        if nt < 1:
            raise _C.F5EError("MMDiT.forward: the text stream needs at least one token")
        if time.ndim == 0:
            time = time.repeat(B)
        # time embedding (modules.py:721-731)
        sin = torch.empty(B, 256, device=dv)
        ops.sinus_embed(time.to(dv, F32).contiguous(), P["sinus_freqs"], sin)
        h = torch.empty(B, D, device=dv)
        ops.gemm_f32(sin, P["tm"][0], P["tm"][1], out=h, act=ops.ACT_SILU)
        t = torch.empty(B, D, device=dv)
        ops.gemm_f32(h, P["tm"][2], P["tm"][3], out=t)
        # text stream (cached per drop flag when asked, as the reference does)
        if cache:
            attr = "text_uncond" if drop_text else "text_cond"
            if getattr(self, attr) is None:
                setattr(self, attr, self._text_embed(P, text, drop_text))
            C = getattr(self, attr).clone()     # the blocks update the stream in place
        else:
            C = self._text_embed(P, text, drop_text)
        # audio stream: Linear of (x, cond) + ConvPositionEmbedding + residual
        xin = x.to(dv, F32).reshape(B * N, mel).contiguous()
        h0 = torch.empty(B * N, D, device=dv)
        h0b = torch.empty(B * N, D, device=dv, dtype=BF)
        if drop_audio_cond:
            ops.gemm_f32(xin, P["w_in"][:, :mel], P["b_in"], out=h0, out_bf16=h0b)
        else:
            hc = torch.empty(B * N, D, device=dv)
            ops.gemm_f32(cond.to(dv, F32).reshape(B * N, mel).contiguous(), P["w_in"][:, mel:], P["b_in"], out=hc)
            ops.gemm_f32(xin, P["w_in"][:, :mel], None, out=h0, out_bf16=h0b, addend=hc)
        c1 = torch.empty_like(h0b)
        X = torch.empty_like(h0)
        ops.convpos(h0b, P["cp"][0][0], P["cp"][0][1], B, N, out_bf16=c1)
        ops.convpos(c1, P["cp"][1][0], P["cp"][1][1], B, N, out_f32=X, resid=h0)
        lens = None
        if mask is not None:
            lens = mask.sum(-1).to(dv, I32).contiguous()
            if not torch.equal(mask.to(dv), torch.arange(N, device=dv)[None] < lens[:, None]):
                raise _C.F5EError("MMDiT.forward takes key-padding masks of the lens_to_mask form only")
        # each stream rotates from its own position 0 (mmdit.py:180-181)
        cs_x = torch.empty(N, 32, 2, device=dv)
        cs_c = torch.empty(nt, 32, 2, device=dv)
        ops.rope_table(P["inv_freq"], cs_x)
        ops.rope_table(P["inv_freq"], cs_c)
        npx, npc = (N + 63) // 64 * 64, (nt + 63) // 64 * 64
        qx = torch.zeros(B, H, npx, 64, device=dv, dtype=BF)
        kx, vx = torch.zeros_like(qx), torch.zeros_like(qx)
        qc = torch.zeros(B, H, npc, 64, device=dv, dtype=BF)
        kc, vc = torch.zeros_like(qc), torch.zeros_like(qc)
        hx = torch.empty(B * N, D, device=dv, dtype=BF)
        hcn = torch.empty(B * nt, D, device=dv, dtype=BF)
        ax = torch.empty(B * N, H * 64, device=dv, dtype=BF)
        ac = torch.empty(B * nt, H * 64, device=dv, dtype=BF)

        def feed_forward(hn, S, w, resid, gate, rows):
            ff = torch.empty(S, w[0].shape[0], device=dv, dtype=BF)
            ops.gemm_bf16_bias(hn, w[0], w[1], ff, act=ops.ACT_GELU_TANH)
            ops.gemm_bf16_gate_residual(ff, w[2], w[3], resid, gate, rows)

        for L in P["blocks"]:   # MMDiTBlock.forward (modules.py:583-604)
            ex = torch.empty(B, 6 * D, device=dv)
            ops.gemm_f32(t, *L["ada_x"], out=ex, a_act=ops.ACT_SILU)
            ec = torch.empty(B, L["ada_c"][0].shape[0], device=dv)
            ops.gemm_f32(t, *L["ada_c"], out=ec, a_act=ops.ACT_SILU)
            ops.layernorm(X, hx, scale=ex[:, D:2 * D], shift=ex[:, 0:D], rows_per_seq=N)
            if L["last"]:   # AdaLayerNorm_Final: (scale, shift)
                ops.layernorm(C, hcn, scale=ec[:, 0:D], shift=ec[:, D:2 * D], rows_per_seq=nt)
            else:
                ops.layernorm(C, hcn, scale=ec[:, D:2 * D], shift=ec[:, 0:D], rows_per_seq=nt)
            ops.gemm_bf16_qkv_rope(hx, *L["qkv_x"], qx, kx, vx, H, H, cs_x, N, q_norm_w=L["norm_x"][0],
                                   k_norm_w=L["norm_x"][1])
            ops.gemm_bf16_qkv_rope(hcn, *L["qkv_c"], qc, kc, vc, H, H, cs_c, nt, q_norm_w=L["norm_c"][0],
                                   k_norm_w=L["norm_c"][1])
            ops.joint_attn(qx, kx, vx, qc, kc, vc, ax, None if L["last"] else ac, N, nt, kv_len=lens)
            # to_out with the reference's masked_fill of padded audio rows = rows past seq_len skipped
            ops.gemm_bf16_gate_residual(ax, *L["out_x"], X, ex[:, 2 * D:3 * D], N, seq_len=lens)
            if not L["last"]:
                ops.gemm_bf16_gate_residual(ac, *L["out_c"], C, ec[:, 2 * D:3 * D], nt)
                ops.layernorm(C, hcn, scale=ec[:, 4 * D:5 * D], shift=ec[:, 3 * D:4 * D], rows_per_seq=nt)
                feed_forward(hcn, B * nt, L["ff_c"], C, ec[:, 5 * D:6 * D], nt)
            ops.layernorm(X, hx, scale=ex[:, 4 * D:5 * D], shift=ex[:, 3 * D:4 * D], rows_per_seq=N)
            feed_forward(hx, B * N, L["ff_x"], X, ex[:, 5 * D:6 * D], N)
        ef = torch.empty(B, 2 * D, device=dv)
        ops.gemm_f32(t, *P["final"], out=ef, a_act=ops.ACT_SILU)
        ops.layernorm(X, hx, scale=ef[:, 0:D], shift=ef[:, D:2 * D], rows_per_seq=N)
        out = torch.empty(B * N, mel, device=dv)
        ops.gemm_bf16_bias(hx, P["w_proj"], P["b_proj"], out)
        return out.view(B, N, mel)
