"""Seeded synthetic weights and inputs: F5TTS-shaped state dicts with the reference's
checkpoint key names, a random-init Vocos, band-limited reference waves and token ids.

NEUTRAL module: neither product code (``f5e-tts_amd/`` never imports it) nor part of the oracle.  ``bench.py``,
``tests/``, ``__graft_entry__.smoke()`` and the scripts under ``tools/`` use it to build identical inputs for the HIP path
and for the CPU oracle.  ``cfg`` is any object with the DiT architecture attributes (``oracle.f5e_oracle.DiTConfig`` or
``f5e_tts_amd.engine.DiTConfig``).
"""
from __future__ import annotations

import math
from typing import Dict

import torch
import torch.nn.functional as F

Tensor = torch.Tensor
State = Dict[str, Tensor]


class DiTConfig:
    """Architecture attributes of a DiT (reference backbones/dit.py:184-204 keyword names); defaults = F5TTS_v1_Base."""

    def __init__(self, dim=1024, depth=22, heads=16, dim_head=64, ff_mult=2, mel_dim=100, text_num_embeds=2545,
                 text_dim=512, text_mask_padding=True, qk_norm=None, conv_layers=4, pe_attn_head=None,
                 long_skip_connection=False, use_ppg=False, ppg_dim=256, conv_groups=16, ppg_transformer=False,
                 ppg_heads=4, ppg_ff=512, ppg_layers=2):
        self.__dict__.update(locals())
        del self.__dict__["self"]


def init_dit_state(cfg, seed: int = 1234, std_zeroed: float = 0.02) -> State:
    """Seeded random F5TTS-shaped state dict with the reference's key names.

    nn.Linear/Conv default-init scale (U(-1/sqrt(fan_in), +)) for ordinary layers; the tensors the
    reference zero-initialises (backbones/dit.py:273-283) get N(0, std_zeroed).
    """
    g = torch.Generator().manual_seed(seed)
    sd: State = {}

    def uni(shape, fan_in):
        bound = 1.0 / math.sqrt(fan_in)
        return (torch.rand(shape, generator=g) * 2 - 1) * bound

    def lin(name, out_f, in_f, bias=True):
        sd[name + ".weight"] = uni((out_f, in_f), in_f)
        if bias:
            sd[name + ".bias"] = uni((out_f,), in_f)

    def nrm(name, out_f, in_f):
        sd[name + ".weight"] = torch.randn((out_f, in_f), generator=g) * std_zeroed
        sd[name + ".bias"] = torch.randn((out_f,), generator=g) * std_zeroed

    d, td = cfg.dim, cfg.text_dim
    lin("time_embed.time_mlp.0", d, 256)
    lin("time_embed.time_mlp.2", d, d)
    sd["text_embed.text_embed.weight"] = torch.randn((cfg.text_num_embeds + 1, td), generator=g)
    for i in range(cfg.conv_layers):
        p = f"text_embed.text_blocks.{i}."
        sd[p + "dwconv.weight"] = uni((td, 1, 7), 7)
        sd[p + "dwconv.bias"] = uni((td,), 7)
        sd[p + "norm.weight"] = 1.0 + 0.1 * torch.randn((td,), generator=g)
        sd[p + "norm.bias"] = 0.1 * torch.randn((td,), generator=g)
        lin(p + "pwconv1", 2 * td, td)
        sd[p + "grn.gamma"] = 0.1 * torch.randn((1, 1, 2 * td), generator=g)
        sd[p + "grn.beta"] = 0.1 * torch.randn((1, 1, 2 * td), generator=g)
        lin(p + "pwconv2", td, 2 * td)
    if cfg.use_ppg and getattr(cfg, "ppg_transformer", False):   # PPGEmbedding(use_transformer=True), dit.py:105-119
        pd, pp = cfg.ppg_dim, "ppg_embed.ppg_proj."
        for i in range(cfg.ppg_layers):
            q = pp + f"0.layers.{i}."
            sd[q + "self_attn.in_proj_weight"] = uni((3 * pd, pd), pd)
            sd[q + "self_attn.in_proj_bias"] = uni((3 * pd,), pd)
            lin(q + "self_attn.out_proj", pd, pd)
            lin(q + "linear1", cfg.ppg_ff, pd)
            lin(q + "linear2", pd, cfg.ppg_ff)
            for n_ in ("norm1", "norm2"):
                sd[q + n_ + ".weight"] = 1.0 + 0.1 * torch.randn((pd,), generator=g)
                sd[q + n_ + ".bias"] = 0.1 * torch.randn((pd,), generator=g)
        lin(pp + "1", td, pd)
    elif cfg.use_ppg:
        pd = cfg.ppg_dim
        pp = "ppg_embed.ppg_proj."
        lin(pp + "0", pd, pd)
        for conv_i, bn_i in ((2, 3), (6, 7), (10, 11)):
            sd[pp + f"{conv_i}.weight"] = uni((pd, pd, 5), pd * 5)
            sd[pp + f"{conv_i}.bias"] = uni((pd,), pd * 5)
            sd[pp + f"{bn_i}.weight"] = 1.0 + 0.1 * torch.randn((pd,), generator=g)
            sd[pp + f"{bn_i}.bias"] = 0.1 * torch.randn((pd,), generator=g)
            sd[pp + f"{bn_i}.running_mean"] = 0.1 * torch.randn((pd,), generator=g)
            sd[pp + f"{bn_i}.running_var"] = 1.0 + 0.2 * torch.rand((pd,), generator=g)
            sd[pp + f"{bn_i}.num_batches_tracked"] = torch.tensor(0, dtype=torch.long)
        lin(pp + "15", td, pd)
    in_dim = cfg.mel_dim * 2 + td * (2 if cfg.use_ppg else 1)
    lin("input_embed.proj", d, in_dim)
    cg = d // getattr(cfg, "conv_groups", 16)
    for j in (0, 2):
        sd[f"input_embed.conv_pos_embed.conv1d.{j}.weight"] = uni((d, cg, 31), cg * 31)
        sd[f"input_embed.conv_pos_embed.conv1d.{j}.bias"] = uni((d,), cg * 31)
    sd["rotary_embed.inv_freq"] = 1.0 / (10000 ** (torch.arange(0, getattr(cfg, "dim_head", 64), 2).float() / getattr(cfg, "dim_head", 64)))
    inner = cfg.heads * getattr(cfg, "dim_head", 64)
    for i in range(cfg.depth):
        p = f"transformer_blocks.{i}."
        nrm(p + "attn_norm.linear", 6 * d, d)
        lin(p + "attn.to_q", inner, d)
        lin(p + "attn.to_k", inner, d)
        lin(p + "attn.to_v", inner, d)
        if cfg.qk_norm == "rms_norm":
            sd[p + "attn.q_norm.weight"] = 1.0 + 0.1 * torch.randn((getattr(cfg, "dim_head", 64),), generator=g)
            sd[p + "attn.k_norm.weight"] = 1.0 + 0.1 * torch.randn((getattr(cfg, "dim_head", 64),), generator=g)
        lin(p + "attn.to_out.0", d, inner)
        lin(p + "ff.ff.0.0", d * cfg.ff_mult, d)
        lin(p + "ff.ff.2", d, d * cfg.ff_mult)
    if cfg.long_skip_connection:
        lin("long_skip_connection", d, 2 * d, bias=False)
    nrm("norm_out.linear", 2 * d, d)
    nrm("proj_out", cfg.mel_dim, d)
    return sd


def init_vocos_state(seed: int = 4321, dim: int = 512, inter: int = 1536, layers: int = 8, n_mels: int = 100,
                     n_fft: int = 1024) -> State:
    """Random-init Vocos (charactr/vocos-mel-24khz architecture), gamma = 1/layers."""
    g = torch.Generator().manual_seed(seed)
    vs: State = {}

    def uni(shape, fan_in):
        bound = 1.0 / math.sqrt(fan_in)
        return (torch.rand(shape, generator=g) * 2 - 1) * bound

    vs["backbone.embed.weight"] = uni((dim, n_mels, 7), n_mels * 7)
    vs["backbone.embed.bias"] = uni((dim,), n_mels * 7)
    vs["backbone.norm.weight"] = torch.ones(dim)
    vs["backbone.norm.bias"] = torch.zeros(dim)
    for i in range(layers):
        p = f"backbone.convnext.{i}."
        vs[p + "dwconv.weight"] = uni((dim, 1, 7), 7)
        vs[p + "dwconv.bias"] = uni((dim,), 7)
        vs[p + "norm.weight"] = torch.ones(dim)
        vs[p + "norm.bias"] = torch.zeros(dim)
        vs[p + "pwconv1.weight"] = uni((inter, dim), dim)
        vs[p + "pwconv1.bias"] = uni((inter,), dim)
        vs[p + "pwconv2.weight"] = uni((dim, inter), inter)
        vs[p + "pwconv2.bias"] = uni((dim,), inter)
        vs[p + "gamma"] = torch.full((dim,), 1.0 / layers)
    vs["backbone.final_layer_norm.weight"] = torch.ones(dim)
    vs["backbone.final_layer_norm.bias"] = torch.zeros(dim)
    vs["head.out.weight"] = uni((n_fft + 2, dim), dim)
    vs["head.out.bias"] = uni((n_fft + 2,), dim)
    return vs


def synthetic_ref_wave(n_frames: int, seed: int = 2024, hop: int = 256, batch: int = 1) -> Tensor:
    """0.1*randn, 5-tap smoothed, RMS-normalised to 0.1; nw = hop*n_frames - 1 -> exactly n_frames mel frames
    when center=True (1 + nw // hop)."""
    g = torch.Generator().manual_seed(seed)
    nw = hop * (n_frames - 1) + hop // 2
    w = 0.1 * torch.randn((batch, nw + 4), generator=g)
    w = F.avg_pool1d(w[:, None], 5, stride=1)[:, 0]
    rms = w.pow(2).mean(dim=-1, keepdim=True).sqrt()
    return w * (0.1 / rms)


def synthetic_text_ids(n_total: int, batch: int = 1, seed: int = 7, vocab: int = 2545) -> Tensor:
    """Uniform ids in [1, vocab-1], nt = round(N/8)."""
    g = torch.Generator().manual_seed(seed)
    nt = max(1, round(n_total / 8))
    return torch.randint(1, vocab, (batch, nt), generator=g)


def bigvgan_config(initial_channel: int = 1536, **kw) -> Dict:
    """BigVGAN-v2 24 kHz / 100-band / 256x config.json fields (smaller ``initial_channel`` for quick tests)."""
    cfg = dict(num_mels=100, upsample_initial_channel=initial_channel, upsample_rates=[4, 4, 2, 2, 2, 2],
               upsample_kernel_sizes=[8, 8, 4, 4, 4, 4], resblock="1", resblock_kernel_sizes=[3, 7, 11],
               resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], activation="snakebeta", snake_logscale=True,
               use_tanh_at_final=False, use_bias_at_final=False, sampling_rate=24000, hop_size=256, n_fft=1024,
               win_size=1024, fmin=0, fmax=None)
    cfg.update(kw)
    return cfg


def init_bigvgan_state(cfg: Dict, seed: int = 777, weight_norm_form: str = "weight_g",
                       post_gain: float = 0.09) -> State:
    """Seeded BigVGAN generator state dict with the package's key names (weight-norm form ``weight_g`` -> weight_g /
    weight_v, ``parametrizations`` -> parametrizations.weight.original0 / 1).  Activations stay O(1) through all stages:
    every conv has std ~ 0.5 / sqrt(C_in k) (weight_v random, weight_g rescales it), the SnakeBeta log-parameters are
    N(0, 0.1), and conv_post has std post_gain / sqrt(C k), which keeps the waveform RMS near 0.2 without clipping (the
    package's normal(0, 0.01) init decays the signal toward zero and would make parity checks vacuous)."""
    g = torch.Generator().manual_seed(seed)
    sd: State = {}

    def conv(prefix, cout, cin, k, std, bias=True, transposed=False):
        shape = (cin, cout, k) if transposed else (cout, cin, k)
        v = torch.randn(shape, generator=g)
        gn = v.flatten(1).norm(dim=1).view(-1, 1, 1) * std   # folded weight g v / ||v|| = std * v
        if weight_norm_form == "weight_g":
            sd[f"{prefix}.weight_g"], sd[f"{prefix}.weight_v"] = gn, v
        else:
            sd[f"{prefix}.parametrizations.weight.original0"] = gn
            sd[f"{prefix}.parametrizations.weight.original1"] = v
        if bias:
            sd[f"{prefix}.bias"] = 0.02 * torch.randn(cout, generator=g)

    def act(prefix, c):
        sd[f"{prefix}.act.alpha"] = 0.1 * torch.randn(c, generator=g)
        if cfg["activation"] == "snakebeta":
            sd[f"{prefix}.act.beta"] = 0.1 * torch.randn(c, generator=g)

    c = cfg["upsample_initial_channel"]
    conv("conv_pre", c, cfg["num_mels"], 7, 0.5 / math.sqrt(cfg["num_mels"] * 7))
    nk = len(cfg["resblock_kernel_sizes"])
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        # a transposed conv sums k / u taps per output: scale for that fan-in
        conv(f"ups.{i}.0", c // 2, c, k, 1.0 / math.sqrt(c * k / u), transposed=True)
        c //= 2
        for j, (kr, dils) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            r = i * nk + j
            for m in range(len(dils)):
                conv(f"resblocks.{r}.convs1.{m}", c, c, kr, 0.5 / math.sqrt(c * kr))
                conv(f"resblocks.{r}.convs2.{m}", c, c, kr, 0.5 / math.sqrt(c * kr))
            for n in range(2 * len(dils)):
                act(f"resblocks.{r}.activations.{n}", c)
    act("activation_post", c)
    conv("conv_post", 1, c, 7, post_gain / math.sqrt(c * 7), bias=bool(cfg["use_bias_at_final"]))
    return sd


def synthetic_mel(n_frames: int, batch: int = 1, seed: int = 99, n_mels: int = 100) -> Tensor:
    """Log-mel-like input [batch, n_mels, n_frames]: a smooth spectral envelope around -4 plus noise."""
    g = torch.Generator().manual_seed(seed)
    env = torch.linspace(-2.0, -7.0, n_mels).view(1, n_mels, 1)
    slow = F.interpolate(torch.randn(batch, n_mels, max(2, n_frames // 8), generator=g), size=n_frames, mode="linear",
                         align_corners=True)
    return (env + 1.5 * slow + 0.5 * torch.randn(batch, n_mels, n_frames, generator=g)).float()


def whisper_config_fields(large: str = "large-v3", **kw) -> Dict:
    """The config.json / generation_config.json fields of whisper-large-v3 or -large-v3-turbo (public model cards) that
    ``f5e_tts_amd.eval.whisper.WhisperConfig`` takes; ``kw`` overrides (fewer layers for quick runs)."""
    f = dict(vocab_size=51866, num_mel_bins=128, d_model=1280, encoder_layers=32, encoder_attention_heads=20, encoder_ffn_dim=5120,
             decoder_layers=4 if large == "large-v3-turbo" else 32, decoder_attention_heads=20, decoder_ffn_dim=5120,
             max_source_positions=1500, max_target_positions=448, eos_token_id=50257, decoder_start_token_id=50258,
             suppress_tokens=(1, 2, 7, 8, 9, 10, 14, 25, 50258, 50359, 50360, 50361, 50362, 50363), begin_suppress_tokens=(220, 50257),
             lang_to_id={"<|en|>": 50259, "<|zh|>": 50260}, task_to_id={"translate": 50359, "transcribe": 50360},
             no_timestamps_token_id=50364)
    f.update(kw)
    return f


def init_whisper_state(shapes: Dict[str, tuple], seed: int = 99, gain: float = 1.0, device="cpu") -> State:
    """Seeded weights for the Hugging Face parameter names of a Whisper (``shapes``: name -> shape, e.g. from a fresh module's
    ``state_dict()``): matrices N(0, gain / fan_in), biases N(0, 0.02), LayerNorm weights 1 + N(0, 0.1), token embedding
    N(0, 0.02 gain), decoder positions N(0, 0.02); the encoder's sinusoids are left to the module (not returned).  ``device``:
    where the draws are made (the full-size models have 1.5e9 parameters; a GPU stream of draws differs from the CPU's)."""
    g = torch.Generator(device=device).manual_seed(seed)
    out = {}
    for name, shape in shapes.items():
        shape = tuple(shape)
        if name == "model.encoder.embed_positions.weight":
            continue
        r = torch.randn(shape, generator=g, device=device)
        if "layer_norm" in name:
            out[name] = 1.0 + 0.1 * r if name.endswith("weight") else 0.1 * r
        elif name.endswith("embed_tokens.weight"):
            out[name] = 0.02 * gain * r
        elif name.endswith("embed_positions.weight") or name.endswith("bias"):
            out[name] = 0.02 * r
        else:
            fan_in = math.prod(shape[1:])
            out[name] = r * math.sqrt(gain / fan_in)
    return out


def qwen2_config_fields(**kw) -> Dict:
    """The config.json fields of Qwen2.5-3B-Instruct (public model card) that ``f5e_tts_amd.infer.qwen2.Qwen2Config.from_dict``
    takes; ``kw`` overrides (fewer layers for quick runs)."""
    f = dict(model_type="qwen2", vocab_size=151936, hidden_size=2048, num_hidden_layers=36, num_attention_heads=16,
             num_key_value_heads=2, intermediate_size=11008, rms_norm_eps=1e-6, rope_theta=1000000.0, max_position_embeddings=32768,
             tie_word_embeddings=True)
    f.update(kw)
    return f


def init_qwen2_state(fields: Dict, seed: int = 77, device="cpu", dtype=torch.bfloat16) -> State:
    """Seeded weights under ``Qwen2ForCausalLM``'s names for ``fields`` (``qwen2_config_fields``): matrices N(0, 1 / fan_in),
    biases N(0, 0.02), norm weights 1 + N(0, 0.1), token embedding N(0, 0.02); matrices in ``dtype``, the rest fp32.  ``device``:
    where the draws are made (3e9 parameters at full size; a GPU stream of draws differs from the CPU's)."""
    g = torch.Generator(device=device).manual_seed(seed)
    D, I, V = fields["hidden_size"], fields["intermediate_size"], fields["vocab_size"]
    H, Hkv = fields["num_attention_heads"], fields["num_key_value_heads"]
    dk = fields.get("head_dim") or D // H

    def mat(n, k, std=None):
        return (torch.randn(n, k, generator=g, device=device) * (std if std is not None else k ** -0.5)).to(dtype)

    def vec(n, mean, std):
        return mean + std * torch.randn(n, generator=g, device=device)
    sd = {"model.embed_tokens.weight": mat(V, D, 0.02), "model.norm.weight": vec(D, 1.0, 0.1)}
    if not fields.get("tie_word_embeddings"):
        sd["lm_head.weight"] = mat(V, D)
    for i in range(fields["num_hidden_layers"]):
        p = f"model.layers.{i}."
        for n, h in (("q", H), ("k", Hkv), ("v", Hkv)):
            sd[p + f"self_attn.{n}_proj.weight"], sd[p + f"self_attn.{n}_proj.bias"] = mat(h * dk, D), vec(h * dk, 0.0, 0.02)
        sd[p + "self_attn.o_proj.weight"] = mat(D, H * dk)
        sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"], sd[p + "mlp.down_proj.weight"] = mat(I, D), mat(I, D), mat(D, I)
        sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = vec(D, 1.0, 0.1), vec(D, 1.0, 0.1)
    return sd
