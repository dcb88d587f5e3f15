"""Paraformer on the device: funasr's ``paraformer-zh`` (speech_paraformer-large_asr_nat-zh-cn-16k-common-vocab8404), the
recogniser of the reference's Chinese WER (eval/utils_eval.py:472-482 ``load_asr_model("zh")``, ``asr_model.generate``).

Non-autoregressive: kaldi fbank -> LFR + CMVN -> SANM encoder (attention + FSMN memory) -> CIF predictor (frame-rate states to
token-rate embeddings) -> a decoder that emits every token in one pass -> argmax.  The holder's ``state_dict`` carries
funasr's parameter names; the arithmetic is restated from the public package and has not been run against funasr or a real
checkpoint (DESIGN 4r lists it with every deviation).  fp32, ragged batches, no CPU path.

Launch sequence: ``f5e_kaldi_fbank`` (Hamming window), ``f5e_lfr_cmvn_f32``; per encoder layer LayerNorm, q|k|v GEMM,
``f5e_mha_f32``, out-projection (+ residual), ``f5e_fsmn_f32`` on the v third (+ that sum), LayerNorm, FF1 + ReLU, FF2 +
residual; the predictor is ``f5e_im2col`` + 2 GEMMs + ``f5e_cif_alpha_f32`` + ``f5e_cif_fire_f32``; the decoder layers are
LayerNorms, GEMMs, ``f5e_fsmn_f32`` and ``f5e_mha_f32`` against the encoder output; ``f5e_nar_pick`` ends it.  The front-end,
encoder and predictor synchronise with nothing and allocate nothing once their scratch is planned (``xfmr_f32.plan``);
``generate`` reads the token counts back ONCE to size the decoder pass, as funasr does."""
from __future__ import annotations

import json
import math
import os
import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from .. import _C, ops
from .. import xfmr_f32 as X

Tensor = torch.Tensor
F32, I32 = torch.float32, torch.int32
SAMPLE_RATE = 16000
LN_EPS = 1e-12             # every LayerNorm of the model
MAX_LFR_FRAMES = 2000      # the cap on T' (120 s of audio at 60 ms per row); beyond it: refused, VAD segmentation is out of scope


@dataclass
class ParaformerConfig:
    """Defaults: speech_paraformer-large_asr_nat-zh-cn-16k-common-vocab8404."""
    n_mels: int = 80
    frame_length: int = 25     # ms
    frame_shift: int = 10      # ms
    lfr_m: int = 7
    lfr_n: int = 6
    d_model: int = 512
    heads: int = 4
    ff: int = 2048
    enc_layers: int = 50       # num_blocks: encoders0 (1 layer, lfr_m * n_mels -> d_model) + encoders
    kernel: int = 11
    sanm_shfit: int = 0        # funasr's spelling
    dec_layers: int = 16
    dec_heads: int = 4
    dec_ff: int = 2048
    dec_kernel: int = 11
    dec_sanm_shfit: int = 0
    vocab: int = 8404
    sos: int = 1
    eos: int = 2
    blank: int = 0
    threshold: float = 1.0
    smooth_factor: float = 1.0
    noise_threshold: float = 0.0
    tail_threshold: float = 0.45
    l_order: int = 1
    r_order: int = 1

    @property
    def in_width(self) -> int:
        return self.lfr_m * self.n_mels

    @classmethod
    def from_yaml_dict(cls, y: dict, vocab: Optional[int] = None) -> "ParaformerConfig":
        """funasr's config.yaml (parsed) -> the record; everything out of scope is refused by name."""
        model = y.get("model", "Paraformer")
        if model != "Paraformer":
            raise _C.F5EError(f"Paraformer: model: {model} is not supported (only `Paraformer`; SeACo / hotword models are out of scope)")
        e, d, p, f = (y.get(k) or {} for k in ("encoder_conf", "decoder_conf", "predictor_conf", "frontend_conf"))
        mc = y.get("model_conf") or {}
        for name, want in (("encoder", "SANMEncoder"), ("decoder", "ParaformerSANMDecoder"), ("predictor", "CifPredictorV2"),
                           ("frontend", "WavFrontend")):
            if y.get(name, want) != want:
                raise _C.F5EError(f"Paraformer: {name}: {y[name]} is not supported (only {want})")
        sa = e.get("selfattention_layer_type", "sanm")
        if sa != "sanm":
            raise _C.F5EError(f"Paraformer: selfattention_layer_type: {sa} is not supported (only sanm)")
        if e.get("input_layer", "pe") != "pe":
            raise _C.F5EError(f"Paraformer: input_layer: {e['input_layer']} is not supported (only pe)")
        if float(mc.get("ctc_weight", 0.0)) > 0.0:
            raise _C.F5EError(f"Paraformer: ctc_weight {mc['ctc_weight']} > 0 (CTC decoding of the encoder) is not supported")
        att = int(d.get("att_layer_num", d.get("num_blocks", 16)))
        if int(d.get("num_blocks", att)) != att:
            raise _C.F5EError(f"Paraformer: decoders2 ({int(d['num_blocks']) - att} layers: num_blocks {d['num_blocks']} above "
                              f"att_layer_num {att}) is not supported")
        if int(f.get("fs", SAMPLE_RATE)) != SAMPLE_RATE or f.get("window", "hamming") != "hamming":
            raise _C.F5EError("Paraformer: the front-end is built for fs 16000 and a hamming window")
        c = cls()
        got = dict(n_mels=f.get("n_mels"), frame_length=f.get("frame_length"), frame_shift=f.get("frame_shift"),
                   lfr_m=f.get("lfr_m"), lfr_n=f.get("lfr_n"), d_model=e.get("output_size"), heads=e.get("attention_heads"),
                   ff=e.get("linear_units"), enc_layers=e.get("num_blocks"), kernel=e.get("kernel_size"),
                   sanm_shfit=e.get("sanm_shfit"), dec_layers=att if d else None, dec_heads=d.get("attention_heads"),
                   dec_ff=d.get("linear_units"), dec_kernel=d.get("kernel_size"), dec_sanm_shfit=d.get("sanm_shfit"),
                   vocab=vocab if vocab is not None else y.get("vocab_size"), sos=mc.get("sos"), eos=mc.get("eos"),
                   threshold=p.get("threshold"), smooth_factor=p.get("smooth_factor"), noise_threshold=p.get("noise_threshold"),
                   tail_threshold=p.get("tail_threshold"), l_order=p.get("l_order"), r_order=p.get("r_order"))
        for k, v in got.items():
            if v is not None:
                setattr(c, k, type(getattr(c, k))(v))
        return c


def param_shapes(cfg: ParaformerConfig) -> Dict[str, tuple]:
    """funasr's parameter names -> shapes: exactly the keys a checkpoint must hold."""
    D, W, FF, K, V = cfg.d_model, cfg.in_width, cfg.ff, cfg.kernel, cfg.vocab
    s: Dict[str, tuple] = {}

    def lin(name, o, i, bias=True):
        s[name + ".weight"] = (o, i)
        if bias:
            s[name + ".bias"] = (o,)

    def ln(name, d):
        s[name + ".weight"], s[name + ".bias"] = (d,), (d,)

    def enc(prefix, din):
        lin(prefix + "self_attn.linear_q_k_v", 3 * D, din)
        lin(prefix + "self_attn.linear_out", D, D)
        s[prefix + "self_attn.fsmn_block.weight"] = (D, 1, K)
        lin(prefix + "feed_forward.w_1", FF, D)
        lin(prefix + "feed_forward.w_2", D, FF)
        ln(prefix + "norm1", din)
        ln(prefix + "norm2", D)

    def dec_ff(prefix):
        lin(prefix + "feed_forward.w_1", cfg.dec_ff, D)
        lin(prefix + "feed_forward.w_2", D, cfg.dec_ff, bias=False)
        ln(prefix + "feed_forward.norm", cfg.dec_ff)
        ln(prefix + "norm1", D)

    enc("encoder.encoders0.0.", W)
    for i in range(cfg.enc_layers - 1):
        enc(f"encoder.encoders.{i}.", D)
    ln("encoder.after_norm", D)
    s["predictor.cif_conv1d.weight"], s["predictor.cif_conv1d.bias"] = (D, D, cfg.l_order + cfg.r_order + 1), (D,)
    lin("predictor.cif_output", 1, D)
    for i in range(cfg.dec_layers):
        p = f"decoder.decoders.{i}."
        s[p + "self_attn.fsmn_block.weight"] = (D, 1, cfg.dec_kernel)
        lin(p + "src_attn.linear_q", D, D)
        lin(p + "src_attn.linear_k_v", 2 * D, D)
        lin(p + "src_attn.linear_out", D, D)
        dec_ff(p)
        ln(p + "norm2", D)
        ln(p + "norm3", D)
    dec_ff("decoder.decoders3.0.")
    ln("decoder.after_norm", D)
    lin("decoder.output_layer", V, D)
    s["decoder.embed.0.weight"] = (V, D)     # loaded and unused: inference embeds nothing
    return s


def seeded_state_dict(cfg: ParaformerConfig, seed: int) -> Dict[str, Tensor]:
    """Seeded weights of the checkpoint's shapes for tests and timing: matrices ~ U(-1, 1) / sqrt(fan_in), non-trivial biases and
    LayerNorm gains, FSMN taps ~ 1 / K."""
    g = torch.Generator().manual_seed(int(seed))
    out = {}
    for name, shape in param_shapes(cfg).items():
        u = torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1
        if "norm" in name and name.endswith(".weight"):
            t = 1.0 + 0.2 * u
        elif name.endswith(".bias"):
            t = 0.1 * u
        else:
            t = u / math.sqrt(max(1, math.prod(shape[1:])))
        out[name] = t.to(F32)
    return out


def parse_am_mvn(text: str) -> Tuple[Tensor, Tensor]:
    """The ``<AddShift>`` and ``<Rescale>`` vectors of a kaldi nnet text file (am.mvn) -> (shift, scale) in float64."""
    vecs = []
    for tag in ("<AddShift>", "<Rescale>"):
        m = re.search(re.escape(tag) + r"[^\[]*\[([^\]]*)\]", text)
        if m is None:
            raise _C.F5EError(f"am.mvn: no {tag} vector")
        vecs.append(torch.tensor([float(v) for v in m.group(1).split()], dtype=torch.float64))
    if vecs[0].numel() == 0 or vecs[0].shape != vecs[1].shape:
        raise _C.F5EError(f"am.mvn: <AddShift> has {vecs[0].numel()} values, <Rescale> {vecs[1].numel()}")
    return vecs[0], vecs[1]


def position_table(rows: int, depth: int) -> Tensor:
    """SinusoidalPositionEncoder: positions 1 .. rows, cat(sin, cos) of p * exp(-i ln(1e4) / (depth / 2 - 1)); float64 [rows, depth]."""
    half = depth // 2
    inv_t = torch.exp(torch.arange(half, dtype=torch.float64) * (-math.log(1e4) / (half - 1)))
    ang = torch.arange(1, rows + 1, dtype=torch.float64)[:, None] * inv_t[None]
    return torch.cat((torch.sin(ang), torch.cos(ang)), 1)


def hamming_window(n: int) -> Tensor:
    return 0.54 - 0.46 * torch.cos(2 * math.pi * torch.arange(n, dtype=torch.float64) / (n - 1))


def _is_cjk(tok: str) -> bool:
    return len(tok) > 0 and all(0x2e80 <= ord(ch) <= 0x9fff or 0xf900 <= ord(ch) <= 0xfaff or 0x20000 <= ord(ch) <= 0x2fa1f
                                for ch in tok)


def join_tokens(tokens: Sequence[str]) -> str:
    """CJK tokens are joined with no separator, a token ending in ``@@`` is glued to the next one, and two neighbouring
    non-CJK words are separated by one space (none between a CJK token and a word)."""
    words, pend = [], ""
    for t in tokens:
        if t.endswith("@@"):
            pend += t[:-2]
            continue
        words.append(pend + t)
        pend = ""
    if pend:
        words.append(pend)
    out, prev_word = "", False
    for w in words:
        word = not _is_cjk(w)
        out += (" " if word and prev_word else "") + w
        prev_word = word
    return out


class _Node(nn.Module):
    pass


def _put(root: nn.Module, name: str, p: nn.Parameter) -> None:
    *path, leaf = name.split(".")
    for part in path:
        if part not in root._modules:
            root.add_module(part, _Node())
        root = root._modules[part]
    root.register_parameter(leaf, p)


class Paraformer(nn.Module):
    """The holder (parameters under funasr's names) and the device passes."""

    def __init__(self, config=None, cmvn: Optional[Tuple[Tensor, Tensor]] = None, tokens: Optional[List[str]] = None):
        super().__init__()
        if config is None:
            config = ParaformerConfig()
        self.cfg = cfg = config if isinstance(config, ParaformerConfig) else ParaformerConfig.from_yaml_dict(config)
        D = cfg.d_model
        if D % cfg.heads or D % cfg.dec_heads or D // cfg.heads not in (16, 32, 64, 128) or D // cfg.dec_heads not in (16, 32, 64, 128):
            raise _C.F5EError(f"Paraformer: head widths {D}/{cfg.heads}, {D}/{cfg.dec_heads} must be 16, 32, 64 or 128 (f5e_mha_f32)")
        if cfg.n_mels % 4 or D % 4 or cfg.ff % 4 or cfg.dec_ff % 4 or cfg.in_width < 4:
            raise _C.F5EError("Paraformer: n_mels, d_model and the feed-forward widths must be multiples of 4")
        if cfg.l_order != 1 or cfg.r_order != 1:
            raise _C.F5EError("Paraformer: the predictor is built for l_order = r_order = 1")
        self.win, self.hop = SAMPLE_RATE * cfg.frame_length // 1000, SAMPLE_RATE * cfg.frame_shift // 1000
        if (1 << (self.win - 1).bit_length()) != 512:
            raise _C.F5EError("Paraformer: f5e_kaldi_fbank is built for a 512-point padded window (25 ms at 16 kHz)")
        for name, shape in param_shapes(cfg).items():
            _put(self, name, nn.Parameter(torch.zeros(shape, dtype=F32), requires_grad=False))
        from ..ppg.ppg_model import _kaldi_mel_banks
        k = torch.arange(256, dtype=torch.float64)
        self.register_buffer("window", hamming_window(self.win).float(), persistent=False)
        self.register_buffer("twiddle", torch.stack((torch.cos(2 * math.pi * k / 512), -torch.sin(2 * math.pi * k / 512)), -1).float(),
                             persistent=False)
        self.register_buffer("fb", _kaldi_mel_banks(cfg.n_mels, 512, float(SAMPLE_RATE)), persistent=False)
        shift, scale = cmvn if cmvn is not None else (torch.zeros(cfg.in_width), torch.ones(cfg.in_width))
        if shift.numel() != cfg.in_width or scale.numel() != cfg.in_width:
            raise _C.F5EError(f"Paraformer: am.mvn holds {shift.numel()} values, lfr_m * n_mels = {cfg.in_width}")
        self.register_buffer("cmvn_shift", shift.to(F32).contiguous(), persistent=False)
        self.register_buffer("cmvn_scale", scale.to(F32).contiguous(), persistent=False)
        self.register_buffer("pos", position_table(1024, cfg.in_width).float(), persistent=False)
        self.tokens = tokens
        self._w = None

    # ---- loading -----------------------------------------------------------------------------------------------------------
    def load_funasr_state(self, sd: Dict[str, Tensor]) -> None:
        """Exactly funasr's names: an unknown or missing key is an error that names it."""
        want = param_shapes(self.cfg)
        d2 = sorted(k for k in sd if k.startswith("decoder.decoders2."))
        if d2:
            raise _C.F5EError(f"Paraformer: decoders2 is not supported (checkpoint key {d2[0]})")
        unknown = sorted(k for k in sd if k not in want)
        if unknown:
            raise _C.F5EError(f"Paraformer: unknown checkpoint key {unknown[0]}" + (f" (and {len(unknown) - 1} more)" if len(unknown) > 1 else ""))
        missing = sorted(k for k in want if k not in sd)
        if missing:
            raise _C.F5EError(f"Paraformer: checkpoint key {missing[0]} is missing" + (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))
        for k, shape in want.items():
            if tuple(sd[k].shape) != tuple(shape):
                raise _C.F5EError(f"Paraformer: {k} has shape {tuple(sd[k].shape)}, the configuration gives {tuple(shape)}")
        self.load_state_dict({k: v.to(F32) for k, v in sd.items()}, strict=True)
        self._w = None

    @classmethod
    def from_pretrained_dir(cls, path: str) -> "Paraformer":
        """A local funasr model directory: config.yaml, model.pt (a plain or {"state_dict": ...} pickle), am.mvn, tokens.json."""
        import yaml
        for f in ("config.yaml", "model.pt", "am.mvn", "tokens.json"):
            if not os.path.exists(os.path.join(path, f)):
                raise _C.F5EError(f"Paraformer.from_pretrained_dir: {os.path.join(path, f)} is missing")
        with open(os.path.join(path, "config.yaml"), encoding="utf-8") as fh:
            y = yaml.safe_load(fh)
        with open(os.path.join(path, "tokens.json"), encoding="utf-8") as fh:
            tokens = json.load(fh)
        with open(os.path.join(path, "am.mvn"), encoding="utf-8") as fh:
            cmvn = parse_am_mvn(fh.read())
        cfg = ParaformerConfig.from_yaml_dict(y, vocab=len(tokens))
        sd = torch.load(os.path.join(path, "model.pt"), map_location="cpu", weights_only=True)
        if isinstance(sd, dict) and "state_dict" in sd:
            sd = sd["state_dict"]
        model = cls(cfg, cmvn=cmvn, tokens=list(tokens))
        model.load_funasr_state(sd)
        return model.eval()

    def _apply(self, fn, *a, **k):
        self._w = None
        return super()._apply(fn, *a, **k)

    # ---- weights as the kernels take them ------------------------------------------------------------------------------------
    def _weights(self) -> dict:
        dev = self.window.device
        if dev.type != "cuda":
            raise _C.F5EError("Paraformer: the model must be on the GPU (.cuda()); there is no CPU path")
        if self._w is not None:
            return self._w
        sd = dict(self.named_parameters())

        def pair(name, bias=True):
            return (sd[name + ".weight"].detach().contiguous(), sd[name + ".bias"].detach().contiguous() if bias else None)

        def taps(name):
            return sd[name].detach()[:, 0, :].t().contiguous()      # [C, 1, K] -> [K, C]

        def enc(p):
            return dict(norm1=pair(p + "norm1"), qkv=pair(p + "self_attn.linear_q_k_v"), out=pair(p + "self_attn.linear_out"),
                        fsmn=taps(p + "self_attn.fsmn_block.weight"), norm2=pair(p + "norm2"), w1=pair(p + "feed_forward.w_1"),
                        w2=pair(p + "feed_forward.w_2"))

        def dff(p):
            return dict(norm1=pair(p + "norm1"), w1=pair(p + "feed_forward.w_1"), ffn=pair(p + "feed_forward.norm"),
                        w2=pair(p + "feed_forward.w_2", bias=False))

        cfg = self.cfg
        w = dict(enc=[enc("encoder.encoders0.0.")] + [enc(f"encoder.encoders.{i}.") for i in range(cfg.enc_layers - 1)],
                 enc_norm=pair("encoder.after_norm"), dec=[], dec3=dff("decoder.decoders3.0."), dec_norm=pair("decoder.after_norm"),
                 out=pair("decoder.output_layer"), cif_out=pair("predictor.cif_output"))
        cw = sd["predictor.cif_conv1d.weight"].detach()            # [oc, ic, tap] -> [oc, tap * D + ic], the im2col order
        w["cif_conv"] = (cw.permute(0, 2, 1).reshape(cw.shape[0], -1).contiguous(), sd["predictor.cif_conv1d.bias"].detach().contiguous())
        for i in range(cfg.dec_layers):
            p = f"decoder.decoders.{i}."
            w["dec"].append(dict(dff(p), fsmn=taps(p + "self_attn.fsmn_block.weight"), norm2=pair(p + "norm2"), norm3=pair(p + "norm3"),
                                 q=pair(p + "src_attn.linear_q"), kv=pair(p + "src_attn.linear_k_v"),
                                 xout=pair(p + "src_attn.linear_out")))
        self._w = w
        return w

    @staticmethod
    def _left(K: int, shift: int) -> int:
        left = (K - 1) // 2 + shift
        if not 0 <= left <= K - 1:
            raise _C.F5EError(f"Paraformer: kernel_size {K} with sanm_shfit {shift} leaves no right context")
        return left

    # ---- geometry and scratch ------------------------------------------------------------------------------------------------
    def frames_of(self, samples: int) -> Tuple[int, int]:
        """(fbank frames T, LFR rows T') of ``samples`` samples; refused when too short or beyond the cap."""
        if samples < self.win:
            raise _C.F5EError(f"Paraformer: {samples} samples are fewer than one {self.win}-sample window")
        T = 1 + (samples - self.win) // self.hop
        Tp = -(-T // self.cfg.lfr_n)
        if Tp > MAX_LFR_FRAMES:
            raise _C.F5EError(f"Paraformer: {samples / SAMPLE_RATE:.1f} s of audio give {Tp} LFR frames, above the cap of "
                              f"{MAX_LFR_FRAMES} ({MAX_LFR_FRAMES * self.cfg.lfr_n * self.cfg.frame_shift / 1000:.0f} s); long-audio "
                              f"segmentation is out of scope")
        return T, Tp

    def _plans(self, B: int, T: int, Tp: int, L: int) -> Dict[str, dict]:
        c = self.cfg
        D, W, M, R, Lc = c.d_model, c.in_width, B * Tp, B * max(L, 1), Tp + 1
        front = X.plan(dict(fbank=(B, T, c.n_mels), feats=(B, Tp, W), frames=(B,)))
        enc = X.plan(dict(x=(M, D), xn=(M, max(W, D)), qkv=(M, 3 * D), ao=(M, D), ff=(M, c.ff), enc=(B, Tp, D)))
        pred = X.plan(dict(col=(B, Tp, 3 * D), hid=(M, D), logit=(B, Tp), alpha=(B, Lc), n=(B,), count=(B,),
                           cif=(ops.cif_fire_scratch(B, Tp, Lc),), embeds=(B, Lc, D)))
        dec = X.plan(dict(x=(R, D), xn=(R, D), t=(R, D), q=(R, D), ao=(R, D), ff=(R, c.dec_ff), kv=(M, 2 * D), logits=(R, c.vocab),
                          arg=(R,), logp=(R,), ids=(R,), length=(B,), score=(B,)))
        return dict(front=front, enc=enc, pred=pred, dec=dec)

    def workspace_bytes(self, B: int, samples: int, L: Optional[int] = None) -> int:
        """Bytes of scratch of ``generate`` / ``encode_predict`` on [B, samples] audio; ``L``: the longest token row the decoder
        pass is sized for (None: the most the predictor can emit, T' + 1)."""
        T, Tp = self.frames_of(samples)
        p = self._plans(B, T, Tp, Tp + 1 if L is None else L)
        return 4 * sum(v["_total"][0] for v in p.values())

    def _stage(self, ws: Optional[Tensor], plan_: dict, dev, who: str) -> Tensor:
        return X.take(ws, plan_["_total"][0], dev, f"Paraformer.{who}")

    def _pos(self, Tp: int) -> Tensor:
        if self.pos.shape[0] < Tp:
            self.pos = position_table(Tp, self.cfg.in_width).float().to(self.pos.device)
        return self.pos

    # ---- passes ----------------------------------------------------------------------------------------------------------------
    def _check_wav(self, wav: Tensor, lens: Optional[Tensor]):
        if wav.ndim != 2 or wav.dtype != F32 or not wav.is_cuda or not wav.is_contiguous():
            raise _C.F5EError("Paraformer: wav must be a contiguous f32 GPU tensor [B, samples] at 16 kHz in [-1, 1]; there is no CPU path")
        if lens is not None and (lens.dtype != I32 or not lens.is_cuda or lens.shape != (wav.shape[0],)):
            raise _C.F5EError(f"Paraformer: lens must be an i32 GPU tensor [{wav.shape[0]}]")

    def _frontend(self, wav: Tensor, lens: Optional[Tensor], ws: Tensor, pl: dict, T: int, Tp: int):
        c = self.cfg
        fbank, feats, frames = X.view(ws, pl, "fbank"), X.view(ws, pl, "feats"), X.view(ws, pl, "frames").view(I32)
        ops.kaldi_fbank(wav, self.window, self.twiddle, self.fb, fbank, self.win, self.hop)
        ops.lfr_cmvn(fbank, lens, self.cmvn_shift, self.cmvn_scale, self._pos(Tp), feats, frames, c.lfr_m, c.lfr_n,
                     xscale=math.sqrt(c.d_model), win=self.win, hop=self.hop)
        return feats, frames

    @torch.no_grad()
    def frontend(self, wav: Tensor, lens: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """wav f32 [B, samples] (16 kHz, [-1, 1]), lens i32 [B] samples per row -> (feats f32 [B, T', lfr_m n_mels], frames i32 [B]).
        ``feats`` is the ENCODER'S INPUT: fbank, LFR, CMVN, times sqrt(d_model), plus the position encoding (one kernel writes all
        of it); rows at or beyond frames[b] are zero."""
        self._check_wav(wav, lens)
        T, Tp = self.frames_of(wav.shape[1])
        pl = self._plans(wav.shape[0], T, Tp, 1)["front"]
        return self._frontend(wav, lens, self._stage(workspace, pl, wav.device, "frontend"), pl, T, Tp)

    def _enc_layer(self, w: dict, src: Tensor, dst: Tensor, xn: Tensor, qkv: Tensor, ao: Tensor, ff: Tensor, frames: Tensor, B: int):
        c = self.cfg
        D, M, din = c.d_model, src.shape[0], src.shape[1]
        h = ops.layernorm(src, xn[:M * din].view(M, din), *w["norm1"], eps=LN_EPS)
        ops.gemm_f32(h, *w["qkv"], out=qkv)
        ops.mha_f32(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], c.heads, (D // c.heads) ** -0.5, B=B, kv_len=frames, out=ao)
        ops.gemm_f32(ao, *w["out"], out=dst, addend=src if din == D else None)
        ops.fsmn(qkv[:, 2 * D:], w["fsmn"], frames, dst, B, self._left(c.kernel, c.sanm_shfit), addend=dst)
        h = ops.layernorm(dst, xn[:M * D].view(M, D), *w["norm2"], eps=LN_EPS)
        ops.gemm_f32(h, *w["w1"], out=ff, act=_C.ACT_RELU)
        ops.gemm_f32(ff, *w["w2"], out=dst, addend=dst)

    def _encode(self, feats: Tensor, frames: Tensor, ws: Tensor, pl: dict) -> Tensor:
        w = self._weights()
        B, Tp, W = feats.shape
        x, qkv, ao, ff, enc = (X.view(ws, pl, k) for k in ("x", "qkv", "ao", "ff", "enc"))
        xn = X.view(ws, pl, "xn").view(-1)
        src = feats.view(B * Tp, W)
        for lw in w["enc"]:
            self._enc_layer(lw, src, x, xn, qkv, ao, ff, frames, B)
            src = x
        e2 = enc.view(B * Tp, -1)
        ops.layernorm(x, e2, *w["enc_norm"], eps=LN_EPS)
        ops.mask_rows(e2, frames, B)
        return enc

    def _check_btc(self, t: Tensor, width: int, name: str):
        if t.ndim != 3 or t.dtype != F32 or not t.is_cuda or not t.is_contiguous() or t.shape[2] != width or min(t.shape) < 1:
            raise _C.F5EError(f"Paraformer: {name} must be a contiguous f32 GPU tensor [B, T, {width}]; there is no CPU path")

    def _check_len(self, t: Tensor, B: int, name: str):
        if t.dtype != I32 or not t.is_cuda or t.shape != (B,):
            raise _C.F5EError(f"Paraformer: {name} must be an i32 GPU tensor [{B}]")

    @torch.no_grad()
    def encode(self, feats: Tensor, frames: Tensor, workspace: Optional[Tensor] = None) -> Tensor:
        """``frontend``'s pair -> the encoder output f32 [B, T', d_model] (after_norm applied; rows at or beyond frames[b] zero)."""
        self._check_btc(feats, self.cfg.in_width, "feats")
        self._check_len(frames, feats.shape[0], "frames")
        pl = self._plans(feats.shape[0], 1, feats.shape[1], 1)["enc"]
        return self._encode(feats, frames, self._stage(workspace, pl, feats.device, "encode"), pl)

    def _predict(self, enc: Tensor, frames: Tensor, ws: Tensor, pl: dict):
        c, w = self.cfg, self._weights()
        B, Tp, D = enc.shape
        col, hid, logit, alpha, cif, embeds = (X.view(ws, pl, k) for k in ("col", "hid", "logit", "alpha", "cif", "embeds"))
        n, count = X.view(ws, pl, "n").view(I32), X.view(ws, pl, "count").view(I32)
        ops.im2col(enc, col, 3, 1)
        ops.gemm_f32(col.view(B * Tp, 3 * D), *w["cif_conv"], out=hid, act=_C.ACT_RELU)
        ops.gemm_f32(hid, *w["cif_out"], out=logit.view(B * Tp, 1))
        ops.cif_alpha(logit, frames, alpha, n, c.smooth_factor, c.noise_threshold, c.tail_threshold)
        ops.cif_fire(alpha, enc.view(B * Tp, D), frames, embeds, count, cif, n_limit=n, threshold=c.threshold)
        return embeds, n, alpha

    @torch.no_grad()
    def predict(self, enc: Tensor, frames: Tensor, workspace: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
        """The CIF predictor: enc f32 [B, T', D] (zero at and beyond frames[b]) -> (embeds f32 [B, T' + 1, D], n i32 [B], alphas f32
        [B, T' + 1]): row b holds its n[b] = floor(sum alpha) token embeddings, zero beyond; index frames[b] of alphas is the tail."""
        self._check_btc(enc, self.cfg.d_model, "enc")
        self._check_len(frames, enc.shape[0], "frames")
        pl = self._plans(enc.shape[0], 1, enc.shape[1], 1)["pred"]
        return self._predict(enc, frames, self._stage(workspace, pl, enc.device, "predict"), pl)

    def _dec_ff(self, w: dict, x: Tensor, xn: Tensor, ff: Tensor, t: Tensor) -> Tensor:
        h = ops.layernorm(x, xn, *w["norm1"], eps=LN_EPS)
        ops.gemm_f32(h, *w["w1"], out=ff, act=_C.ACT_RELU)
        ops.layernorm(ff, ff, *w["ffn"], eps=LN_EPS)
        return ops.gemm_f32(ff, w["w2"][0], None, out=t)

    def _decode(self, enc: Tensor, frames: Tensor, n: Tensor, L: int, ws: Tensor, pl: dict) -> Tensor:
        """Logits f32 [B * L, V] of the token embeddings already in the plan's ``x``."""
        c, w = self.cfg, self._weights()
        B, Tp, D = enc.shape
        R = B * L
        x, xn, t, q, ao = (X.view(ws, pl, k)[:R] for k in ("x", "xn", "t", "q", "ao"))
        ff, logits, kv = X.view(ws, pl, "ff")[:R], X.view(ws, pl, "logits")[:R], X.view(ws, pl, "kv")
        mem = enc.view(B * Tp, D)
        left = self._left(c.dec_kernel, c.dec_sanm_shfit)
        for lw in w["dec"]:
            self._dec_ff(lw, x, xn, ff, t)
            h = ops.layernorm(t, xn, *lw["norm2"], eps=LN_EPS)
            ops.fsmn(h, lw["fsmn"], n, x, B, left, addend=x)
            h = ops.layernorm(x, xn, *lw["norm3"], eps=LN_EPS)
            ops.gemm_f32(h, *lw["q"], out=q)
            ops.gemm_f32(mem, *lw["kv"], out=kv)
            ops.mha_f32(q, kv[:, :D], kv[:, D:], c.dec_heads, (D // c.dec_heads) ** -0.5, B=B, kv_len=frames, out=ao)
            ops.gemm_f32(ao, *lw["xout"], out=x, addend=x)
        self._dec_ff(w["dec3"], x, xn, ff, t)
        h = ops.layernorm(t, xn, *w["dec_norm"], eps=LN_EPS)
        return ops.gemm_f32(h, *w["out"], out=logits)

    def _dec_plan(self, B: int, Tp: int, L: int) -> dict:
        return self._plans(B, 1, Tp, L)["dec"]

    @torch.no_grad()
    def decode(self, enc: Tensor, frames: Tensor, embeds: Tensor, n: Tensor, workspace: Optional[Tensor] = None) -> Tensor:
        """enc [B, T', D], frames i32 [B], embeds f32 [B, L, D] (any L >= 1 rows of ``predict``'s), n i32 [B] -> log-probabilities f32
        [B, L, V] of every token in one pass (rows at or beyond n[b] are computed from zero embeddings and mean nothing)."""
        self._check_btc(enc, self.cfg.d_model, "enc")
        B, L = enc.shape[0], embeds.shape[1] if embeds.ndim == 3 else 0
        if embeds.ndim != 3 or embeds.shape[0] != B or embeds.shape[2] != self.cfg.d_model or L < 1 or embeds.dtype != F32 or \
                not embeds.is_cuda:
            raise _C.F5EError(f"Paraformer.decode: embeds must be an f32 GPU tensor [{B}, L >= 1, {self.cfg.d_model}]")
        self._check_len(frames, B, "frames")
        self._check_len(n, B, "n")
        pl = self._dec_plan(B, enc.shape[1], L)
        ws = self._stage(workspace, pl, enc.device, "decode")
        X.view(ws, pl, "x")[:B * L].view(B, L, -1).copy_(embeds)
        logits = self._decode(enc, frames, n, L, ws, pl)
        return ops.log_softmax_rows(logits, logits).view(B, L, -1)

    @torch.no_grad()
    def encode_predict(self, wav: Tensor, lens: Optional[Tensor] = None, workspace: Optional[Tensor] = None):
        """Front-end, encoder and predictor on one scratch: -> (feats, frames, enc, embeds, n, alphas), all views of it.  With a
        caller's ``workspace`` (``workspace_bytes``) nothing is allocated and nothing synchronises: capturable as a graph (run
        it once eagerly first, which folds the weights)."""
        self._check_wav(wav, lens)
        B = wav.shape[0]
        T, Tp = self.frames_of(wav.shape[1])
        p = self._plans(B, T, Tp, 1)
        tot = [p[k]["_total"][0] for k in ("front", "enc", "pred")]
        ws = X.take(workspace, sum(tot), wav.device, "Paraformer.encode_predict")
        feats, frames = self._frontend(wav, lens, ws, p["front"], T, Tp)
        enc = self._encode(feats, frames, ws[tot[0]:], p["enc"])
        embeds, n, alpha = self._predict(enc, frames, ws[tot[0] + tot[1]:], p["pred"])
        return feats, frames, enc, embeds, n, alpha

    @torch.no_grad()
    def generate(self, wav: Tensor, lens: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
        """wav f32 [B, samples], lens i32 [B] -> (tokens i32 [B, L] = the picked ids without sos / eos / blank, padded with -1;
        n i32 [B] their count; score f32 [B] = the sum of the picked log-probabilities over the predictor's tokens).  ONE read-back:
        the predictor's token counts, which size the decoder pass."""
        self._check_wav(wav, lens)
        c, B = self.cfg, wav.shape[0]
        T, Tp = self.frames_of(wav.shape[1])
        p = self._plans(B, T, Tp, Tp + 1)
        tot = [p[k]["_total"][0] for k in ("front", "enc", "pred", "dec")]
        ws = X.take(workspace, sum(tot), wav.device, "Paraformer.generate")
        _, frames, enc, embeds, n, _ = self.encode_predict(wav, lens, ws)
        L = int(n.cpu().max())
        if L < 1:
            return (torch.full((B, 0), -1, dtype=I32, device=wav.device), torch.zeros(B, dtype=I32, device=wav.device),
                    torch.zeros(B, dtype=F32, device=wav.device))
        pl, wd = self._dec_plan(B, Tp, L), ws[tot[0] + tot[1] + tot[2]:]
        X.view(wd, pl, "x")[:B * L].view(B, L, -1).copy_(embeds[:, :L])
        logits = self._decode(enc, frames, n, L, wd, pl)
        arg, ids, length = (X.view(wd, pl, k).view(I32) for k in ("arg", "ids", "length"))
        ops.nar_pick(logits, n, B, arg, X.view(wd, pl, "logp"), ids.view(B, L), length, X.view(wd, pl, "score"),
                     sos=c.sos, eos=c.eos, blank=c.blank, pad=-1)
        return ids.view(B, L).clone(), length.clone(), X.view(wd, pl, "score").clone()

    def decode_ids(self, ids: Sequence[int]) -> str:
        """Token ids (``generate``'s row, the -1 padding dropped) -> text by ``join_tokens``; needs tokens.json."""
        if self.tokens is None:
            raise _C.F5EError("Paraformer.decode_ids: the model was built without tokens.json")
        return join_tokens([self.tokens[i] for i in (int(v) for v in ids) if i >= 0])


class ParaformerRecognizer:
    """The duck type ``eval_wer.run_asr_wer`` takes: ``transcribe(wav_or_path, sr) -> str`` (as ``WhisperRecognizer``)."""

    def __init__(self, path: str, device="cuda"):
        self.device = torch.device(device)
        self.model = Paraformer.from_pretrained_dir(path).to(self.device)

    def _audio(self, audio, sr: Optional[int]) -> Tensor:
        from ..infer import audio as A
        from ..infer.utils_infer import load_wav
        if isinstance(audio, str):
            audio, sr = load_wav(audio)
        if sr is None:
            raise _C.F5EError("ParaformerRecognizer.transcribe: a tensor needs its sample rate")
        audio = torch.as_tensor(audio, dtype=F32)
        if audio.ndim == 1:
            audio = audio.unsqueeze(0)
        if audio.shape[0] > 1:
            audio = audio.mean(0, keepdim=True)
        return A.resample_device(audio.to(self.device, F32), int(sr), SAMPLE_RATE).contiguous()

    @torch.no_grad()
    def transcribe(self, audio, sr: Optional[int] = None, mode=None, **ignored) -> str:
        """One recording, or a list of them (-> a list of texts, one pass each)."""
        if isinstance(audio, (list, tuple)):
            return [self.transcribe(a, sr) for a in audio]
        tokens, _, _ = self.model.generate(self._audio(audio, sr))
        return self.model.decode_ids(tokens[0].tolist())
