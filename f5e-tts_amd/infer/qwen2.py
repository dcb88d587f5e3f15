"""Qwen2 on the device: the chat model between Whisper and the sampler in voice chat.

``Qwen2`` is a decoder-only language model under ``transformers``' state-dict names (``Qwen2ForCausalLM``).  Its matrices stay
in 16 bits on the device and go through the fp32 GEMMs that widen them in registers (``ops.gemm_f32_w16`` for a prompt,
``ops.gemm_f32_w16_skinny`` for a decode step of at most 16 rows), so the arithmetic is the fp32 model's on the widened
weights; the reference computes in bf16.  Everything else is csrc/llm.hip: RMSNorm, SwiGLU, the token gather, grouped-query
attention with rotary positions (a prompt or a turn's new text behind the cache; one position read from the step record) and
the pick that applies ``transformers``' sampling processors.  A layer is 8 launches:

    RMSNorm, q|k|v GEMM + bias, attention, o_proj + residual, RMSNorm, gate|up GEMM, SwiGLU, down_proj + residual

``generate`` decodes R >= 1 left-padded rows; ``step_graph=True`` captures ONE decode step (a single chain of launches) as a
hipGraph and replays it per token from the device record, with the eager run's tokens.  ``ChatSession`` keeps the caches across
the turns of a conversation and prefills only a turn's new text.  ``Qwen2Tokenizer`` is byte-level BPE with Qwen2's
pre-tokeniser; ``apply_chat_template`` renders ChatML.
"""
from __future__ import annotations

import json
import math
import os
import unicodedata
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import _C, ops
from ..eval.whisper import bpe_merge, bytes_to_unicode, decode_pieces
from ..xfmr_f32 import plan as ws_plan, take as ws_take, view as ws_view

Tensor = torch.Tensor
F32, I32 = torch.float32, torch.int32
MAX_POSITIONS = ops.LLM_MAX_POS              # cached positions per row: the kernels' cap
HEAD_DIMS = (32, 64, 128)
MAX_GROUP = 8
WEIGHT_TYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}

QWEN2_PATTERN = (r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+")
CHATML_SPECIALS = ("<|endoftext|>", "<|im_start|>", "<|im_end|>")
# Qwen2.5-Instruct's default system line (its public chat template), used when the first message is not a system message
DEFAULT_SYSTEM = "You are Qwen, created by Alibaba Cloud. You are a helpful assistant."


# ---- configuration ------------------------------------------------------------------------------------------------------------
@dataclass
class Qwen2Config:
    vocab_size: int
    hidden_size: int
    num_hidden_layers: int
    num_attention_heads: int
    num_key_value_heads: int
    intermediate_size: int
    rms_norm_eps: float = 1e-6
    rope_theta: float = 1000000.0
    max_position_embeddings: int = 32768
    tie_word_embeddings: bool = False
    head_dim: Optional[int] = None

    def __post_init__(self):
        if self.head_dim is None:
            if self.hidden_size % self.num_attention_heads:
                raise _C.F5EError(f"Qwen2Config: hidden_size {self.hidden_size} is not a multiple of num_attention_heads "
                                  f"{self.num_attention_heads}")
            self.head_dim = self.hidden_size // self.num_attention_heads
        if self.head_dim not in HEAD_DIMS:
            raise _C.F5EError(f"Qwen2Config: head_dim = {self.head_dim} is not built ({HEAD_DIMS} are)")
        if self.num_key_value_heads < 1 or self.num_attention_heads % self.num_key_value_heads:
            raise _C.F5EError(f"Qwen2Config: num_key_value_heads = {self.num_key_value_heads} must divide num_attention_heads = "
                              f"{self.num_attention_heads}")
        if self.group > MAX_GROUP:
            raise _C.F5EError(f"Qwen2Config: {self.group} query heads per key/value head; the attention kernels take at most "
                              f"{MAX_GROUP}")
        if self.hidden_size % 4 or self.intermediate_size % 4 or self.hidden_size > 8192:
            raise _C.F5EError(f"Qwen2Config: hidden_size {self.hidden_size} / intermediate_size {self.intermediate_size} must be "
                              f"multiples of 4, hidden_size at most 8192")
        if not 2 <= self.vocab_size <= 262144:
            raise _C.F5EError(f"Qwen2Config: vocab_size = {self.vocab_size} must lie in 2 .. 262144")

    @property
    def group(self) -> int:
        return self.num_attention_heads // self.num_key_value_heads

    @classmethod
    def from_dict(cls, d: dict) -> "Qwen2Config":
        """A ``config.json`` as a dict.  Refused by name: another ``model_type``, ``rope_scaling`` (or a ``rope_parameters``
        type other than default), ``use_sliding_window``, a ``layer_types`` entry other than ``full_attention``."""
        mt = d.get("model_type", "qwen2")
        if mt != "qwen2":
            raise _C.F5EError(f"Qwen2Config: model_type = {mt!r} is not built (qwen2 is)")
        if d.get("rope_scaling"):
            raise _C.F5EError(f"Qwen2Config: rope_scaling = {d['rope_scaling']!r} is not built")
        rp = d.get("rope_parameters") or {}
        if rp.get("rope_type", "default") != "default":
            raise _C.F5EError(f"Qwen2Config: rope_scaling (rope_parameters.rope_type = {rp.get('rope_type')!r}) is not built")
        if d.get("use_sliding_window"):
            raise _C.F5EError("Qwen2Config: use_sliding_window = true is not built")
        for t in d.get("layer_types") or ():
            if t != "full_attention":
                raise _C.F5EError(f"Qwen2Config: layer_types entry {t!r} is not built (full_attention is)")
        theta = d.get("rope_theta", rp.get("rope_theta", 1000000.0))
        keys = ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size")
        missing = [k for k in keys if k not in d]
        if missing:
            raise _C.F5EError(f"Qwen2Config: config.json lacks {missing}")
        return cls(**{k: int(d[k]) for k in keys}, num_key_value_heads=int(d.get("num_key_value_heads", d["num_attention_heads"])),
                   rms_norm_eps=float(d.get("rms_norm_eps", 1e-6)), rope_theta=float(theta),
                   max_position_embeddings=int(d.get("max_position_embeddings", 32768)),
                   tie_word_embeddings=bool(d.get("tie_word_embeddings", False)), head_dim=d.get("head_dim"))

    @classmethod
    def from_json(cls, path: str) -> "Qwen2Config":
        with open(path) as f:
            return cls.from_dict(json.load(f))


@dataclass
class GenerationDefaults:
    """What ``generation_config.json`` supplies (``transformers``' own defaults where it is silent)."""
    do_sample: bool = False
    temperature: float = 1.0
    top_k: int = 50
    top_p: float = 1.0
    repetition_penalty: float = 1.0
    eos_token_id: Tuple[int, ...] = ()
    pad_token_id: Optional[int] = None

    @classmethod
    def from_dict(cls, d: dict) -> "GenerationDefaults":
        eos = d.get("eos_token_id")
        eos = () if eos is None else (int(eos),) if isinstance(eos, int) else tuple(int(e) for e in eos)
        g = cls(eos_token_id=eos, pad_token_id=d.get("pad_token_id"))
        for k in ("do_sample", "temperature", "top_k", "top_p", "repetition_penalty"):
            if d.get(k) is not None:
                setattr(g, k, type(getattr(g, k))(d[k]))
        return g


def rotary_table(head_dim: int, theta: float, positions: int) -> Tuple[Tensor, Tensor]:
    """cos, sin f32 [positions, head_dim / 2] on the host, as ``Qwen2RotaryEmbedding`` computes them in fp32 (the two halves of
    its tables are equal, so one is kept)."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).to(dtype=torch.float) / head_dim))
    freqs = torch.arange(positions, dtype=torch.int64).float()[:, None] * inv_freq.float()[None, :]
    return freqs.cos().contiguous(), freqs.sin().contiguous()


# ---- tokeniser and template -----------------------------------------------------------------------------------------------------
class Qwen2Tokenizer:
    """Byte-level BPE as ``Qwen2Tokenizer`` applies it: NFC, the special tokens split out of the text, Qwen2's pre-tokeniser
    pattern, GPT-2's byte alphabet and greedy merges by rank."""

    def __init__(self, vocab: Dict[str, int], merges: Sequence[Tuple[str, str]], specials: Dict[str, int],
                 non_special: Sequence[str] = ()):
        """``specials``: every added token (split out of the text before the pattern runs); ``non_special``: those of them that
        ``skip_special_tokens`` keeps (``"special": false`` entries such as Qwen2.5's tool-call markers)."""
        import regex
        self.vocab = dict(vocab)
        self.ranks = {tuple(m): i for i, m in enumerate(merges)}
        self.specials = dict(specials)
        self.id_to_piece = {i: s for s, i in self.vocab.items()}
        self.added = {i: s for s, i in self.specials.items()}
        self.skipped = {i for s, i in self.specials.items() if s not in set(non_special)}
        self.first_special = min(self.skipped) if self.skipped else len(self.vocab)
        self._b2u = bytes_to_unicode()
        self._pat = regex.compile(QWEN2_PATTERN)
        self._split = regex.compile("(" + "|".join(regex.escape(s) for s in sorted(self.specials, key=len, reverse=True)) + ")") \
            if self.specials else None
        self._cache: Dict[str, List[int]] = {}

    @classmethod
    def from_dir(cls, path: str) -> "Qwen2Tokenizer":
        """``vocab.json`` + ``merges.txt``, the special tokens from ``tokenizer_config.json`` (``added_tokens_decoder``) and /
        or ``added_tokens.json``."""
        with open(os.path.join(path, "vocab.json"), encoding="utf-8") as f:
            vocab = json.load(f)
        merges = []
        with open(os.path.join(path, "merges.txt"), encoding="utf-8") as f:
            for line in f:
                line = line.rstrip("\n")
                if not line or line.startswith("#version"):
                    continue
                a, b = line.split(" ")
                merges.append((a, b))
        specials: Dict[str, int] = {}
        plain = set()
        p = os.path.join(path, "added_tokens.json")
        if os.path.exists(p):
            with open(p, encoding="utf-8") as f:
                specials.update({s: int(i) for s, i in json.load(f).items()})
        p = os.path.join(path, "tokenizer_config.json")
        if os.path.exists(p):
            with open(p, encoding="utf-8") as f:
                for i, t in (json.load(f).get("added_tokens_decoder") or {}).items():
                    specials[t["content"]] = int(i)
                    if not t.get("special", True):
                        plain.add(t["content"])
        specials = {s: i for s, i in specials.items() if s not in vocab}
        return cls(vocab, merges, specials, sorted(plain))

    def _word(self, tok: str) -> List[int]:
        ids = self._cache.get(tok)
        if ids is None:
            sym = [self._b2u[b] for b in tok.encode("utf-8")]
            ids = self._cache[tok] = [self.vocab[s] for s in bpe_merge(sym, self.ranks)]
        return ids

    def encode(self, text: str) -> List[int]:
        text = unicodedata.normalize("NFC", text)
        parts = self._split.split(text) if self._split is not None else [text]
        out: List[int] = []
        for part in parts:
            if part in self.specials:
                out.append(self.specials[part])
            elif part:
                for tok in self._pat.findall(part):
                    out.extend(self._word(tok))
        return out

    def decode_ids(self, ids: Sequence[int], skip_special_tokens: bool = True) -> str:
        """Runs of ordinary ids through ``decode_pieces``; an added token is spelled as it is, unless it is special and skipped."""
        out, run = [], []
        for i in list(ids) + [None]:
            if i is not None and int(i) not in self.added:
                run.append(int(i))
                continue
            if run:
                out.append(decode_pieces(self.id_to_piece, 1 << 62, run))
                run = []
            if i is not None and not (skip_special_tokens and int(i) in self.skipped):
                out.append(self.added[int(i)])
        return "".join(out)


def apply_chat_template(messages: Sequence[dict], add_generation_prompt: bool = True, tools=None) -> str:
    """ChatML as Qwen2.5-Instruct's public template renders a conversation without tools:
    ``<|im_start|>{role}\\n{content}<|im_end|>\\n`` per message, Qwen2.5's default system line first when the first message is
    not a system message, ``<|im_start|>assistant\\n`` at the end."""
    if tools:
        raise _C.F5EError("apply_chat_template: tools are not built")
    out = []
    if not messages or messages[0].get("role") != "system":
        out.append(f"<|im_start|>system\n{DEFAULT_SYSTEM}<|im_end|>\n")
    for m in messages:
        if m.get("role") not in ("system", "user", "assistant") or not isinstance(m.get("content"), str):
            raise _C.F5EError(f"apply_chat_template: a message needs a role of system / user / assistant and a string content (got "
                              f"{m!r})")
        out.append(f"<|im_start|>{m['role']}\n{m['content']}<|im_end|>\n")
    if add_generation_prompt:
        out.append("<|im_start|>assistant\n")
    return "".join(out)


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _sampling(gen: GenerationDefaults, do_sample, temperature, top_k, top_p, repetition_penalty, vocab: int) -> SimpleNamespace:
    """The call's settings: None means the checkpoint's generation_config."""
    s = SimpleNamespace(do_sample=bool(gen.do_sample if do_sample is None else do_sample),
                        temperature=float(gen.temperature if temperature is None else temperature),
                        top_k=int(gen.top_k if top_k is None else top_k), top_p=float(gen.top_p if top_p is None else top_p),
                        penalty=float(gen.repetition_penalty if repetition_penalty is None else repetition_penalty))
    if not s.penalty >= 1.0 or not math.isfinite(s.penalty):
        raise _C.F5EError(f"Qwen2.generate: repetition_penalty = {s.penalty} must be finite and >= 1")
    if s.do_sample:
        if not (s.temperature > 0 and math.isfinite(s.temperature)) or not 0 < s.top_p <= 1:
            raise _C.F5EError(f"Qwen2.generate: need temperature > 0 and 0 < top_p <= 1 (got {s.temperature}, {s.top_p})")
        if s.top_k == 0:                     # transformers: no top-k filter; the pick keeps at most 64
            s.top_k = ops.LLM_MAX_TOP_K
        if not 1 <= s.top_k <= min(ops.LLM_MAX_TOP_K, vocab):
            raise _C.F5EError(f"Qwen2.generate: top_k = {s.top_k} must lie in 1 .. {min(ops.LLM_MAX_TOP_K, vocab)}")
    return s


class Qwen2:
    """``Qwen2ForCausalLM`` on the device.  ``weights``: the element type the matrices are kept in ("bf16", "fp16" or "f32";
    norms and biases are always fp32)."""

    def __init__(self, config: Qwen2Config, weights: str = "bf16", generation: Optional[GenerationDefaults] = None,
                 tokenizer: Optional[Qwen2Tokenizer] = None):
        if weights not in WEIGHT_TYPES:
            raise _C.F5EError(f"Qwen2: weights = {weights!r} must be one of {tuple(WEIGHT_TYPES)}")
        self.cfg, self.weights, self.wdtype = config, weights, WEIGHT_TYPES[weights]
        self.gen = generation or GenerationDefaults()
        self.tokenizer = tokenizer
        self.layers: List[SimpleNamespace] = []
        self.embed = self.norm = self.lm_head = None
        self.cos = self.sin = None
        self.device = None

    # -- loading
    def load_state_dict(self, sd: Dict[str, Tensor], device="cuda") -> "Qwen2":
        """A state dict under ``transformers``' names (``model.embed_tokens.weight``, ``model.layers.N...``, ``model.norm.weight``,
        ``lm_head.weight`` unless tied).  q | k | v and gate | up are stacked once here."""
        cfg, wd = self.cfg, self.wdtype
        H, Hkv, dk, D, I = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, cfg.hidden_size, cfg.intermediate_size

        def get(name, shape):
            if name not in sd:
                raise _C.F5EError(f"Qwen2: the state dict lacks {name}")
            t = sd[name]
            if tuple(t.shape) != tuple(shape):
                raise _C.F5EError(f"Qwen2: {name} is {tuple(t.shape)}, the configuration asks for {tuple(shape)}")
            return t

        mat = lambda t: t.to(device=device, dtype=wd).contiguous()          # noqa: E731
        vec = lambda t: t.to(device=device, dtype=F32).contiguous()         # noqa: E731
        self.embed = mat(get("model.embed_tokens.weight", (cfg.vocab_size, D)))
        self.layers = []
        for i in range(cfg.num_hidden_layers):
            p = f"model.layers.{i}."
            qkv_w = torch.cat([get(p + f"self_attn.{n}_proj.weight", (h * dk, D)) for n, h in (("q", H), ("k", Hkv), ("v", Hkv))], 0)
            qkv_b = torch.cat([get(p + f"self_attn.{n}_proj.bias", (h * dk,)) for n, h in (("q", H), ("k", Hkv), ("v", Hkv))], 0)
            gu = torch.cat([get(p + "mlp.gate_proj.weight", (I, D)), get(p + "mlp.up_proj.weight", (I, D))], 0)
            self.layers.append(SimpleNamespace(
                ln1=vec(get(p + "input_layernorm.weight", (D,))), wqkv=mat(qkv_w), bqkv=vec(qkv_b),
                wo=mat(get(p + "self_attn.o_proj.weight", (D, H * dk))), ln2=vec(get(p + "post_attention_layernorm.weight", (D,))),
                wgu=mat(gu), wdown=mat(get(p + "mlp.down_proj.weight", (D, I)))))
        self.norm = vec(get("model.norm.weight", (D,)))
        self.lm_head = self.embed if cfg.tie_word_embeddings else mat(get("lm_head.weight", (cfg.vocab_size, D)))
        cos, sin = rotary_table(dk, cfg.rope_theta, MAX_POSITIONS)
        self.cos, self.sin = cos.to(device), sin.to(device)
        self.device = torch.device(device)
        return self

    @classmethod
    def from_pretrained_dir(cls, path: str, weights: str = "auto", device="cuda") -> "Qwen2":
        """``config.json``, ``generation_config.json``, ``model.safetensors`` (or the shards of
        ``model.safetensors.index.json``) and, where present, the tokeniser's files.  ``weights="auto"``: the checkpoint's type."""
        from safetensors.torch import load_file
        cfg = Qwen2Config.from_json(os.path.join(path, "config.json"))
        gen = GenerationDefaults()
        gp = os.path.join(path, "generation_config.json")
        if os.path.exists(gp):
            with open(gp) as f:
                gen = GenerationDefaults.from_dict(json.load(f))
        index = os.path.join(path, "model.safetensors.index.json")
        if os.path.exists(index):
            with open(index) as f:
                shards = sorted(set(json.load(f)["weight_map"].values()))
        else:
            shards = ["model.safetensors"]
        sd: Dict[str, Tensor] = {}
        for s in shards:
            sd.update(load_file(os.path.join(path, s)))
        if weights == "auto":
            dt = sd["model.embed_tokens.weight"].dtype
            weights = {torch.bfloat16: "bf16", torch.float16: "fp16"}.get(dt, "f32")
        tok = Qwen2Tokenizer.from_dir(path) if os.path.exists(os.path.join(path, "vocab.json")) else None
        return cls(cfg, weights, gen, tok).load_state_dict(sd, device)

    def device_bytes(self) -> int:
        """Bytes of device memory the weights and the rotary tables take (a tied ``lm_head`` counted once)."""
        seen, total = set(), 0
        ts = [self.embed, self.norm, self.lm_head, self.cos, self.sin]
        for L in self.layers:
            ts += [L.ln1, L.wqkv, L.bqkv, L.wo, L.ln2, L.wgu, L.wdown]
        for t in ts:
            if t is not None and t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                total += t.numel() * t.element_size()
        return total

    # -- state
    def new_state(self, R: int, positions: int) -> SimpleNamespace:
        """The caches of R rows and ``positions`` positions, the token table, the step record and the decode step's scratch: all
        a decode step touches, so the step allocates nothing."""
        cfg, dev = self.cfg, self.device
        if self.embed is None:
            raise _C.F5EError("Qwen2: no weights are loaded")
        if not 2 <= positions <= MAX_POSITIONS:
            raise _C.F5EError(f"Qwen2: {positions} positions; the caches hold 2 .. {MAX_POSITIONS}")
        H, Hkv, dk, D, I, V = (cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, cfg.hidden_size, cfg.intermediate_size,
                               cfg.vocab_size)
        zi = lambda *s: torch.zeros(*s, dtype=I32, device=dev)   # noqa: E731
        S = SimpleNamespace(R=R, P=positions, tokens=zi(R, positions), last=zi(R), done=zi(R), alive=zi(1), begin=zi(R),
                            row_key=zi(R), serial=zi(R), rec=zi(ops.STEP_REC_WORDS), n=0, graph=None, graph_key=None,
                            stream=None, captures=0, replays=0)
        S.kc = [torch.zeros(R, positions, Hkv * dk, dtype=F32, device=dev) for _ in self.layers]
        S.vc = [torch.zeros(R, positions, Hkv * dk, dtype=F32, device=dev) for _ in self.layers]
        S.plan = ws_plan(dict(x=(R, D), xn=(R, D), qkv=(R, (H + 2 * Hkv) * dk), ao=(R, H * dk), gu=(R, 2 * I), ff=(R, I),
                              logits=(R, V)))
        S.ws = ws_take(None, S.plan["_total"][0], dev, "Qwen2")
        S.skinny = R <= ops.SKINNY_MAX_M
        if S.skinny:
            shapes = (((H + 2 * Hkv) * dk, D), (D, H * dk), (2 * I, D), (D, I), (V, D))
            need = max(ops._skinny_need(n, k, dev) for n, k in shapes)
            S.gemm_ws = torch.empty(max(need, 16) // 4, dtype=F32, device=dev)
        return S

    def _gemm(self, a, w, bias=None, *, out, addend=None):
        fn = ops.gemm_f32 if w.dtype == F32 else ops.gemm_f32_w16
        return fn(a, w, bias, out=out, addend=addend)

    def _gemm_step(self, S, a, w, bias=None, *, out, addend=None):
        if not S.skinny:
            return self._gemm(a, w, bias, out=out, addend=addend)
        fn = ops.gemm_f32_skinny if w.dtype == F32 else ops.gemm_f32_w16_skinny
        return fn(a, w, bias, out=out, addend=addend, workspace=S.gemm_ws)

    # -- a prompt, or a turn's new text, behind the cache
    @torch.no_grad()
    def append(self, S: SimpleNamespace, ids: Tensor, p0: int, hidden: Optional[list] = None) -> Tensor:
        """ids i32 [R, U] at positions p0 .. p0+U-1 of the state's rows (left padding through ``S.begin``) -> the logits of
        the last position, f32 [R, V].  ``hidden``: receives every layer's input and the last layer's output, [R, U, D] each."""
        cfg, dev = self.cfg, self.device
        R, U = ids.shape
        if R != S.R or U < 1 or p0 < 0 or p0 + U > S.P:
            raise _C.F5EError(f"Qwen2.append: {R} x {U} ids at position {p0} do not fit the state's {S.R} rows of {S.P} positions")
        H, Hkv, dk, D, I, V = (cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, cfg.hidden_size, cfg.intermediate_size,
                               cfg.vocab_size)
        M = R * U
        pl = ws_plan(dict(x=(M, D), xn=(M, D), qkv=(M, (H + 2 * Hkv) * dk), ao=(M, H * dk), gu=(M, 2 * I), ff=(M, I), xl=(R, D)))
        ws = ws_take(None, pl["_total"][0], dev, "Qwen2.append")
        x, xn, qkv, ao, gu, ff, xl = (ws_view(ws, pl, n) for n in ("x", "xn", "qkv", "ao", "gu", "ff", "xl"))
        ops.llm_embed(ids.to(device=dev, dtype=I32).reshape(-1).contiguous(), self.embed, x)
        scale = dk ** -0.5
        for i, L in enumerate(self.layers):
            if hidden is not None:
                hidden.append(x.view(R, U, D).clone())
            ops.rmsnorm_f32(x, L.ln1, cfg.rms_norm_eps, out=xn)
            self._gemm(xn, L.wqkv, L.bqkv, out=qkv)
            ops.gqa_rope_append_f32(qkv, S.kc[i], S.vc[i], self.cos, self.sin, U, p0, H, Hkv, scale, begin=S.begin, out=ao)
            self._gemm(ao, L.wo, None, out=x, addend=x)
            ops.rmsnorm_f32(x, L.ln2, cfg.rms_norm_eps, out=xn)
            self._gemm(xn, L.wgu, None, out=gu)
            ops.swiglu_f32(gu, out=ff)
            self._gemm(ff, L.wdown, None, out=x, addend=x)
        if hidden is not None:
            hidden.append(x.view(R, U, D).clone())
        ops.rmsnorm_f32(x[U - 1::U], self.norm, cfg.rms_norm_eps, out=xl)     # the last position of every row
        logits = torch.empty(R, V, dtype=F32, device=dev)
        self._gemm(xl, self.lm_head, None, out=logits)
        return logits

    def _pick(self, S: SimpleNamespace, logits: Tensor, sm: SimpleNamespace, eos, pad: int, keep=None) -> None:
        kw = {} if keep is None else dict(keep_id=keep[0], keep_p=keep[1], keep_n=keep[2])
        ops.llm_pick_dev(logits, S.tokens, S.last, S.done, S.alive, S.rec, eos=eos, pad=pad, do_sample=sm.do_sample,
                         penalty=sm.penalty, temperature=sm.temperature, top_k=sm.top_k if sm.do_sample else 1, top_p=sm.top_p,
                         begin=S.begin, row_key=S.row_key, serial=S.serial, **kw)

    def _step(self, S: SimpleNamespace, sm: SimpleNamespace, eos, pad: int) -> None:
        """The launches of ONE decode step at the record's position: the gather, 8 per layer, the final norm, lm_head and the
        pick's 2 (8 L + 5).  No allocation, no
        copy, no host read: this is what the graph captures."""
        cfg = self.cfg
        H, Hkv, dk = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        x, xn, qkv, ao, gu, ff, logits = (ws_view(S.ws, S.plan, n) for n in ("x", "xn", "qkv", "ao", "gu", "ff", "logits"))
        scale = dk ** -0.5
        ops.llm_embed(S.last, self.embed, x)
        for i, L in enumerate(self.layers):
            ops.rmsnorm_f32(x, L.ln1, cfg.rms_norm_eps, out=xn)
            self._gemm_step(S, xn, L.wqkv, L.bqkv, out=qkv)
            ops.gqa_rope_decode_dev_f32(qkv, S.kc[i], S.vc[i], self.cos, self.sin, S.rec, H, Hkv, scale, begin=S.begin, out=ao)
            self._gemm_step(S, ao, L.wo, None, out=x, addend=x)
            ops.rmsnorm_f32(x, L.ln2, cfg.rms_norm_eps, out=xn)
            self._gemm_step(S, xn, L.wgu, None, out=gu)
            ops.swiglu_f32(gu, out=ff)
            self._gemm_step(S, ff, L.wdown, None, out=x, addend=x)
        ops.rmsnorm_f32(x, self.norm, cfg.rms_norm_eps, out=xn)
        self._gemm_step(S, xn, self.lm_head, None, out=logits)
        self._pick(S, logits, sm, eos, pad)

    def _capture(self, S: SimpleNamespace, sm: SimpleNamespace, eos, pad: int) -> None:
        """Captures ``_step`` on the state's side stream: one stream, a linear chain.  Capturing executes nothing, so it needs
        no ordering against the caller's stream, where the graph is then launched."""
        if S.stream is None:
            S.stream = torch.cuda.Stream(device=self.device)
        if S.graph is not None:
            S.graph.retire()
        g = ops.Graph()
        with torch.cuda.stream(S.stream):
            g.begin()
            try:
                self._step(S, sm, eos, pad)
            finally:
                g.end()
        S.graph, S.captures = g, S.captures + 1
        ops.Graph.reap()

    @torch.no_grad()
    def decode(self, S: SimpleNamespace, logits: Tensor, max_new_tokens: int, sm: SimpleNamespace, eos, pad: int, seed: int = 0,
               step_graph: bool = False, sync_every: int = 8) -> int:
        """Picks from ``logits`` (the last position's, S.n tokens stand in the table) and decodes until every row is done or
        ``max_new_tokens`` are out.  -> the number of token columns written; S.n moves behind them, the caches hold all of
        them but the last."""
        n0 = S.n
        if max_new_tokens < 1 or n0 < 1 or n0 + max_new_tokens > S.P or sync_every < 1:
            raise _C.F5EError(f"Qwen2.generate: {n0} tokens and max_new_tokens = {max_new_tokens} exceed the {S.P} positions of "
                              f"the state (at most {MAX_POSITIONS}), or nothing is asked for")
        S.rec.copy_(ops.whisper_step_record(n0 - 1, n0, seed if sm.do_sample else 0))
        S.done.zero_()
        S.alive.fill_(S.R)
        self._pick(S, logits, sm, eos, pad)
        made = 1
        key = (sm.do_sample, sm.penalty, sm.temperature, sm.top_k, sm.top_p, tuple(eos), pad)
        if step_graph and (S.graph is None or S.graph_key != key):
            self._capture(S, sm, eos, pad)
            S.graph_key = key
        while made < max_new_tokens:
            if made % sync_every == 0 and int(S.alive.item()) == 0:
                break
            if step_graph:
                S.graph.launch()
                S.replays += 1
            else:
                self._step(S, sm, eos, pad)
            made += 1
        S.n = n0 + made
        return made

    def _rows_of(self, ids) -> List[List[int]]:
        if isinstance(ids, Tensor):
            ids = ids.tolist()
        if ids and isinstance(ids[0], dict):                    # one conversation
            ids = [ids]
        if ids and ids[0] and isinstance(ids[0][0], dict):      # conversations
            if self.tokenizer is None:
                raise _C.F5EError("Qwen2.generate: messages need the model's tokenizer")
            ids = [self.tokenizer.encode(apply_chat_template(m)) for m in ids]
        elif ids and isinstance(ids[0], int):
            ids = [ids]
        rows = [[int(t) for t in r] for r in ids]
        if not rows or any(not r for r in rows):
            raise _C.F5EError("Qwen2.generate: every row needs at least one token")
        V = self.cfg.vocab_size
        if any(t < 0 or t >= V for r in rows for t in r):
            raise _C.F5EError(f"Qwen2.generate: a token id lies outside 0 .. {V - 1}")
        return rows

    @torch.no_grad()
    def generate(self, ids, max_new_tokens: int = 512, do_sample: Optional[bool] = None, temperature: Optional[float] = None,
                 top_k: Optional[int] = None, top_p: Optional[float] = None, repetition_penalty: Optional[float] = None,
                 seed: int = 0, step_graph: bool = False, sync_every: int = 8, eos_token_id=None,
                 pad_token_id: Optional[int] = None, stats: Optional[dict] = None) -> Tuple[Tensor, List[int]]:
        """``ids``: token rows (a list of lists, ragged: shorter rows are left-padded), or messages / a list of conversations,
        rendered with the chat template.  None means the checkpoint's generation_config.  -> (tokens i32 [R, n_max] on the
        device: the generated tokens, ``pad`` behind a row's end; n: the tokens of every row, its closing eos included)."""
        rows = self._rows_of(ids)
        if not isinstance(step_graph, bool):
            raise _C.F5EError(f"Qwen2.generate: step_graph = {step_graph!r} must be a bool")
        sm = _sampling(self.gen, do_sample, temperature, top_k, top_p, repetition_penalty, self.cfg.vocab_size)
        eos = self.gen.eos_token_id if eos_token_id is None else eos_token_id
        eos = [int(eos)] if isinstance(eos, int) else [int(e) for e in eos]
        pad = pad_token_id if pad_token_id is not None else self.gen.pad_token_id
        pad = int(pad) if pad is not None else (eos[0] if eos else 0)
        R, U = len(rows), max(len(r) for r in rows)
        if U + max_new_tokens > MAX_POSITIONS:
            raise _C.F5EError(f"Qwen2.generate: a prompt of {U} tokens plus max_new_tokens = {max_new_tokens} exceeds the "
                              f"{MAX_POSITIONS}-position cap")
        S = self.new_state(R, U + max_new_tokens)
        begin = [U - len(r) for r in rows]
        table = torch.tensor([[pad] * b + r for b, r in zip(begin, rows)], dtype=I32)
        S.tokens.fill_(pad)
        S.tokens[:, :U] = table.to(self.device)
        S.begin.copy_(torch.tensor(begin, dtype=I32))
        S.row_key.copy_(torch.arange(R, dtype=I32))
        logits = self.append(S, S.tokens[:, :U], 0)
        S.n = U
        made = self.decode(S, logits, max_new_tokens, sm, eos, pad, seed, step_graph, sync_every)
        if stats is not None:
            stats.update(captures=S.captures, replays=S.replays, prefill_logits=logits)
        return finish_rows(S.tokens[:, U:U + made], eos, pad)


def finish_rows(gen: Tensor, eos: Sequence[int], pad: int) -> Tuple[Tensor, List[int]]:
    """The generated columns -> (tokens with ``pad`` behind each row's first eos, the rows' lengths, the eos included)."""
    gen = gen.clone()
    R, W = gen.shape
    host = gen.tolist()
    n = []
    for r, row in enumerate(host):
        k = next((i + 1 for i, t in enumerate(row) if t in eos), W)
        n.append(k)
        if k < W:
            gen[r, k:] = pad
    return gen, n


class ChatSession:
    """One conversation with a model: the caches and the ids behind them are kept across turns, and only a turn's new text is
    prefilled (the reference re-encodes the whole conversation every turn)."""

    def __init__(self, model: Qwen2, system_prompt: Optional[str] = None, positions: int = MAX_POSITIONS):
        self.model, self.system_prompt, self.positions = model, system_prompt, positions
        self.state: Optional[SimpleNamespace] = None
        self.clear()

    def clear(self) -> None:
        self.messages: List[dict] = [] if self.system_prompt is None else [dict(role="system", content=self.system_prompt)]
        self.ids: List[int] = []             # the conversation's tokens so far
        self.cached = 0                      # how many of them the caches hold
        self.prefilled: List[int] = []       # tokens prefilled per turn
        self.closed = False                  # the last reply ended on an eos id
        self.last_logits: Optional[Tensor] = None
        if self.state is not None:
            self.state.n = 0

    def _new_ids(self, user_text: str) -> List[int]:
        tok = self.model.tokenizer
        if tok is None:
            raise _C.F5EError("ChatSession.say: the model has no tokenizer (turn_ids takes token ids)")
        if not self.ids:
            return tok.encode(apply_chat_template(self.messages + [dict(role="user", content=user_text)]))
        end = tok.specials.get("<|im_end|>")
        if end is None:
            raise _C.F5EError("ChatSession.say: the tokenizer has no <|im_end|> token; the ChatML template needs it")
        closing = []
        if self.ids[-1] != end:
            if self.closed and len(self.ids) == self.cached + 1:
                self.ids[-1] = end           # the reply closed on another eos id (<|endoftext|>), which was picked but never fed:
            else:                            # the template renders <|im_end|> in its place; a reply cut at the bound gets one
                closing = [end]
        return closing + tok.encode("\n") + tok.encode(f"<|im_start|>user\n{user_text}<|im_end|>\n<|im_start|>assistant\n")

    @torch.no_grad()
    def turn_ids(self, new_ids: Sequence[int], max_new_tokens: int = 512, **kw) -> List[int]:
        """Feeds ``new_ids`` behind the conversation and generates: -> the generated ids, the closing eos included."""
        m = self.model
        if self.state is None:
            self.state = m.new_state(1, self.positions)
        S = self.state
        new_ids = [int(t) for t in new_ids]
        total = len(self.ids) + len(new_ids)
        if not new_ids or max_new_tokens < 1 or total + max_new_tokens > S.P:      # refused before the session changes
            raise _C.F5EError(f"ChatSession: the conversation's {total} tokens plus max_new_tokens = {max_new_tokens} exceed the "
                              f"{S.P}-position cap (or the turn is empty); clear() the session")
        sm = _sampling(m.gen, kw.pop("do_sample", None), kw.pop("temperature", None), kw.pop("top_k", None), kw.pop("top_p", None),
                       kw.pop("repetition_penalty", None), m.cfg.vocab_size)
        eos = kw.pop("eos_token_id", None)
        eos = m.gen.eos_token_id if eos is None else eos
        eos = [int(eos)] if isinstance(eos, int) else [int(e) for e in eos]
        pad = kw.pop("pad_token_id", None)
        pad = int(pad) if pad is not None else (m.gen.pad_token_id if m.gen.pad_token_id is not None else (eos[0] if eos else 0))
        seed, step_graph, sync_every = kw.pop("seed", 0), kw.pop("step_graph", False), kw.pop("sync_every", 8)
        if kw:
            raise _C.F5EError(f"ChatSession: unknown arguments {sorted(kw)}")
        self.ids += new_ids
        feed = self.ids[self.cached:]        # the previous turn's last token, which was picked but never fed, and the new text
        t = torch.tensor([feed], dtype=I32, device=m.device)
        S.tokens[:, self.cached:len(self.ids)] = t
        self.last_logits = m.append(S, t, self.cached)
        self.prefilled.append(len(feed))
        S.n = len(self.ids)
        made = m.decode(S, self.last_logits, max_new_tokens, sm, eos, pad, seed, step_graph, sync_every)
        _, n = finish_rows(S.tokens[:, len(self.ids):len(self.ids) + made], eos, pad)
        out = S.tokens[0, len(self.ids):len(self.ids) + n[0]].tolist()
        self.cached = len(self.ids) + n[0] - 1
        self.closed = bool(out) and out[-1] in eos
        self.ids += out
        S.n = len(self.ids)
        return out

    def say(self, user_text: str, max_new_tokens: int = 512, **kw) -> str:
        """One turn: the user's message in, the assistant's reply out (and into the conversation)."""
        out = self.turn_ids(self._new_ids(user_text), max_new_tokens, **kw)
        self.messages.append(dict(role="user", content=user_text))
        reply = self.model.tokenizer.decode_ids(out, skip_special_tokens=True)
        self.messages.append(dict(role="assistant", content=reply))
        return reply
