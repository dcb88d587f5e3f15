"""UTMOS (``utmos22_strong``; the reference fetches it through ``torch.hub``, eval/eval_utmos.py:18), from 16 kHz audio to one
naturalness score per utterance, on the device:

    wav2vec2-base (eval/wav2vec2.py) -> [B, T, D]; every frame joined with domain_emb[0] and judge_emb[0];
    BiLSTM (one layer, zero initial state) -> [B, T, 2 H]; Linear - ReLU - Linear -> one value per frame;
    score = 2 * (mean over the row's frames) + 3

The sub-modules only HOLD the weights (``blstm`` is an ``nn.LSTM`` for its parameter names alone).  At load they are folded:
  * the domain and judge columns of W_ih multiply constants, so they join the gate bias: W_ih[:, D:] [domain; judge] + b_ih + b_hh;
  * the W_ih[:, :D] of the two directions become ONE [2 * 4 H, D] operand: one f5e_gemm_f32 gives the input projections of every
    frame and direction, and f5e_lstm_f32 only runs the recurrence on W_hh (packed by ``ops.pack_lstm_weight``);
  * f5e_lstm_f32 takes hidden sizes that are multiples of 64: a smaller H is padded with units whose weights and biases are zero.
    Such a unit has g = tanh(0) = 0, so its cell and its output stay exactly 0 and nothing reads it through a non-zero weight.

The names ``wav2vec2.*``, ``domain_emb``, ``judge_emb``, ``blstm.*`` and ``projection.{0,2}.*`` are RESTATED from the published
predictor; no copy of it was at hand to verify them against.

Ragged batches: row b of a padded batch equals its own B = 1 run (the upstream's rule; the LSTM walks each row's own frames, the
backward direction from the row's last frame; the mean runs over the row's frames)."""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn as nn

from .. import _C, ops
from ..xfmr_f32 import plan, take, view
from .wav2vec2 import Wav2Vec2, Wav2Vec2Config, convert_hf_state_dict
from .wavlm import _f

Tensor = torch.Tensor
F32, I32 = torch.float32, torch.int32


def fold_lstm(blstm: nn.LSTM, const: Tensor, D: int):
    """(w_ih [ND * 4 Hp, D], bias [ND * 4 Hp], w_hh [ND, 4 Hp, Hp], Hp) in float64 from an ``nn.LSTM`` whose input is [x (D);
    const]: the constant columns go into the bias, H is padded to Hp = the next multiple of 64 with all-zero units (rows of a
    gate block, and columns of W_hh)."""
    H = blstm.hidden_size
    Hp = (H + 63) // 64 * 64
    nd = 2 if blstm.bidirectional else 1
    w_ih, bias, w_hh = [], [], []
    for d in range(nd):
        sfx = "_reverse" if d else ""
        wi, wh = getattr(blstm, "weight_ih_l0" + sfx).detach().double(), getattr(blstm, "weight_hh_l0" + sfx).detach().double()
        b = getattr(blstm, "bias_ih_l0" + sfx).detach().double() + getattr(blstm, "bias_hh_l0" + sfx).detach().double()
        b = b + wi[:, D:] @ const.detach().double().to(wi.device)
        wi_p, b_p, wh_p = wi.new_zeros(4, Hp, D), wi.new_zeros(4, Hp), wi.new_zeros(4, Hp, Hp)
        wi_p[:, :H], b_p[:, :H], wh_p[:, :H, :H] = wi[:, :D].view(4, H, D), b.view(4, H), wh.view(4, H, H)
        w_ih.append(wi_p.view(4 * Hp, D)), bias.append(b_p.view(-1)), w_hh.append(wh_p.view(4 * Hp, Hp))
    return torch.cat(w_ih, 0), torch.cat(bias, 0), torch.stack(w_hh), Hp


class UTMOS22Strong(nn.Module):
    def __init__(self, cfg: Optional[Wav2Vec2Config] = None, emb_dim: int = 128, lstm_hidden: int = 512, proj_hidden: int = 2048):
        super().__init__()
        self.wav2vec2 = Wav2Vec2(cfg)
        D = self.wav2vec2.cfg.encoder_embed_dim
        if emb_dim < 1 or not 1 <= lstm_hidden <= ops.LSTM_MAX_H or proj_hidden < 1:
            raise _C.F5EError(f"UTMOS22Strong: emb_dim = {emb_dim}, lstm_hidden = {lstm_hidden} (at most {ops.LSTM_MAX_H}), "
                              f"proj_hidden = {proj_hidden} are not built")
        self.domain_emb = nn.Parameter(0.1 * torch.randn(1, emb_dim))
        self.judge_emb = nn.Parameter(0.1 * torch.randn(1, emb_dim))
        self.blstm = nn.LSTM(D + 2 * emb_dim, lstm_hidden, batch_first=True, bidirectional=True)
        self.projection = nn.Sequential(nn.Linear(2 * lstm_hidden, proj_hidden), nn.ReLU(), nn.Linear(proj_hidden, 1))
        self._head = None
        super().train(False)
        for p in self.parameters():
            p.requires_grad_(False)

    @classmethod
    def from_checkpoint(cls, state_dict: Dict[str, Tensor], prefix: str = "", **kw) -> "UTMOS22Strong":
        """``state_dict``: the predictor's checkpoint (keys below ``prefix``); ``wav2vec2.*`` keys in ``transformers`` naming are
        converted.  Every key of this module must be there."""
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        up = {k[len("wav2vec2."):]: v for k, v in sd.items() if k.startswith("wav2vec2.")}
        if any(".conv.weight" in k or k.startswith("feature_projection.") for k in up):
            up = convert_hf_state_dict(up)
        sd = {k: v for k, v in sd.items() if not k.startswith("wav2vec2.")}
        sd.update({"wav2vec2." + k: v for k, v in up.items()})
        model = cls(**kw)
        missing, _unexpected = model.load_state_dict(sd, strict=False)
        if missing:
            raise _C.F5EError(f"UTMOS22Strong.from_checkpoint: the checkpoint lacks {len(missing)} keys, e.g. {missing[:3]}")
        return model

    # ---- eval mode only; the head as the kernels take it, once per load ------------------------------------------------------
    def train(self, mode: bool = True):
        if mode:
            raise _C.F5EError("UTMOS22Strong: training is out of scope (eval mode only)")
        return nn.Module.train(self, False)

    def _apply(self, fn, *a, **kw):
        self._head = None
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, *a, **kw):
        self._head = None
        return super().load_state_dict(*a, **kw)

    def _fold(self) -> dict:
        dev = self.domain_emb.device
        if self._head is not None and self._head["device"] == dev:
            return self._head
        if dev.type != "cuda":
            raise _C.F5EError(f"UTMOS22Strong lives on {dev}: move it to the GPU (there is no CPU path)")
        D, H = self.wav2vec2.cfg.encoder_embed_dim, self.blstm.hidden_size
        const = torch.cat([self.domain_emb[0], self.judge_emb[0]])
        w_ih, bias, w_hh, Hp = fold_lstm(self.blstm, const, D)
        l1, l2 = self.projection[0], self.projection[2]
        w1 = l1.weight.detach().new_zeros(l1.out_features, 2, Hp)
        w1[:, :, :H] = l1.weight.detach().view(l1.out_features, 2, H)          # the padded units meet zero columns
        self._head = dict(device=dev, H=H, Hp=Hp, w_ih=_f(w_ih, dev), b_ih=_f(bias, dev), w_hh=ops.pack_lstm_weight(w_hh).to(dev),
                          w1=_f(w1.view(l1.out_features, 2 * Hp), dev), b1=_f(l1.bias, dev), w2=_f(l2.weight.reshape(-1), dev),
                          b2=_f(l2.bias.reshape(1), dev))
        return self._head

    # ---- workspace -----------------------------------------------------------------------------------------------------------
    def _plan(self, B: int, S: int):
        T = max(self.wav2vec2.frame_count(S), 1)
        D, Hp, P = self.wav2vec2.cfg.encoder_embed_dim, (self.blstm.hidden_size + 63) // 64 * 64, self.projection[0].out_features
        M = B * T
        pl = plan(dict(hid=(B, T, D), xg=(M, 8 * Hp), lstm=(B, T, 2 * Hp), cell=(2, B, Hp), p1=(M, P)))
        pl["_up"] = pl.pop("_total")
        return pl, pl["_up"][0] + self.wav2vec2.workspace_bytes(B, S) // 4

    def workspace_bytes(self, B: int, S: int) -> int:
        """Scratch bytes of ``predict`` for B rows of S samples, the upstream's included (host arithmetic)."""
        return self._plan(int(B), int(S))[1] * 4

    # ---- forward -------------------------------------------------------------------------------------------------------------
    def _run(self, wav16k: Tensor, lengths, out, workspace, frame_scores):
        if not isinstance(wav16k, Tensor) or wav16k.ndim != 2 or wav16k.dtype != F32 or not wav16k.is_cuda:
            raise _C.F5EError("UTMOS22Strong.predict: wav16k must be a float32 GPU tensor [B, S]; there is no CPU path")
        B, S = wav16k.shape
        if not 1 <= B <= ops.LSTM_MAX_B:
            raise _C.F5EError(f"UTMOS22Strong.predict: B = {B} rows (1 .. {ops.LSTM_MAX_B} are built)")
        T = self.wav2vec2.frame_count(S)
        if not 1 <= T <= ops.LSTM_MAX_T:
            raise _C.F5EError(f"UTMOS22Strong.predict: {S} samples give {T} frames (1 .. {ops.LSTM_MAX_T} are built; a row needs "
                              f"{self.wav2vec2.min_samples()} samples)")
        dev = wav16k.device
        hd = self._fold()
        pl, total = self._plan(B, S)
        ws = take(workspace, total, dev, "UTMOS22Strong.predict")
        if out is None:
            out = torch.empty(B, dtype=F32, device=dev)
        elif out.shape != (B,) or out.dtype != F32 or not out.is_cuda:
            raise _C.F5EError(f"UTMOS22Strong.predict: out must be an f32 GPU tensor [{B}]")
        if frame_scores is not None and (frame_scores.shape != (B, T) or frame_scores.dtype != F32 or not frame_scores.is_cuda):
            raise _C.F5EError(f"UTMOS22Strong.predict: frame_scores must be an f32 GPU tensor [{B}, {T}]")

        hid, xg, lstm, cell, p1 = (view(ws, pl, name) for name in ("hid", "xg", "lstm", "cell", "p1"))
        _, frames = self.wav2vec2.extract(wav16k, lengths, out=hid, workspace=ws[pl["_up"][0]:total])
        M, D = B * T, hid.shape[2]
        ops.gemm_f32(hid.view(M, D), hd["w_ih"], hd["b_ih"], out=xg)          # both directions, every frame, constants folded
        ops.lstm_f32(xg, hd["w_hh"], frames, lstm, cell)
        ops.gemm_f32(lstm.view(M, -1), hd["w1"], hd["b1"], out=p1, act=ops.ACT_RELU)
        ops.score_mean(p1, hd["w2"], hd["b2"], frames, out, B, scale=2.0, offset=3.0, frame_scores=frame_scores)
        return out, frames, hid, lstm

    @torch.no_grad()
    def predict(self, wav16k: Tensor, lengths=None, *, out: Optional[Tensor] = None, workspace: Optional[Tensor] = None,
                frame_scores: Optional[Tensor] = None) -> Tensor:
        """wav16k f32 [B, S] on the GPU, 16 kHz, raw; lengths as ``Wav2Vec2.extract`` takes them -> scores f32 [B].
        ``frame_scores`` f32 [B, T] (optional) receives the per-frame values before the mean, zero beyond a row's frames.  No
        device-to-host copy, no synchronisation; with ``out``, ``workspace`` (``workspace_bytes(B, S)`` bytes) and device lengths
        it allocates nothing once the weights are folded (a first call does that), so it can be captured into a graph: T + 4
        launches for the head after the upstream's."""
        return self._run(wav16k, lengths, out, workspace, frame_scores)[0]

    @torch.no_grad()
    def parts(self, wav16k: Tensor, lengths=None) -> dict:
        """The intermediate tensors of ``predict`` (allocates; for tests and diagnostics): ``hidden`` [B, T, D], ``blstm`` [B, T,
        2 H] without the padding units, ``frame_scores`` [B, T], ``scores`` [B], ``frames`` i32 [B]."""
        B, T = wav16k.shape[0], self.wav2vec2.frame_count(wav16k.shape[1])
        fs = torch.empty(B, max(T, 1), dtype=F32, device=wav16k.device)
        out, frames, hid, lstm = self._run(wav16k, lengths, None, None, fs)
        H, Hp = self._head["H"], self._head["Hp"]
        return dict(hidden=hid.clone(), blstm=lstm.view(B, T, 2, Hp)[..., :H].reshape(B, T, 2 * H), frame_scores=fs, scores=out,
                    frames=frames.clone())

    @torch.no_grad()
    def forward(self, wave: Tensor, sr: int) -> Tensor:
        """The reference's call (eval_utmos.py:29): wave [B, S] (or [S]) on the GPU at ``sr`` Hz -> scores f32 [B]; resampled to
        16 kHz on the device."""
        from ..infer.audio import resample_device
        if not isinstance(wave, Tensor) or not wave.is_cuda or wave.ndim not in (1, 2):
            raise _C.F5EError("UTMOS22Strong: forward takes a GPU tensor [B, S] or [S]; there is no CPU path")
        wave = wave[None] if wave.ndim == 1 else wave
        return self.predict(resample_device(wave.to(F32), int(sr), 16000).contiguous())
