"""CPU restatement of the ECAPA-TDNN speaker-encoder head (f5e_tts_amd/eval/ecapa_tdnn.py, csrc/ecapa.hip) in plain torch,
channels-last, ragged batches included, and the synthetic weights the tests load into it.

``forward(sd, cfg, hs, lengths)`` takes a state dict with the reference's key names, hidden states [L, B, T, feat_dim] and
per-row lengths, and returns out1..out4 [B, T, C], the pooled vector [B, 3072] and the embedding [B, emb_dim].  A frame at or
beyond a row's length is zero after every conv -> ReLU -> BN, is zero padding for every convolution and is left out of every
mean, variance and softmax over time -- so row b equals the B = 1 run on its first lengths[b] frames.

``synth_state_dict(cfg, seed)``: every value is a counter-based hash (splitmix64 in uint64 arithmetic) of (seed, tensor
index, element index): the same bits on every machine, no RNG implementation involved.  Weights are uniform with variance
1 / fan_in so activations stay of order one through the stack; BatchNorm running_var lies in [0.5, 1.5], running means and
BN biases in +-0.3 (non-zero), BN weights in [0.5, 1.5], feature_weight in +-1."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

POOL_DIM, ATT_DIM, SE_DIM, SCALE = 1536, 128, 128, 8
DILATIONS = {"layer2": 2, "layer3": 3, "layer4": 4}


def make_cfg(feat_dim, channels=512, emb_dim=192, global_context_att=False, feat_num=25):
    return dict(feat_dim=feat_dim, channels=channels, emb_dim=emb_dim, global_context_att=bool(global_context_att),
                feat_num=feat_num)


def _bn_names(p: str, n: int) -> List[Tuple[str, tuple]]:
    return [(p + ".weight", (n,)), (p + ".bias", (n,)), (p + ".running_mean", (n,)), (p + ".running_var", (n,)),
            (p + ".num_batches_tracked", ())]


def head_shapes(cfg) -> List[Tuple[str, tuple]]:
    """(name, shape) of every parameter and buffer of the head, in the reference's state-dict order."""
    Fd, C, w = cfg["feat_dim"], cfg["channels"], cfg["channels"] // SCALE
    out = [("feature_weight", (cfg["feat_num"],)), ("layer1.conv.weight", (C, Fd, 5)), ("layer1.conv.bias", (C,))]
    out += _bn_names("layer1.bn", C)
    for lay in ("layer2", "layer3", "layer4"):
        out += [(f"{lay}.Conv1dReluBn1.conv.weight", (C, C, 1)), (f"{lay}.Conv1dReluBn1.conv.bias", (C,))]
        out += _bn_names(f"{lay}.Conv1dReluBn1.bn", C)
        for i in range(SCALE - 1):
            out += [(f"{lay}.Res2Conv1dReluBn.convs.{i}.weight", (w, w, 3)), (f"{lay}.Res2Conv1dReluBn.convs.{i}.bias", (w,))]
        for i in range(SCALE - 1):
            out += _bn_names(f"{lay}.Res2Conv1dReluBn.bns.{i}", w)
        out += [(f"{lay}.Conv1dReluBn2.conv.weight", (C, C, 1)), (f"{lay}.Conv1dReluBn2.conv.bias", (C,))]
        out += _bn_names(f"{lay}.Conv1dReluBn2.bn", C)
        out += [(f"{lay}.SE_Connect.linear1.weight", (SE_DIM, C)), (f"{lay}.SE_Connect.linear1.bias", (SE_DIM,)),
                (f"{lay}.SE_Connect.linear2.weight", (C, SE_DIM)), (f"{lay}.SE_Connect.linear2.bias", (C,))]
    att_in = POOL_DIM * (3 if cfg["global_context_att"] else 1)
    out += [("conv.weight", (POOL_DIM, 3 * C, 1)), ("conv.bias", (POOL_DIM,)),
            ("pooling.linear1.weight", (ATT_DIM, att_in, 1)), ("pooling.linear1.bias", (ATT_DIM,)),
            ("pooling.linear2.weight", (POOL_DIM, ATT_DIM, 1)), ("pooling.linear2.bias", (POOL_DIM,))]
    out += _bn_names("bn", 2 * POOL_DIM)
    out += [("linear.weight", (cfg["emb_dim"], 2 * POOL_DIM)), ("linear.bias", (cfg["emb_dim"],))]
    return out


def hash_uniform(seed: int, stream: int, n: int) -> np.ndarray:
    """n float64 in [0, 1): splitmix64 of the counter (seed, stream, index), top 53 bits."""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15) \
            + np.uint64(stream) * np.uint64(0xD1B54A32D192ED03)
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))


def hash_tensor(seed: int, stream: int, shape, lo: float, hi: float) -> torch.Tensor:
    n = int(np.prod(shape)) if len(shape) else 1
    v = lo + (hi - lo) * hash_uniform(seed, stream, n)
    return torch.from_numpy(v.astype(np.float32).reshape(shape))


def synth_state_dict(cfg, seed: int) -> Dict[str, torch.Tensor]:
    sd = {}
    for idx, (name, shape) in enumerate(head_shapes(cfg)):
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            sd[name] = torch.zeros((), dtype=torch.long)
        elif name == "feature_weight":
            sd[name] = hash_tensor(seed, idx, shape, -1.0, 1.0)
        elif leaf in ("running_var",) or (leaf == "weight" and len(shape) == 1):
            sd[name] = hash_tensor(seed, idx, shape, 0.5, 1.5)
        elif leaf == "running_mean" or (leaf == "bias" and (".bn" in name or name.startswith("bn.") or ".bns." in name)):
            sd[name] = hash_tensor(seed, idx, shape, -0.3, 0.3)
        elif leaf == "bias":
            sd[name] = hash_tensor(seed, idx, shape, -0.1, 0.1)
        else:  # conv / linear weight: variance 1 / fan_in
            a = math.sqrt(3.0 / float(np.prod(shape[1:])))
            sd[name] = hash_tensor(seed, idx, shape, -a, a)
    return sd


def synth_hidden_states(seed: int, L: int, B: int, T: int, feat_dim: int) -> torch.Tensor:
    """Hidden states [L, B, T, feat_dim] in +-2 with a per-layer offset, hashed like the weights."""
    h = hash_tensor(seed, 1_000_003, (L, B, T, feat_dim), -2.0, 2.0)
    return h + hash_tensor(seed, 1_000_033, (L, 1, 1, feat_dim), -0.5, 0.5)


# ---------------------------------------------------------------------------------------------------------------------

def _conv(x, w, b, dil=1):
    """Conv1d with 'same' zero padding on channels-last x [B, T, Cin]; w [Cout, Cin, k]."""
    k, T = w.shape[2], x.shape[1]
    pad = dil * (k - 1) // 2
    xp = F.pad(x, (0, 0, pad, pad))
    return b + sum(xp[:, j * dil: j * dil + T] @ w[:, :, j].T for j in range(k))


def _bn(x, sd, p):
    return (x - sd[p + ".running_mean"]) / torch.sqrt(sd[p + ".running_var"] + 1e-5) * sd[p + ".weight"] + sd[p + ".bias"]


def _crb(x, sd, p, mask, dil=1):
    return _bn(torch.relu(_conv(x, sd[p + ".conv.weight"], sd[p + ".conv.bias"], dil)), sd, p + ".bn") * mask


def layer_mix_inorm(hs, feature_weight, lengths):
    """[L, B, T, F] -> [B, T, F]: softmax(feature_weight)-weighted sum + 1e-6, instance norm over the valid frames."""
    L, B, T, Fd = hs.shape
    mask = (torch.arange(T, device=lengths.device)[None, :] < lengths[:, None]).to(hs.dtype)[..., None]
    n = lengths.to(hs.dtype).clamp(min=1)[:, None, None]
    x = (torch.softmax(feature_weight, 0)[:, None, None, None] * hs).sum(0) + 1e-6
    x = torch.where(mask > 0, x, torch.zeros_like(x))
    mean = x.sum(1, keepdim=True) / n
    var = (((x - mean) * mask) ** 2).sum(1, keepdim=True) / n
    return (x - mean) / torch.sqrt(var + 1e-5) * mask


def res2_chain(x, convs, bns, dil, mask):
    """convs: 7 x (weight [w, w, 3], bias [w]); bns: 7 x (scale [w], shift [w]) -- BatchNorm folded."""
    w = x.shape[2] // SCALE
    out, sp = [], None
    for i in range(SCALE - 1):
        xi = x[:, :, i * w:(i + 1) * w]
        sp = xi if i == 0 else sp + xi
        sp = (torch.relu(_conv(sp, convs[i][0], convs[i][1], dil)) * bns[i][0] + bns[i][1]) * mask
        out.append(sp)
    out.append(x[:, :, (SCALE - 1) * w:] * mask)
    return torch.cat(out, 2)


def fold_bn(sd, p):
    s = sd[p + ".weight"] / torch.sqrt(sd[p + ".running_var"] + 1e-5)
    return s, sd[p + ".bias"] - sd[p + ".running_mean"] * s


def se_gate(x, resid, w1, b1, w2, b2, lengths):
    n = lengths.to(x.dtype).clamp(min=1)[:, None]
    m = x.sum(1) / n                                   # x is zero beyond the length
    g = torch.sigmoid(torch.relu(m @ w1.T + b1) @ w2.T + b2)
    return x * g[:, None, :] + resid


def _block(x, sd, lay, mask, lengths):
    y = _crb(x, sd, f"{lay}.Conv1dReluBn1", mask)
    p = f"{lay}.Res2Conv1dReluBn"
    y = res2_chain(y, [(sd[f"{p}.convs.{i}.weight"], sd[f"{p}.convs.{i}.bias"]) for i in range(SCALE - 1)],
                   [fold_bn(sd, f"{p}.bns.{i}") for i in range(SCALE - 1)], DILATIONS[lay], mask)
    y = _crb(y, sd, f"{lay}.Conv1dReluBn2", mask)
    q = f"{lay}.SE_Connect"
    return se_gate(y, x, sd[q + ".linear1.weight"], sd[q + ".linear1.bias"], sd[q + ".linear2.weight"],
                   sd[q + ".linear2.bias"], lengths)


def context_stats(x, lengths):
    """mean and sqrt(unbiased variance + 1e-10) over the valid frames, [B, C] each (x zero beyond the length)."""
    T = x.shape[1]
    mask = (torch.arange(T, device=lengths.device)[None, :] < lengths[:, None]).to(x.dtype)[..., None]
    n = lengths.to(x.dtype)[:, None]
    mean = x.sum(1) / n
    var = (((x - mean[:, None]) * mask) ** 2).sum(1) / (n - 1)
    return mean, torch.sqrt(var + 1e-10)


def attn_stats_pool(x, logits, lengths):
    T = x.shape[1]
    valid = (torch.arange(T, device=lengths.device)[None, :] < lengths[:, None])[..., None]
    alpha = torch.softmax(logits.masked_fill(~valid, float("-inf")), 1)
    mean = (alpha * x).sum(1)
    std = torch.sqrt(((alpha * x * x).sum(1) - mean * mean).clamp(min=1e-9))
    return torch.cat([mean, std], 1)


def pooling(x, sd, lengths, global_context_att):
    w1, b1 = sd["pooling.linear1.weight"][:, :, 0], sd["pooling.linear1.bias"]
    pre = x @ w1[:, :POOL_DIM].T + b1
    if global_context_att:
        mean, std = context_stats(x, lengths)
        pre = pre + (torch.cat([mean, std], 1) @ w1[:, POOL_DIM:].T)[:, None, :]
    logits = torch.tanh(pre) @ sd["pooling.linear2.weight"][:, :, 0].T + sd["pooling.linear2.bias"]
    return attn_stats_pool(x, logits, lengths)


@torch.no_grad()
def forward(sd, cfg, hs, lengths: Optional[torch.Tensor] = None, dtype=torch.float32) -> Dict[str, torch.Tensor]:
    sd = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    hs = torch.as_tensor(hs).to(dtype)
    L, B, T, _ = hs.shape
    lengths = torch.full((B,), T, dtype=torch.long) if lengths is None else torch.as_tensor(lengths).long()
    lengths = lengths.to(hs.device)
    mask = (torch.arange(T, device=lengths.device)[None, :] < lengths[:, None]).to(dtype)[..., None]
    x = layer_mix_inorm(hs, sd["feature_weight"], lengths)
    out = {"feat": x}
    out["out1"] = _crb(x, sd, "layer1", mask)
    out["out2"] = _block(out["out1"], sd, "layer2", mask, lengths)
    out["out3"] = _block(out["out2"], sd, "layer3", mask, lengths)
    out["out4"] = _block(out["out3"], sd, "layer4", mask, lengths)
    cat = torch.cat([out["out2"], out["out3"], out["out4"]], 2)
    h = torch.relu(cat @ sd["conv.weight"][:, :, 0].T + sd["conv.bias"]) * mask
    out["pooled"] = pooling(h, sd, lengths, cfg["global_context_att"])
    out["emb"] = _bn(out["pooled"], sd, "bn") @ sd["linear.weight"].T + sd["linear.bias"]
    return out


def rel_l2(got, want) -> float:
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    return float((got - want).norm() / want.norm().clamp(min=1e-30))
