"""Float64 restatement of Paraformer (funasr paraformer-zh) as the issue that added it specifies it: WavFrontend (kaldi fbank,
LFR, CMVN), SANMEncoder, CifPredictorV2, ParaformerSANMDecoder and the pick.  Written from that specification, not from the
device code; one utterance at a time (a ragged batch is its rows).  ``dtype=torch.float32`` where exactness is tested.  It has
not been run against funasr or a real checkpoint."""
import math

import torch

F64 = torch.float64
LN_EPS = 1e-12


def rel_l2(got, want) -> float:
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    return float((got - want).norm() / want.norm().clamp_min(1e-300))


# ------------------------------------------------------------------ front-end
def hamming(n: int):
    return 0.54 - 0.46 * torch.cos(2 * math.pi * torch.arange(n, dtype=F64) / (n - 1))


def mel_banks(n_mels: int, padded: int = 512, sr: float = 16000.0, low: float = 20.0):
    """kaldi's triangular mel filters over the first padded / 2 bins (the Nyquist bin gets none) -> [padded / 2 + 1, n_mels]."""
    def mel(f):
        return 1127.0 * torch.log(1.0 + torch.as_tensor(f, dtype=F64) / 700.0)
    lo, hi = mel(low), mel(sr / 2)
    delta = (hi - lo) / (n_mels + 1)
    b = torch.arange(n_mels, dtype=F64)[:, None]
    left, center, right = lo + b * delta, lo + (b + 1) * delta, lo + (b + 2) * delta
    m = mel(sr / padded * torch.arange(padded // 2, dtype=F64))[None]
    w = torch.minimum((m - left) / (center - left), (right - m) / (right - center)).clamp_min(0.0)
    return torch.cat((w, torch.zeros(n_mels, 1, dtype=F64)), 1).t()


def fbank(wav, n_mels: int, win: int = 400, hop: int = 160):
    """kaldi fbank: wav * 32768, snip_edges frames, DC removal, pre-emphasis 0.97, Hamming, 512-point power spectrum, mel, log."""
    x = wav.to(F64) * 32768.0
    T = 1 + (x.numel() - win) // hop
    fr = x.unfold(0, win, hop)[:T]
    fr = fr - fr.mean(1, keepdim=True)
    prev = torch.cat((fr[:, :1], fr[:, :-1]), 1)
    fr = (fr - 0.97 * prev) * hamming(win)
    spec = torch.fft.rfft(torch.nn.functional.pad(fr, (0, 512 - win)), dim=1)
    power = spec.real ** 2 + spec.imag ** 2
    return torch.log((power @ mel_banks(n_mels)).clamp_min(1.1920928955078125e-07))


def lfr(x, m: int = 7, n: int = 6):
    """[T, C] -> [ceil(T / n), m C]: (m - 1) // 2 copies of frame 0 in front; row i = frames [n i, n i + m) of that sequence; a
    window that runs past the end repeats the last frame."""
    T = x.shape[0]
    Tp = -(-T // n)
    padded = torch.cat([x[:1]] * ((m - 1) // 2) + [x], 0)
    rows = []
    for i in range(Tp):
        idx = [min(n * i + j, padded.shape[0] - 1) for j in range(m)]
        rows.append(padded[idx].reshape(-1))
    return torch.stack(rows)


def position_table(rows: int, depth: int):
    half = depth // 2
    inv_t = torch.exp(-torch.arange(half, dtype=F64) * math.log(1e4) / (half - 1))
    p = torch.arange(1, rows + 1, dtype=F64)[:, None] * inv_t[None]
    return torch.cat((torch.sin(p), torch.cos(p)), 1)


def lfr_cmvn(fb, shift, scale, pos, m: int, n: int, xscale, dtype=F64):
    """The encoder's input from fbank frames: LFR, (x + shift) * scale, * xscale, + pos, each step rounded in ``dtype``."""
    x = lfr(fb.to(dtype), m, n)
    x = (x + shift.to(dtype)) * scale.to(dtype)
    x = x * torch.tensor(xscale, dtype=dtype)
    return x + pos[: x.shape[0]].to(dtype)


# ------------------------------------------------------------------ blocks
def layer_norm(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + LN_EPS) * w + b


def linear(x, w, b=None):
    y = x @ w.t()
    return y if b is None else y + b


def attention(q, k, v, heads: int):
    Tq, D = q.shape
    dk = D // heads
    qh, kh, vh = (t.view(-1, heads, dk).transpose(0, 1) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(1, 2) / math.sqrt(dk), -1)
    return (p @ vh).transpose(0, 1).reshape(Tq, D)


def fsmn(v, weight, shift: int = 0):
    """The memory block on the valid frames of one row: depthwise Conv1d over time, weight [D, 1, K], zero padding left =
    (K - 1) // 2 + shift, right = K - 1 - left; plus the input."""
    K = weight.shape[2]
    left = (K - 1) // 2 + shift
    x = torch.nn.functional.pad(v.t()[None], (left, K - 1 - left))
    y = torch.nn.functional.conv1d(x, weight.to(v.dtype), groups=v.shape[1])[0].t()
    return y + v


def sd64(sd):
    return {k: v.to(F64) for k, v in sd.items()}


def encoder_layer(sd, p, x, heads, shift):
    D = sd[p + "self_attn.linear_out.weight"].shape[0]
    h = layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"])
    q, k, v = linear(h, sd[p + "self_attn.linear_q_k_v.weight"], sd[p + "self_attn.linear_q_k_v.bias"]).split(D, -1)
    a = linear(attention(q, k, v, heads), sd[p + "self_attn.linear_out.weight"], sd[p + "self_attn.linear_out.bias"]) + \
        fsmn(v, sd[p + "self_attn.fsmn_block.weight"], shift)
    x = x + a if x.shape[1] == D else a
    h = layer_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"])
    return x + linear(torch.relu(linear(h, sd[p + "feed_forward.w_1.weight"], sd[p + "feed_forward.w_1.bias"])),
                      sd[p + "feed_forward.w_2.weight"], sd[p + "feed_forward.w_2.bias"])


def encoder(sd, cfg, x):
    x = encoder_layer(sd, "encoder.encoders0.0.", x, cfg.heads, cfg.sanm_shfit)
    for i in range(cfg.enc_layers - 1):
        x = encoder_layer(sd, f"encoder.encoders.{i}.", x, cfg.heads, cfg.sanm_shfit)
    return layer_norm(x, sd["encoder.after_norm.weight"], sd["encoder.after_norm.bias"])


def cif_alpha(logit, smooth=1.0, noise=0.0, tail=0.45):
    """Logits of the valid frames [T] -> alpha [T + 1] with the tail step, and n = floor(sum)."""
    a = torch.relu(torch.sigmoid(logit) * smooth - noise)
    a = torch.cat((a, torch.tensor([tail], dtype=a.dtype)))
    return a, int(torch.floor(a.sum()))


def predictor_alpha(sd, cfg, h):
    x = torch.nn.functional.pad(h.t()[None], (1, 1))
    y = torch.relu(torch.nn.functional.conv1d(x, sd["predictor.cif_conv1d.weight"], sd["predictor.cif_conv1d.bias"])[0].t())
    logit = linear(y, sd["predictor.cif_output.weight"], sd["predictor.cif_output.bias"])[:, 0]
    return cif_alpha(logit, cfg.smooth_factor, cfg.noise_threshold, cfg.tail_threshold)


def cif(alpha, h, threshold=1.0):
    """The literal per-step loop in the dtype of ``alpha``: alpha [T + 1] (tail last), h [T, D] (the tail's hidden state is zero)
    -> (emitted frames [fires, D], fire steps, the value of ``integrate`` at each fire decision)."""
    dt = alpha.dtype
    h = torch.cat((h.to(dt), torch.zeros(1, h.shape[1], dtype=dt)), 0)
    one, thr = torch.tensor(1.0, dtype=dt), torch.tensor(threshold, dtype=dt)
    integrate, frame = torch.tensor(0.0, dtype=dt), torch.zeros(h.shape[1], dtype=dt)
    out, pos, seen = [], [], []
    for t in range(alpha.numel()):
        comp = one - integrate
        integrate = integrate + alpha[t]
        seen.append(float(integrate))
        fire = bool(integrate >= thr)
        if fire:
            integrate = integrate - one
        cur = comp if fire else alpha[t]
        frame = frame + cur * h[t]
        if fire:
            out.append(frame)
            pos.append(t)
            frame = (alpha[t] - cur) * h[t]
    return (torch.stack(out) if out else torch.zeros(0, h.shape[1], dtype=dt)), pos, seen


def dec_ff(sd, p, x):
    h = layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"])
    h = torch.relu(linear(h, sd[p + "feed_forward.w_1.weight"], sd[p + "feed_forward.w_1.bias"]))
    return linear(layer_norm(h, sd[p + "feed_forward.norm.weight"], sd[p + "feed_forward.norm.bias"]), sd[p + "feed_forward.w_2.weight"])


def decoder_layer(sd, p, x, memory, heads, shift):
    D = x.shape[1]
    t = dec_ff(sd, p, x)
    s = x + fsmn(layer_norm(t, sd[p + "norm2.weight"], sd[p + "norm2.bias"]), sd[p + "self_attn.fsmn_block.weight"], shift)
    h = layer_norm(s, sd[p + "norm3.weight"], sd[p + "norm3.bias"])
    q = linear(h, sd[p + "src_attn.linear_q.weight"], sd[p + "src_attn.linear_q.bias"])
    k, v = linear(memory, sd[p + "src_attn.linear_k_v.weight"], sd[p + "src_attn.linear_k_v.bias"]).split(D, -1)
    return s + linear(attention(q, k, v, heads), sd[p + "src_attn.linear_out.weight"], sd[p + "src_attn.linear_out.bias"])


def decoder(sd, cfg, embeds, memory):
    x = embeds
    for i in range(cfg.dec_layers):
        x = decoder_layer(sd, f"decoder.decoders.{i}.", x, memory, cfg.dec_heads, cfg.dec_sanm_shfit)
    x = dec_ff(sd, "decoder.decoders3.0.", x)
    x = layer_norm(x, sd["decoder.after_norm.weight"], sd["decoder.after_norm.bias"])
    return torch.log_softmax(linear(x, sd["decoder.output_layer.weight"], sd["decoder.output_layer.bias"]), -1)


def pick(logp, cfg):
    """Log-probabilities of the first n tokens [n, V] -> (ids without sos / eos / blank, score)."""
    if logp.shape[0] == 0:
        return [], 0.0
    best, ids = logp.max(-1)          # torch's max returns the first of equal maxima on the CPU
    return [int(i) for i in ids if int(i) not in (cfg.sos, cfg.eos, cfg.blank)], float(best.sum())


def join_tokens(tokens):
    """CJK tokens with no separator; a token ending in @@ is glued to the next one; neighbouring Latin words get one space."""
    words, pend = [], ""
    for t in tokens:
        if t.endswith("@@"):
            pend += t[:-2]
        else:
            words.append(pend + t)
            pend = ""
    if pend:
        words.append(pend)
    out, prev_latin = "", False
    for w in words:
        latin = not all(0x2e80 <= ord(ch) <= 0x9fff for ch in w)
        out += (" " if latin and prev_latin else "") + w
        prev_latin = latin
    return out


def forward(sd, cfg, wav, shift, scale):
    """One utterance, float64 -> every stage: feats, enc, alpha, n, embeds, logp, ids, score, and the two margins the whole-model
    test asserts (``fire_margin`` = min |integrate - 1| over all fire decisions, ``frac`` = the fractional part of sum alpha)."""
    sd = sd64(sd)
    fb = fbank(wav, cfg.n_mels, 16 * cfg.frame_length, 16 * cfg.frame_shift)
    Tp = -(-fb.shape[0] // cfg.lfr_n)
    feats = lfr_cmvn(fb, shift, scale, position_table(Tp, cfg.in_width), cfg.lfr_m, cfg.lfr_n, math.sqrt(cfg.d_model))
    enc = encoder(sd, cfg, feats)
    alpha, n = predictor_alpha(sd, cfg, enc)
    frames, _, seen = cif(alpha, enc, cfg.threshold)
    embeds = frames[:n]
    logp = decoder(sd, cfg, embeds, enc) if n > 0 else torch.zeros(0, cfg.vocab, dtype=F64)
    ids, score = pick(logp, cfg)
    s = float(alpha.sum())
    return dict(feats=feats, enc=enc, alpha=alpha, n=n, fires=frames.shape[0], embeds=embeds, logp=logp, ids=ids, score=score,
                fire_margin=min(abs(v - 1.0) for v in seen), frac=s - math.floor(s))
