"""Whisper on the GPU (csrc/whisper.hip, eval/whisper.py) against
  * the fixture made from ``transformers`` (tests/golden/whisper.npz): features, encoder output and teacher-forced logits at
    relative L2 < 2e-4, the project's gate for fp32 chains against reference fixtures (tests/test_wavlm_gpu.py); the greedy token
    sequences exactly (every step's margin in the fixture is >= 1e-2 of the logits' RMS, 50x that gate), for sync_every 1 and 8;
  * its own B = 1 runs for the rows of a ragged batch (1e-5, tests/test_ecapa_gpu.py's figure for the same property);
  * the float64 restatement (tests/whisper_ref.py, pinned by the same fixture), kernel by kernel.

Bounds.  tol(K) = 10 * sqrt(K) * 2^-24: one rounding of 2^-24 per operation grows like sqrt(K) as a root mean square over a chain
of K fp32 operations; ten times that (the rule of tests/test_ecapa_gpu.py).

f5e_cross_attn_decode_f32: relative L2 < tol(Tk + dk) (the dk products of a score, the Tk terms of the context).

f5e_whisper_logmel: an ABSOLUTE bound per output cell, on the output scale, from tol(K) on the power with K = 400 + 201 (the
DFT's terms and the filterbank's).  With E_f = sum_n (x_n w_n)^2 of frame f (the root-sum-square scale of the DFT's summands):
    |d X_k|   <= tol(K) sqrt(E_f)                                   (each of re, im; a 400-term fp32 sum)
    d p_k     <= 2 sqrt(p_k) |d X_k| sqrt(2) + 2 |d X_k|^2          (p = re^2 + im^2)
    d mel_m   <= sum_k fb[k][m] d p_k + tol(K) mel_m                (non-negative terms: the sum's own error is relative)
    d out     <= d mel / (mel ln 10) / 4 + 2^-21 (|log10 mel| + 4) / 4   (d log10(x) / 4, then log10f's and the affine's ulps)
A cell whose power is small against its frame's energy (cancellation in the DFT) gets a wide bound, a dominant one a tight one,
which is what fp32 can do.  Cross-check: the same formulas evaluated by NumPy in float32 (tests/whisper_ref.py, a sequential
float32 DFT) are held to the same bound and their worst ratio is printed next to the kernel's.  Cells of all-zero frames (the
padding) have power exactly 0 and must come out exactly at the clamp: (rowmax - 8 + 4) / 4 of the kernel's own rowmax, or at the
floor (log10(1e-10) + 4) / 4 = -1.5 where the row is so quiet that rowmax - 8 lies below it (the one-sample row).

f5e_greedy_pick: exact.

Every test prints its measured error before it asserts.

Measured on an MI355X: see DESIGN.md 4o."""
import math

import numpy as np
import pytest
import torch

import whisper_ref as R
from test_whisper_cpu import gold, tiny_model

pytestmark = pytest.mark.gpu

GATE, ROW_GATE = 2e-4, 1e-5
F32, I32 = torch.float32, torch.int32
HOP = 160


def tol(K):
    return 10.0 * math.sqrt(K) * 2.0 ** -24


_dev = {}


def model_gpu(eos_case=False):
    key = ("model", eos_case)
    if key not in _dev:
        _dev[key] = tiny_model(eos_case).cuda()
    return _dev[key]


def wave_gpu(n):
    return torch.from_numpy(gold()["wave_f32"][:n].copy()).cuda()[None]


def kv_gpu(n, eos_case=False):
    key = ("kv", n, eos_case)
    if key not in _dev:
        _dev[key] = model_gpu(eos_case).encode(wave_gpu(n))
    return _dev[key]


# ---- end to end against the fixture ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (14400, 40000, 48000))
def test_fixture_features_encoder_and_logits(n):
    fx, model = gold(), model_gpu()
    feats = model.features(wave_gpu(n))
    got = feats[0].cpu().numpy()
    want = fx[f"feat_{n}"]
    e_feat = R.rel_l2(got[fx[f"feat_idx_{n}"]] if f"feat_idx_{n}" in fx else got, want)
    enc = model.encode_features(feats)
    e_enc = R.rel_l2(enc[0].cpu().numpy(), fx[f"enc_{n}"])
    ids = torch.from_numpy(fx[f"tokens_{n}"][:12].copy()).cuda()[None]
    logits = model.decoder_logits(model.cross_kv(enc), ids)
    e_log = R.rel_l2(logits[0].cpu().numpy(), fx[f"logits_{n}"])
    print(f"n={n}: features {e_feat:.2e}, encoder {e_enc:.2e}, teacher-forced logits {e_log:.2e} (gate {GATE:g})")
    assert torch.isfinite(logits).all()
    assert e_feat < GATE and e_enc < GATE and e_log < GATE


def test_fixture_features_with_80_filters():
    from f5e_tts_amd import ops
    from f5e_tts_amd.eval import whisper as W
    fx = gold()
    dev = torch.device("cuda")
    got = ops.whisper_logmel(wave_gpu(14400), None, torch.from_numpy(W.hann_window()).to(dev, F32),
                             torch.from_numpy(W.dft_twiddle()).to(dev, F32), torch.from_numpy(W.mel_filters(80)).to(dev, F32), 300)
    e = R.rel_l2(got[0].cpu().numpy()[fx["feat_idx_14400"]], fx["feat80_14400"])
    print(f"80 filters: {e:.2e} (gate {GATE:g})")
    assert e < GATE


@pytest.mark.parametrize("sync_every", (1, 8))
@pytest.mark.parametrize("case", ("14400", "40000", "48000", "eos"))
def test_greedy_tokens_equal_the_fixture(case, sync_every):
    fx = gold()
    eos_case = case == "eos"
    n = 14400 if eos_case else int(case)
    model = model_gpu(eos_case)
    tokens, cnt = model.generate_from_kv(kv_gpu(n, eos_case), fx["prompt"].tolist(), sync_every=sync_every)
    want = fx[f"tokens_{case}"].tolist()
    got = tokens[0, :int(cnt[0])].tolist()
    print(f"{case} sync_every={sync_every}: {len(got)} tokens, first difference at "
          f"{next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)}")
    assert got == want
    assert tokens.shape == (1, 48) and (tokens[0, int(cnt[0]):] == 140).all()       # eos from the row's end on


def test_generate_from_audio_and_max_new_tokens():
    fx, model = gold(), model_gpu()
    tokens, cnt = model.generate(wave_gpu(40000), None, "english", max_new_tokens=5, sync_every=3)
    assert tokens.shape == (1, 9) and int(cnt[0]) == 9 and tokens[0].tolist() == fx["tokens_40000"][:9].tolist()


def test_ragged_pair_equals_its_own_single_runs():
    fx, model = gold(), model_gpu()
    lens = (40000, 14400)
    S = 41000
    pair = torch.full((2, S), 1e4, dtype=F32)                       # garbage beyond len, whatever the buffer holds
    pair[1] = torch.sin(torch.arange(S) * 0.37) * 3e3
    for b, n in enumerate(lens):
        pair[b, :n] = torch.from_numpy(fx["wave_f32"][:n].copy())
    pair = pair.cuda()
    feats = model.features(pair, list(lens))
    enc = model.encode_features(feats)
    tokens, cnt = model.generate(pair, torch.tensor(lens, dtype=I32).cuda(), "en", sync_every=8)
    for b, n in enumerate(lens):
        f1 = model.features(wave_gpu(n))
        e1 = model.encode_features(f1)
        ef, ee = R.rel_l2(feats[b].cpu().numpy(), f1[0].cpu().numpy()), R.rel_l2(enc[b].cpu().numpy(), e1[0].cpu().numpy())
        print(f"row {b} (n={n}): features {ef:.2e}, encoder {ee:.2e} against the B = 1 run (gate {ROW_GATE:g})")
        assert ef < ROW_GATE and ee < ROW_GATE
        assert tokens[b, :int(cnt[b])].tolist() == fx[f"tokens_{n}"].tolist()


# ---- f5e_whisper_logmel against float64 --------------------------------------------------------------------------------------

def logmel_bound(wav, length, T, fb):
    """(reference [T][n_mels] in float64, the per-cell absolute bound of the module docstring, the all-zero-frame mask)."""
    p, _ = R.power_frames(wav, length, T)
    N = HOP * T
    row = np.zeros(N)
    n = min(int(length), len(wav), N)
    row[:n] = wav[:n]
    padded = np.pad(row, (200, 200), mode="reflect")
    idx = np.arange(T)[:, None] * HOP + np.arange(400)[None, :]
    E = ((padded[idx] * R.hann()[None, :]) ** 2).sum(1)
    t = tol(400 + 201)
    dX = t * np.sqrt(E)[:, None]
    dp = 2.0 * np.sqrt(p) * dX * math.sqrt(2.0) + 2.0 * dX ** 2
    mel = p @ fb
    dmel = dp @ fb + t * mel
    safe = np.maximum(mel, 1e-300)
    bound = dmel / (safe * math.log(10.0)) / 4.0 + 2.0 ** -21 * (np.abs(np.log10(safe)) + 4.0) / 4.0
    return R.log_mel(wav, length, T, fb), bound, (E == 0.0)


LOGMEL_CASES = {
    # name: (T, S, lens)
    "T10": (10, 1637, (1, 199, 200, 201, 1599, 1600)),          # the reflect pad reaches past the data; hop*T - 1 and hop*T
    # a buffer shorter than hop * T, more than one workgroup; len = 120 mod 160, so that the last live frame holds 160 samples
    # (one that held 40 samples under the window's foot would fall below rowmax - 8, and no live cell may sit at the clamp)
    "T300": (300, 40500, (40120, 20120)),
}


@pytest.mark.parametrize("n_mels", (80, 128))
@pytest.mark.parametrize("name", sorted(LOGMEL_CASES))
def test_logmel_against_float64(name, n_mels):
    from f5e_tts_amd import ops
    from f5e_tts_amd.eval import whisper as W
    T, S, lens = LOGMEL_CASES[name]
    B = len(lens)
    g = torch.Generator().manual_seed(11 + T)
    t = torch.arange(S) / 16000.0
    wav = 0.1 * torch.randn(B, S, generator=g) + 0.1 * torch.sin(2 * math.pi * 440.0 * t)[None]       # a noise floor under a tone
    wav[:, 0] = 0.25
    wav = (torch.round(wav * 32768) / 32768).to(F32)
    buf = wav.clone()
    for b, n in enumerate(lens):
        buf[b, n:] = 1e4                                            # must not matter
    fb64 = R.slaney_filters(n_mels)
    dev = torch.device("cuda")
    out = ops.whisper_logmel(buf.cuda(), torch.tensor(lens, dtype=I32).cuda(), torch.from_numpy(W.hann_window()).to(dev, F32),
                             torch.from_numpy(W.dft_twiddle()).to(dev, F32), torch.from_numpy(fb64).to(dev, F32), T)
    got = out.cpu().numpy().astype(np.float64)
    assert got.shape == (B, T, n_mels) and np.isfinite(got).all()
    for b, n in enumerate(lens):
        w64 = wav[b].numpy().astype(np.float64)
        ref, bound, zero = logmel_bound(w64, n, T, fb64)
        ref32 = R.log_mel(wav[b].numpy(), n, T, fb64, dtype=np.float32).astype(np.float64)
        clamp = ref.max() - 2.0                                     # (rowmax - 8 + 4) / 4 on the output scale
        live = ~zero[:, None] & (ref > clamp + 1e-3)                # the noise floor keeps every live cell off the clamp
        assert live[~zero].all(), "a live cell sits at the clamp: the test's inputs lack their noise floor"
        ratio = np.abs(got[b] - ref)[live] / np.broadcast_to(bound, ref.shape)[live]
        ratio32 = np.abs(ref32 - ref)[live] / np.broadcast_to(bound, ref.shape)[live]
        print(f"{name} n_mels={n_mels} len={n}: max |err| {np.abs(got[b] - ref)[live].max():.2e}, worst err / bound "
              f"{ratio.max():.3f} (NumPy float32: {ratio32.max():.3f}), {int(zero.sum())} zero frames")
        assert ratio.max() < 1.0 and ratio32.max() < 1.0
        if zero.any():
            cells = out[b].cpu()[torch.from_numpy(zero)]
            # the kernel's own rowmax, in fp32 -- or the floor log10(1e-10) where the row is so quiet that rowmax - 8 lies below it
            want = torch.maximum((out[b].max().cpu() * 4.0 - 4.0 - 8.0 + 4.0) / 4.0, torch.tensor(-1.5))
            print(f"    padding cells: {cells.min().item():.9g} .. {cells.max().item():.9g}, clamp {want.item():.9g}")
            assert (cells == cells[0, 0]).all() and abs(cells[0, 0].item() - want.item()) <= 2.0 ** -22 * 2


def test_logmel_refusals():
    from f5e_tts_amd import _C, ops
    from f5e_tts_amd.eval import whisper as W
    dev = torch.device("cuda")
    win, tw = torch.from_numpy(W.hann_window()).to(dev, F32), torch.from_numpy(W.dft_twiddle()).to(dev, F32)
    wav = torch.zeros(1, 1600, device=dev)
    with pytest.raises(_C.F5EError, match="80 or 128"):
        ops.whisper_logmel(wav, None, win, tw, torch.zeros(201, 64, device=dev), 10)
    with pytest.raises(_C.F5EError, match="T >= 2"):
        ops.whisper_logmel(wav, None, win, tw, torch.zeros(201, 80, device=dev), 1)


# ---- f5e_cross_attn_decode_f32 against float64 -------------------------------------------------------------------------------

def cross_ref(q, K, V, H, scale, rpu, kv_len):
    R_, D = q.shape
    dk = D // H
    out = np.zeros((R_, D))
    for r in range(R_):
        u = r // rpu
        n = K.shape[1] if kv_len is None else kv_len[u]
        if n == 0:
            continue
        for h in range(H):
            sl = slice(h * dk, (h + 1) * dk)
            s = scale * (K[u, :n, sl] @ q[r, sl])
            e = np.exp(s - s.max())
            out[r, sl] = (e / e.sum()) @ V[u, :n, sl]
    return out


@pytest.mark.parametrize("dk", (16, 64))
@pytest.mark.parametrize("Tk", (1, 63, 64, 65, 1500))
def test_cross_attn_decode_against_float64(Tk, dk):
    from f5e_tts_amd import ops
    H, B = 3, 2
    D = H * dk
    g = torch.Generator().manual_seed(1000 * dk + Tk)
    for rpu in (1, 3):
        R_ = B * rpu
        q = torch.randn(R_, D, generator=g, dtype=torch.float64)
        q[R_ - 1] = 0.0                                            # a row whose scores are all equal: the mean of the values
        kv = torch.randn(B, Tk, 2 * D + 4, generator=g, dtype=torch.float64)      # k | v side by side: row strides beyond D
        K, V = kv[..., :D], kv[..., D:2 * D]
        for lens in (None, (Tk, 0) if Tk == 1 else (Tk - 1, Tk // 2)):
            qd = q.to(F32).cuda()
            kvd = kv.to(F32).cuda()
            outbuf = torch.full((R_, D + 8), -7.0, dtype=F32, device="cuda")
            ops.cross_attn_decode_f32(qd, kvd[..., :D], kvd[..., D:2 * D], H, dk ** -0.5, rows_per_utt=rpu,
                                      kv_len=None if lens is None else torch.tensor(lens, dtype=I32).cuda(), out=outbuf[:, :D])
            got = outbuf.cpu().numpy().astype(np.float64)
            ref = cross_ref(q.to(F32).double().numpy(), K.to(F32).double().numpy(), V.to(F32).double().numpy(), H, dk ** -0.5,
                            rpu, lens)
            err = float(np.linalg.norm(got[:, :D] - ref) / np.linalg.norm(ref))
            print(f"Tk={Tk} dk={dk} rows_per_utt={rpu} kv_len={lens}: rel L2 {err:.2e} (bound {tol(Tk + dk):.2e})")
            assert (got[:, D:] == -7.0).all(), "padding columns beyond H * dk were written"
            assert err < tol(Tk + dk)
            if lens is not None and 0 in lens:
                assert (got[rpu * lens.index(0):rpu * (lens.index(0) + 1), :D] == 0.0).all()       # no visible key: zeros


def test_cross_attn_decode_refusals():
    from f5e_tts_amd import _C, ops
    q = torch.zeros(2, 48, device="cuda")
    k = torch.zeros(1, 5, 48, device="cuda")
    with pytest.raises(_C.F5EError, match="head dim"):
        ops.cross_attn_decode_f32(q, k, k, 2, 1.0, rows_per_utt=2)          # dk = 24
    with pytest.raises(_C.F5EError, match="inconsistent"):
        ops.cross_attn_decode_f32(q, k, k, 3, 1.0, rows_per_utt=1)          # 2 rows, 1 utterance


# ---- f5e_greedy_pick, exact --------------------------------------------------------------------------------------------------

def pick_ref(logits, V, sup, beg, first, done, eos):
    toks, done = [], list(done)
    for r in range(logits.shape[0]):
        if done[r]:
            toks.append(eos)
            continue
        l = logits[r, :V].astype(np.float64).copy()
        l[[s for s in sup if 0 <= s < V]] = -np.inf
        if first:
            l[[s for s in beg if 0 <= s < V]] = -np.inf
        toks.append(int(np.argmax(l)))                             # the first of equal maxima
        if toks[-1] == eos:
            done[r] = 1
    return toks, done


@pytest.mark.parametrize("V,ld", ((1, 1), (63, 63), (64, 64), (65, 68), (51866, 51868)))
def test_greedy_pick_exact(V, ld):
    from f5e_tts_amd import ops
    Rr, p, eos = 6, 3, 0 if V == 1 else V - 2
    g = torch.Generator().manual_seed(V)
    logits = torch.randn(Rr, ld, generator=g)
    logits[:, V:] = 1e9                                            # beyond V: never read as a class
    if V > 8:
        logits[0, [5, V - 1, 7]] = 50.0                            # a tie: the lowest index wins
        logits[1, 3] = 60.0                                        # the raw maximum is suppressed
        logits[2, 4] = 60.0                                        # suppressed at the first step only
        logits[3, eos] = 70.0                                      # picks eos: becomes done
        logits[4, 6] = 80.0                                        # already done: stays eos
    sup, beg = [3, -1, V + 5, 2], [4, 4]
    done0 = [0, 0, 0, 0, 1, 0]
    for first in (True, False):
        tokens = torch.full((Rr, p + 4), -5, dtype=I32).cuda()
        last, alive = torch.full((Rr,), -5, dtype=I32).cuda(), torch.full((3,), -5, dtype=I32).cuda()
        done = torch.tensor(done0, dtype=I32).cuda()
        ld_before = logits.clone()
        dl = logits.cuda()
        ops.greedy_pick(dl[:, :V] if ld > V else dl, tokens, last, done, alive[1:2], p, eos, V=V,
                        suppress=torch.tensor(sup, dtype=I32).cuda(), begin_suppress=torch.tensor(beg, dtype=I32).cuda(),
                        first_step=first)
        want, want_done = pick_ref(logits.numpy(), V, sup, beg, first, done0, eos)
        got = tokens[:, p + 1].tolist()
        print(f"V={V} ld={ld} first_step={first}: tokens {got}, done {done.tolist()}, alive {alive[1].item()}")
        assert got == want and last.tolist() == want and done.tolist() == want_done
        assert alive[1].item() == want_done.count(0)
        assert alive[0].item() == -5 and alive[2].item() == -5                         # cells outside the documented ones
        rest = tokens.clone()
        rest[:, p + 1] = -5
        assert (rest == -5).all() and torch.equal(dl.cpu(), ld_before)
        if V > 8:
            assert got[0] == 5 and got[1] != 3 and (got[2] == 4) == (not first) and got[3] == eos and got[4] == eos


def test_greedy_pick_refusals():
    from f5e_tts_amd import _C, ops
    z = lambda *s: torch.zeros(*s, dtype=I32, device="cuda")       # noqa: E731
    with pytest.raises(_C.F5EError, match="eos"):
        ops.greedy_pick(torch.zeros(2, 8, device="cuda"), z(2, 4), z(2), z(2), z(1), 0, 8)
    with pytest.raises(_C.F5EError):
        ops.greedy_pick(torch.zeros(2, 8, device="cuda"), z(2, 4), z(2), z(2), z(1), 3, 1)     # tokens needs p + 2 columns


# ---- one full-width smoke test --------------------------------------------------------------------------------------------------

def test_full_width_tokens_equal_the_float64_argmax():
    """d 1280, 20 heads, 2 + 2 layers, 1500 positions, vocab 51866, synthetic weights: finite outputs, and the 4 generated tokens
    equal the float64 restatement's teacher-forced argmax (whose margins are printed: >= 1e-2 of the logits' RMS, asserted)."""
    from f5e_tts_amd.eval.whisper import Whisper, WhisperConfig
    from tools import synth as SY
    fields = SY.whisper_config_fields(encoder_layers=2, decoder_layers=2)
    model = Whisper(WhisperConfig(**fields))
    sd = SY.init_whisper_state({k: v.shape for k, v in model.state_dict().items()}, 99, 4.0)
    model.load_state_dict(sd, strict=False)
    full = {k: v.numpy() for k, v in model.state_dict().items()}
    model = model.cuda()
    wav = SY.synthetic_ref_wave(300, seed=5, hop=160)                      # 3 s of the 30 s window
    feats = model.features(wav.cuda())
    enc = model.encode_features(feats)
    tokens, cnt = model.generate_from_kv(model.cross_kv(enc), model.prompt_ids("en"), max_new_tokens=4, sync_every=8)
    assert torch.isfinite(feats).all() and torch.isfinite(enc).all() and tokens.shape == (1, 8)
    ref = R.Ref(full, dict(encoder_layers=2, decoder_layers=2, encoder_attention_heads=20, decoder_attention_heads=20))
    w = wav[0].numpy().astype(np.float64)
    f64 = R.log_mel(w, len(w), 3000, R.slaney_filters(128))
    e64 = ref.encoder(f64)
    got = tokens[0].tolist()
    lg = ref.decoder_logits(e64, got[:-1])
    e_feat, e_enc = R.rel_l2(feats[0].cpu().numpy(), f64), R.rel_l2(enc[0].cpu().numpy(), e64)
    print(f"full width: features {e_feat:.2e}, encoder {e_enc:.2e} against float64; tokens {got}")
    for p in range(3, 7):
        l = lg[p].copy()
        l[list(fields["suppress_tokens"])] = -np.inf
        if p == 3:
            l[list(fields["begin_suppress_tokens"])] = -np.inf
        top = np.sort(l)[-2:]
        margin = (top[1] - top[0]) / math.sqrt((l[np.isfinite(l)] ** 2).mean())
        print(f"    step {p - 3}: float64 argmax {int(np.argmax(l))}, device {got[p + 1]}, margin / RMS {margin:.3f}")
        assert margin >= 1e-2 and int(np.argmax(l)) == got[p + 1]
    assert e_feat < GATE and e_enc < GATE
