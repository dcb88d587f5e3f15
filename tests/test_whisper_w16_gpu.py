"""Whisper with 16-bit weights (``Whisper(config, weights="fp16" | "bf16")``, eval/whisper.py, csrc/gemm_f32_w16.hip).

For each 16-bit type every matrix of a tiny model's state dict is rounded to that type on the CPU; the rounded dict is loaded
into the fp32 model A and into model B with ``weights=`` that type.  B holds each matrix once, in 16 bits, and widens it in
registers; A holds the same values in fp32.  Widening is exact and the kernels share their bodies, so B must give A's BITS in
every decode path: every comparison here is ``torch.equal`` (or ``==`` on segments), with no tolerance.

The models: the tiny model of tests/golden/whisper.npz with the alignment heads of whisper_align.npz ("short"), and case (g) of
whisper_long.npz, whose recording takes two windows ("long": timestamp rules, sampling, the seek loop), and case (g) of
whisper_prompt.npz with its own fallback and conditioning ("prompt")."""
import json

import pytest
import torch

import test_whisper_align_cpu as AC
import test_whisper_cpu as WC
import test_whisper_long_cpu as LC
import test_whisper_prompt_cpu as PC
import whisper_long_ref as LR

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
MODES = {"fp16": torch.float16, "bf16": torch.bfloat16}
_dev = {}


def W():
    from f5e_tts_amd.eval import whisper
    return whisper


def source(kind):
    """(config, fp32 state dict) of a tiny model."""
    if kind == "short":
        return AC.align_cfg(), {k: torch.from_numpy(v.copy()) for k, v in WC.gold()["sd"].items()}
    if kind == "prompt":
        return PC.tiny_cfg(), {k: torch.from_numpy(v.copy()) for k, v in LR.case_sd(PC.gold(), PC.case("g")).items()}
    return LC.tiny_cfg(), {k: torch.from_numpy(v.copy()) for k, v in LR.case_sd(LC.gold(), LC.case("g")).items()}


def pair(kind, mode):
    """(A, B) on the device: the fp32 model and the ``mode`` model, both holding the state dict rounded to ``mode``."""
    if (kind, mode) not in _dev:
        cfg, sd = source(kind)
        rounded = {k: (v.to(MODES[mode]).float() if W().is_matrix(k) else v) for k, v in sd.items()}
        # (the fixtures' weights are bf16 values already, so the bf16 rounding changes nothing; the fp16 one does)
        changed = sum(int((rounded[k] != sd[k]).sum()) for k in sd)
        print(f"{kind} {mode}: rounding changed {changed} weights")
        assert changed > 0 or mode == "bf16"
        A, B = W().Whisper(cfg), W().Whisper(cfg, weights=mode)
        for m in (A, B):
            m.load_state_dict({k: v.clone() for k, v in rounded.items()})
            if kind == "short":
                m.set_vocab(json.loads(str(WC.gold()["vocab_json"])), json.loads(str(WC.gold()["added_tokens_json"])))
        _dev[(kind, mode)] = (A.cuda(), B.cuda())
    return _dev[(kind, mode)]


def short_wave(n=40000):
    return torch.from_numpy(WC.gold()["wave_f32"][:n].copy()).cuda()[None]


def long_wave():
    return torch.from_numpy(LC.case_wave(LC.case("g")).copy()).cuda()[None]


def same(a, b):
    """Tuples of tensors (tokens, lengths, times, ...) equal item by item."""
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


modes = pytest.mark.parametrize("mode", tuple(MODES))


@modes
def test_encoder_logits_and_prefill_are_bit_equal(mode):
    A, B = pair("short", mode)
    w = short_wave()
    enc_a, enc_b = A.encode_features(A.features(w)), B.encode_features(B.features(w))
    assert torch.equal(enc_a, enc_b) and torch.isfinite(enc_a).all()
    kv_a, kv_b = A.cross_kv(enc_a), B.cross_kv(enc_b)
    assert all(torch.equal(x, y) for la, lb in zip(kv_a, kv_b) for x, y in zip(la, lb))
    tokens, n = A.generate(w, None, "en")
    k = int(n[0])
    print(f"{mode}: {k} tokens {tokens[0, :k].tolist()}")
    ids = tokens[:, :k].contiguous()
    la, lb = A.decoder_logits(kv_a, ids), B.decoder_logits(kv_b, ids)               # the per-step logits of the greedy decode
    assert torch.equal(la, lb) and torch.isfinite(la).all()
    assert torch.equal(A.decoder_logits(kv_a, ids, one_pass=True), B.decoder_logits(kv_b, ids, one_pass=True))
    # decoder_prefill on a ragged batch of 2: row 1 left-padded by 2 positions
    w2 = torch.cat([short_wave(48000), torch.cat([short_wave(14400), torch.zeros(1, 48000 - 14400).cuda()], 1)], 0)
    ids2 = torch.stack([ids[0, :6], torch.cat([ids[0, :2], ids[0, :4]])]).contiguous()
    begin = torch.tensor([0, 2], dtype=I32).cuda()
    outs = []
    for m in (A, B):
        kv = m.encode(w2, [48000, 14400])
        st = m._dec_state(2, 8, w2.device)
        outs.append((m.decoder_prefill(st, kv, ids2, begin, want=range(6)).clone(),
                     [(kc.clone(), vc.clone()) for kc, vc in st["caches"]]))
    assert torch.equal(outs[0][0], outs[1][0])
    # cache slots at or beyond the prompt are not written and hold whatever the allocation held: compare the filed ones
    assert all(torch.equal(x[:, :6], y[:, :6]) for ca, cb in zip(outs[0][1], outs[1][1]) for x, y in zip(ca, cb))


@modes
def test_generate_modes_are_bit_equal(mode):
    A, B = pair("short", mode)
    w = short_wave()
    assert same(A.generate(w, None, "en"), B.generate(w, None, "en"))
    assert same(A.generate(w, None, "en", beam_size=3), B.generate(w, None, "en", beam_size=3))
    ta, tb = A.generate(w, None, "en", return_token_timestamps=True), B.generate(w, None, "en", return_token_timestamps=True)
    assert len(ta) == 3 and same(ta, tb)
    La, Lb = pair("long", mode)
    lw = long_wave()
    for kw in (dict(return_timestamps=True), dict(temperature=0.4, seed=1), dict(return_timestamps=True, temperature=0.4, seed=1)):
        ga, gb = La.generate(lw, None, "en", **kw), Lb.generate(lw, None, "en", **kw)
        print(f"{mode} {kw}: {ga[0][0, :int(ga[1][0])].tolist()}")
        assert same(ga, gb), kw


@modes
def test_token_timestamps_and_decoder_append_are_bit_equal(mode):
    """The two entry points by name: ``token_timestamps`` on given tokens, and ``decoder_append`` behind a prefilled cache with 3
    new rows (the skinny GEMM) and with 17 (beyond it: the general one)."""
    A, B = pair("short", mode)
    w = short_wave()
    tokens, n = A.generate(w, None, "en")
    assert int(n[0]) >= 21
    outs = []
    for m in (A, B):
        kv = m.encode(w)
        times = m.token_timestamps(kv, tokens, n, 40000 // 160, AC.N0)
        res = [times]
        for U in (3, 17):
            st = m._dec_state(1, 24, w.device)
            m.decoder_prefill(st, kv, tokens[:, :4].contiguous())
            res.append(m.decoder_append(st, kv, tokens[:, 4:4 + U].contiguous(), 4).clone())
            res += [c[:, :4 + U].clone() for pair_ in st["caches"] for c in pair_]
        outs.append(res)
    assert (outs[0][0] != 0).any() and outs[0][1].shape[1] == 3
    assert same(outs[0], outs[1])


@modes
def test_transcribe_long_two_windows_is_equal(mode):
    La, Lb = pair("long", mode)
    lw = long_wave()
    sa = La.transcribe_long(lw, [lw.shape[1]], language="en")
    sb = Lb.transcribe_long(lw, [lw.shape[1]], language="en")
    seeks = sorted({s.seek for s in sa[0]})
    print(f"{mode}: {len(sa[0])} segments, windows at {seeks}")
    assert len(seeks) >= 2, "the case must take two windows"
    assert sa == sb
    # fallback and context: case (g) of the prompt fixture, with the thresholds and the seed it was made with
    Pa, Pb = pair("prompt", mode)
    c = PC.case("g")
    lo, hi = c["waves"][0]
    pw = torch.from_numpy(PC.gold()["wave_f32"][lo:hi].copy()).cuda()[None]
    f = c["fallback"]
    kw = dict(fallback=W().Fallback(tuple(f["temperatures"]), f["compression_ratio_threshold"], f["logprob_threshold"], f["seed"]),
              row_keys=[f["row_key"]], context=PC.context_of(c))
    ta, tb = [], []
    pa = Pa.transcribe_long(pw, [pw.shape[1]], "en", trace=ta, **kw)
    pb = Pb.transcribe_long(pw, [pw.shape[1]], "en", trace=tb, **kw)
    print(f"{mode}: fallback + context: {len(pa[0])} segments")
    assert pa == pb and len(pa[0]) >= 1 and repr(ta) == repr(tb)


@modes
def test_assisted_generation_is_equal_also_with_an_fp32_assistant(mode):
    A, B = pair("short", mode)
    w = short_wave()
    base = A.generate(w, None, "en")
    runs = {}
    for name, main, draft in (("a/a", A, A), ("b/b", B, B), ("b/a", B, A)):        # b/a: the mixed case (fp16: main fp16, draft fp32)
        stats = {}
        out = main.generate(w, None, "en", assistant=draft, num_assistant_tokens=3, stats=stats, assistant_shares_encoder=draft is main)
        runs[name] = (out, stats["assistant"])
        assert same(out, base), name
    print(f"{mode}: {runs['b/b'][1]}")
    assert runs["a/a"][1] == runs["b/b"][1] == runs["b/a"][1]
    # a draft that disagrees: the long decoder's noise is not needed, a draft of other weights is the other tiny model's seed
    other = AC.align_model("b").cuda()
    for main in (A, B):
        stats = {}
        out = main.generate(w, None, "en", assistant=other, num_assistant_tokens=3, stats=stats)
        assert same(out, base)
        runs[id(main)] = stats["assistant"]
    assert runs[id(A)] == runs[id(B)]


@modes
def test_captured_step_is_equal_with_both_gemms(mode):
    A, B = pair("short", mode)
    w = short_wave()
    base = A.generate(w, None, "en")
    for g in ("f32", "skinny"):
        assert same(B.generate(w, None, "en", step_graph=True, step_gemm=g), base), g
        assert same(A.generate(w, None, "en", step_graph=True, step_gemm=g), base), g
    keys = list(B._fold()["step_states"])
    assert {k[3] for k in keys} == {f"f32+{mode}", f"skinny+{mode}"}, keys           # keyed on the weight mode as well
    La, Lb = pair("long", mode)
    lw = long_wave()
    want = La.generate(lw, None, "en", return_timestamps=True, temperature=0.4, seed=1)
    assert same(Lb.generate(lw, None, "en", return_timestamps=True, temperature=0.4, seed=1, step_graph=True, step_gemm="skinny"), want)


@modes
@pytest.mark.parametrize("kind", ("short", "long"))
def test_device_bytes_is_two_bytes_per_matrix_element_and_four_for_the_rest(kind, mode):
    """Stored once, in 16 bits: the figure follows from the config alone."""
    A, B = pair(kind, mode)
    c = B.cfg
    D, V, Le, Ld, Fe, Fd = c.d_model, c.vocab_size, c.encoder_layers, c.decoder_layers, c.encoder_ffn_dim, c.decoder_ffn_dim
    matrices = Le * (4 * D * D + 2 * D * Fe) + Ld * (8 * D * D + 2 * D * Fd) + 3 * c.num_mel_bins * D + 3 * D * D + V * D
    # fp32 parameters: conv biases, both position tables, per layer the q / v / out biases, fc1 / fc2 biases and LayerNorm pairs
    rest = 2 * D + c.max_source_positions * D + c.max_target_positions * D
    rest += Le * (3 * D + Fe + D + 4 * D) + 2 * D
    rest += Ld * (6 * D + Fd + D + 6 * D) + 2 * D
    # beside them: the zero k third / half of every stacked bias, the front-end's tables, the lists of token ids
    rest += (Le + 2 * Ld) * D
    rest += W().hann_window().size + W().dft_twiddle().size + W().mel_filters(c.num_mel_bins).size
    langs = {int(v) for v in c.lang_to_id.values()}
    rest += len(c.suppress_tokens or ()) + len(c.begin_suppress_tokens or ()) + (V - len(langs) if langs else 0)
    rest += len(c.alignment_heads)
    want = 2 * matrices + 4 * rest
    got = B.device_bytes()
    print(f"{kind} {mode}: device_bytes {got} (f32 mode: {A.device_bytes()}); matrices {matrices} elements, rest {rest}")
    assert got == want
    B.generate(short_wave() if kind == "short" else long_wave(), None, "en")         # a decode leaves no weight behind
    assert B.device_bytes() == want
    sd = B.state_dict()                                                              # and the parameters still read as a state dict
    assert all(v.dtype == (MODES[mode] if W().is_matrix(k) else F32) for k, v in sd.items())
    _, src = source(kind)
    k = "model.decoder.layers.0.encoder_attn.v_proj.weight"
    assert torch.equal(sd[k].cpu(), src[k].to(MODES[mode])) and torch.equal(
        sd["model.encoder.conv2.weight"].cpu(), src["model.encoder.conv2.weight"].to(MODES[mode]))


def test_default_construction_takes_the_fp32_launches_only(monkeypatch):
    from f5e_tts_amd import ops
    A, _ = pair("short", "fp16")
    # fresh models: a captured step that an earlier test left behind would run without passing through ``ops``
    default, B = W().Whisper(A.cfg), W().Whisper(A.cfg, weights="fp16")             # ``weights`` absent
    for m in (default, B):
        m.load_state_dict(A.state_dict())
        m.set_vocab(json.loads(str(WC.gold()["vocab_json"])), json.loads(str(WC.gold()["added_tokens_json"])))
    default, B = default.cuda(), B.cuda()
    assert default.weights == "f32" and B.weights == "fp16"
    calls = dict.fromkeys(("gemm_f32", "gemm_f32_skinny", "gemm_f32_w16", "gemm_f32_w16_skinny"), 0)
    for name in calls:
        def wrapped(*a, _n=name, _f=getattr(ops, name), **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, wrapped)
    w = short_wave()

    def run(m):
        for k in calls:
            calls[k] = 0
        out = m.generate(w, None, "en")
        m.generate(w, None, "en", assistant=m, num_assistant_tokens=3, assistant_shares_encoder=True)
        m.generate(w, None, "en", step_graph=True, step_gemm="skinny")
        return out, dict(calls)
    out_d, c_d = run(default)
    out_b, c_b = run(B)
    print(f"default {c_d}; fp16 {c_b}")
    assert c_d["gemm_f32"] > 0 and c_d["gemm_f32_skinny"] > 0 and c_d["gemm_f32_w16"] == 0 and c_d["gemm_f32_w16_skinny"] == 0
    assert c_b["gemm_f32_w16"] == c_d["gemm_f32"] and c_b["gemm_f32_w16_skinny"] == c_d["gemm_f32_skinny"]
    assert c_b["gemm_f32"] == 0 and c_b["gemm_f32_skinny"] == 0
    assert same(out_d, out_b)


def test_load_rounds_a_mismatching_checkpoint_and_refuses_what_the_type_cannot_hold():
    """fp32 values into an fp16 model: rounded to nearest-even, the bits of ``.half()``; 1e5 is refused by name."""
    cfg, sd = source("short")
    m = W().Whisper(cfg, weights="fp16")
    m.load_state_dict(sd)
    k = "model.decoder.layers.0.fc1.weight"
    assert torch.equal(m.state_dict()[k], sd[k].half())
    bad = dict(sd)
    bad[k] = sd[k].clone()
    bad[k][0, 0] = 1.0e5
    with pytest.raises(W()._C.F5EError, match="model.decoder.layers.0.fc1.weight"):
        m.load_state_dict(bad)
    W().Whisper(cfg, weights="bf16").load_state_dict(bad)                            # bf16 holds it
