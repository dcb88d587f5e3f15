"""CTC prefix beam search and attention rescoring, host side: tests/ctc_beam_ref.py and tests/asr_decoder_ref.py equal the
reference's own ``_ctc_prefix_beam_search`` lists, decoder outputs and rescoring winners on the fixtures of
tests/golden/make_ctc_beam_golden.py; the new C-ABI entries are declared, exported, bound and validate their arguments
without a GPU; the wrappers check their operands first; ``ConformerPPG`` keeps its state_dict without a decoder and owns the
reference's keys with one.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import asr_decoder_ref as DR
import ctc_beam_ref as BR
from test_ctc_cpu import on_own_thread

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
KW = dict(input_dim=80, vocab_size=40, output_size=64, attention_heads=4, linear_units=128, num_blocks=2)
DEC = dict(attention_heads=4, linear_units=64, num_blocks=1)


def hyps_of(ids, lens):
    return [tuple(int(v) for v in ids[i, :n]) for i, n in enumerate(lens)]


# ------------------------------------------------------------------ the restatements against the reference's outputs

def test_beam_restatement_equals_every_reference_list():
    z = np.load(os.path.join(GOLD, "ctc_beam.npz"))
    n = int(z["n_cases"])
    assert n >= 6
    cases = [(z[f"logp_{i}"], int(z[f"beam_{i}"]), z[f"ids_{i}"], z[f"len_{i}"], z[f"score_{i}"]) for i in range(n)]
    asr = np.load(os.path.join(GOLD, "ctc_asr.npz"))
    cases.append((asr["logp"][0, :int(asr["enc_len"][0])], 10, z["asr_ids"], z["asr_len"], z["asr_score"]))
    for logp, K, ids, lens, score in cases:
        hyps, delta, E, same = BR.margin(logp, K, normalised=True)             # the reference's arithmetic: logp as stored
        assert [h for h, _ in hyps] == hyps_of(ids, lens)                      # lists: exact
        assert np.allclose([s for _, s in hyps], score, rtol=1e-9, atol=0)
        assert same and BR.usable(delta, E)                                    # the margin rule the generator asserted
        # normalising again (what the kernel does) changes no list
        assert [h for h, _ in BR.search(logp, K)[0]] == hyps_of(ids, lens)
    assert BR.search(np.zeros((0, 5), np.float32), 3)[0] == [(tuple(), 0.0)]
    hyp, n_, sc = BR.pack([((1, 2, 3), -0.5)], 2, 2)
    assert hyp.tolist() == [[1, 2], [-1, -1]] and n_.tolist() == [3, -1] and sc.tolist() == [-0.5, -np.inf]


@pytest.mark.parametrize("kind", ["transformer", "bitransformer"])
def test_decoder_restatement_equals_the_reference_outputs_and_picks_its_winner(kind):
    z = np.load(os.path.join(GOLD, f"asr_decoder_{kind}.npz"))
    rw, V = float(z["reverse_weight"]), 40
    w = {k[2:]: z[k] for k in z.files if k.startswith("w/")}
    hyps = hyps_of(z["ids"], z["len"])
    ys, r_ys, n = DR.inputs(hyps, V - 1, V - 1)
    pre = "decoder." if kind == "transformer" else "decoder.left_decoder."
    logits = DR.decoder_forward(w, pre, z["encoder_out"], ys, n, 4)
    rms = float(logits.pow(2).mean().sqrt())
    out = torch.log_softmax(logits, -1)
    atol = 2e-5 * max(1.0, rms)                       # the atol test_ctc_cpu.py uses for stored log-probabilities
    assert float((out - torch.from_numpy(z["decoder_out"])).abs().max()) < atol
    r_out = None
    if rw > 0:
        r_out = torch.log_softmax(DR.decoder_forward(w, "decoder.right_decoder.", z["encoder_out"], r_ys, n, 4), -1)
        assert float((r_out - torch.from_numpy(z["r_decoder_out"])).abs().max()) < atol
    for tag, cw in (("w0", 0.0), ("w5", 0.5)):
        sc = DR.rescoring_scores(hyps, z["score"].tolist(), out, r_out, V - 1, cw, rw)
        assert DR.winner(sc) == int(z[f"winner_{tag}"])
        assert np.allclose(sc, z[f"scores_{tag}"], rtol=0, atol=(ys.shape[1] + 1) * atol)
    # the model-side builder of the decoder inputs equals the restatement's
    from f5e_tts_amd.ppg.ppg_model import rescoring_inputs
    a, b, c, tg, r_tg = rescoring_inputs(hyps, V - 1, V - 1, rows=len(hyps) + 1)
    assert np.array_equal(a[:-1], ys.numpy()) and np.array_equal(b[:-1], r_ys.numpy()) and np.array_equal(c[:-1], n.numpy())
    assert a[-1].tolist() == [V - 1] * ys.shape[1] and c[-1] == 1 and (tg[-1] == -1).all()
    for i, h in enumerate(hyps):
        assert tg[i, :len(h) + 1].tolist() == list(h) + [V - 1] and (tg[i, len(h) + 1:] == -1).all()
        assert r_tg[i, :len(h) + 1].tolist() == list(h[::-1]) + [V - 1]


# ------------------------------------------------------------------ the C ABI

ENTRIES = (("f5e_ctc_beam", 16), ("f5e_ctc_beam_workspace_bytes", 4), ("f5e_mha_f32", 17), ("f5e_token_logp", 7),
           ("f5e_log_softmax_rows", 7))


def test_new_entries_are_declared_exported_and_bound():
    from f5e_tts_amd import _C
    text = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    lib = _C.lib()
    for name, arity in ENTRIES:
        m = re.search(r"F5E_API int " + name + r"\((.*?)\);", text, flags=re.S)
        assert m, f"{name} is not declared in f5e_abi.h"
        assert len(m.group(1).split(",")) == arity == len(_C.SIGNATURES[name])
        assert hasattr(lib, name)
    assert lib.f5e_abi_version() == _C.ABI_VERSION == 2
    assert "ctc_beam.hip" in open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "Makefile")).read()


def test_workspace_query_and_every_argument_check_without_launching():
    on_own_thread(_argument_checks)


def _argument_checks():
    from f5e_tts_amd import _C, ops
    lib = _C.lib()
    assert ops.ctc_beam_workspace_bytes(1, 250, 10) == 250 * 10 * 16
    assert ops.ctc_beam_workspace_bytes(16, 750, 16) == 16 * 750 * 16 * 16
    n = C.c_ulonglong()
    assert lib.f5e_ctc_beam_workspace_bytes(1, 16385, 10, C.byref(n)) == -1 and b"16384" in lib.f5e_last_error()
    assert lib.f5e_ctc_beam_workspace_bytes(1, 16, 17, C.byref(n)) == -1 and b"beam" in lib.f5e_last_error()
    assert lib.f5e_ctc_beam_workspace_bytes(1, 16, 0, C.byref(n)) == -1
    assert lib.f5e_ctc_beam_workspace_bytes(1, 16, 4, None) == -1
    p, big = C.c_void_p(8), 10 ** 9

    def beam(scores=p, bs=0, ld=50, t=p, blank=0, K=10, hyp=p, ldh=100, hl=p, sc=p, ws=p, wsb=big, B=1, T=100, V=50):
        return lib.f5e_ctc_beam(None, scores, bs, ld, t, blank, K, hyp, ldh, hl, sc, ws, wsb, B, T, V)

    for bad in (dict(scores=None), dict(t=None), dict(hyp=None), dict(hl=None), dict(sc=None), dict(ws=None)):
        assert beam(**bad) == -1 and b"null" in lib.f5e_last_error()
    for K in (0, 17, -1):
        assert beam(K=K) == -1 and b"beam" in lib.f5e_last_error()
    assert beam(K=12, V=11, ld=11) == -1 and b"beam <= V" in lib.f5e_last_error()
    assert beam(V=1, ld=1, K=1) == -1 and b"V >= 2" in lib.f5e_last_error()
    assert beam(blank=50) == -1 and beam(blank=-1) == -1
    assert beam(ld=49) == -1 and b"ld" in lib.f5e_last_error()
    assert beam(ldh=0) == -1
    assert beam(B=2, bs=99 * 50 + 49) == -1 and b"batch_stride" in lib.f5e_last_error()       # overlapping batch stride
    assert beam(wsb=100 * 10 * 16 - 1) == -1 and b"workspace" in lib.f5e_last_error()         # too small
    assert beam(ws=C.c_void_p(12)) == -1 and b"aligned" in lib.f5e_last_error()               # misaligned
    assert beam(T=16385) == -1 and b"16384" in lib.f5e_last_error()
    assert beam(T=0) == -1 and beam(B=0) == -1

    q = C.c_void_p(16)

    def mha(q_=q, ldq=64, k=q, ldk=64, v=q, ldv=64, out=q, ldo=64, B=1, Tq=8, Tk=8, H=4, dk=16, causal=0):
        return lib.f5e_mha_f32(None, q_, ldq, k, ldk, v, ldv, out, ldo, None, B, Tq, Tk, H, dk, causal, 0.25)

    for bad in (dict(q_=None), dict(k=None), dict(v=None), dict(out=None)):
        assert mha(**bad) == -1 and b"null" in lib.f5e_last_error()
    assert mha(dk=24) == -1 and b"head dim" in lib.f5e_last_error()
    assert mha(causal=1, Tq=8, Tk=9) == -1 and b"causal" in lib.f5e_last_error()
    assert mha(ldq=63) == -1 and mha(ldk=60) == -1 and mha(ldv=63) == -1 and mha(ldo=66) == -1
    assert mha(q_=C.c_void_p(20)) == -1 and b"aligned" in lib.f5e_last_error()
    assert mha(Tq=0) == -1 and mha(Tk=0) == -1 and mha(B=0) == -1 and mha(H=0) == -1

    def logp(x=p, ld=40, t=p, out=p, rows=5, V=40):
        return lib.f5e_token_logp(None, x, ld, t, out, rows, V)

    for bad in (dict(x=None), dict(t=None), dict(out=None)):
        assert logp(**bad) == -1 and b"null" in lib.f5e_last_error()
    assert logp(ld=39) == -1 and logp(rows=0) == -1 and logp(V=0, ld=0) == -1
    assert lib.f5e_log_softmax_rows(None, None, 40, p, 40, 5, 40) == -1 and b"null" in lib.f5e_last_error()
    assert lib.f5e_log_softmax_rows(None, p, 39, p, 40, 5, 40) == -1 and lib.f5e_log_softmax_rows(None, p, 40, p, 39, 5, 40) == -1
    assert lib.f5e_log_softmax_rows(None, p, 40, p, 40, 0, 40) == -1


def test_wrappers_check_their_tensors_before_anything_else():
    from f5e_tts_amd import _C, ops
    i32 = torch.int32
    t = torch.tensor([8], dtype=i32)
    for scores in (torch.zeros(1, 8, 5), torch.zeros(8, 5), torch.zeros(1, 8, 5, dtype=torch.float64),
                   torch.zeros(1, 8, 10)[:, :, ::2], torch.empty(1, 8, 5, device="meta")):
        with pytest.raises(_C.F5EError, match="ctc_beam_search: scores must be an f32 GPU tensor"):
            ops.ctc_beam_search(scores, t, 4)
    x = torch.zeros(8, 16)
    with pytest.raises(_C.F5EError, match="mha_f32: q must live on the GPU"):
        ops.mha_f32(x, x, x, 1, 1.0)
    with pytest.raises(_C.F5EError, match="mha_f32: inconsistent shapes"):
        ops.mha_f32(x, torch.zeros(8, 12), x, 1, 1.0)
    with pytest.raises(_C.F5EError, match="mha_f32: causal needs Tq == Tk"):
        ops.mha_f32(x, torch.zeros(4, 16), torch.zeros(4, 16), 1, 1.0, causal=True)
    with pytest.raises(_C.F5EError, match="mha_f32: inconsistent shapes"):
        ops.mha_f32(x, x, x, 1, 1.0, B=3)
    with pytest.raises(_C.F5EError, match="token_logp: logits must be an f32 GPU tensor"):
        ops.token_logp(x, torch.zeros(8, dtype=i32))
    with pytest.raises(_C.F5EError, match="log_softmax_rows: x must be an f32 GPU tensor"):
        ops.log_softmax_rows(x)


# ------------------------------------------------------------------ the model mirror

def test_state_dict_is_unchanged_without_a_decoder_and_holds_the_reference_keys_with_one():
    from f5e_tts_amd import _C
    from f5e_tts_amd.ppg.ppg_model import ConformerPPG
    z = np.load(os.path.join(GOLD, "ppg_conformer.npz"))
    fixture = {k[2:] for k in z.files if k.startswith("w/") and not k.startswith("w/encoder.global_cmvn")}
    plain, with_ctc = ConformerPPG(**KW), ConformerPPG(**KW, ctc=True)
    assert {k for k in plain.state_dict() if "concat_linear" not in k} == fixture            # as before this feature
    assert [k for k in with_ctc.state_dict() if k not in plain.state_dict()] == ["ctc.ctc_lo.weight", "ctc.ctc_lo.bias"]
    assert plain.decoder_type is None and not hasattr(plain, "decoder")
    cmvn = (torch.zeros(80), torch.ones(80))
    for kind, conf in (("transformer", DEC), ("bitransformer", dict(DEC, r_num_blocks=1))):
        ref_keys = [str(k) for k in np.load(os.path.join(GOLD, f"asr_decoder_{kind}.npz"))["keys"]]
        m = ConformerPPG(**KW, global_cmvn=cmvn, ctc=True, decoder=kind, decoder_conf=conf)
        mine = set(m.state_dict())
        # the reference's ASR model: everything here plus the speaker-embedding input layer, which use_emb False never runs
        assert mine == {k for k in ref_keys if not k.startswith("encoder.linear_xs_embs.")}
        assert {k for k in mine if k.startswith("decoder.")} == {k for k in ref_keys if k.startswith("decoder.")}
        assert [k for k in m.state_dict() if not k.startswith("decoder.")] == \
            list(ConformerPPG(**KW, global_cmvn=cmvn, ctc=True).state_dict())
    cfg = dict(input_dim=80, output_dim=40, cmvn_file=None, encoder_conf=dict(output_size=64, linear_units=128, num_blocks=1),
               decoder="transformer", decoder_conf=dict(DEC, dropout_rate=0.1))
    assert list(ConformerPPG.from_config(cfg).state_dict()) == list(ConformerPPG.from_config(cfg, ctc=False, decoder=False).state_dict())
    full = ConformerPPG.from_config(cfg, ctc=True, decoder=True)
    assert "decoder.decoders.0.src_attn.linear_k.weight" in full.state_dict() and full.decoder_heads == 4
    bi = ConformerPPG.from_config(dict(cfg, decoder="bitransformer", decoder_conf=dict(DEC, r_num_blocks=2)), decoder=True)
    assert "decoder.right_decoder.decoders.1.norm3.bias" in bi.state_dict()
    del cfg["decoder"]                                 # init_asr_model's default is bitransformer, which needs r_num_blocks
    with pytest.raises(_C.F5EError, match="r_num_blocks"):
        ConformerPPG.from_config(cfg, decoder=True)


@pytest.mark.parametrize("entry", [dict(concat_after=True), dict(normalize_before=False), dict(input_layer="linear"),
                                   dict(use_output_layer=False), dict(no_such_entry=1)])
def test_an_unsupported_decoder_conf_entry_raises_naming_it(entry):
    from f5e_tts_amd import _C
    from f5e_tts_amd.ppg.ppg_model import ConformerPPG
    with pytest.raises(_C.F5EError, match=next(iter(entry))):
        ConformerPPG(**KW, decoder="transformer", decoder_conf=dict(DEC, **entry))
    with pytest.raises(_C.F5EError, match="unsupported decoder"):
        ConformerPPG(**KW, decoder="lstm")
    with pytest.raises(_C.F5EError, match="attention_heads"):
        ConformerPPG(**KW, decoder="transformer", decoder_conf=dict(DEC, attention_heads=5))


def test_decoding_methods_need_their_halves_and_validate_host_values():
    from f5e_tts_amd import _C
    from f5e_tts_amd.ppg.ppg_model import ConformerPPG, check_beam, check_hyps
    feats, lens = torch.zeros(1, 20, 80), torch.tensor([20])
    plain, with_ctc = ConformerPPG(**KW), ConformerPPG(**KW, ctc=True)
    with pytest.raises(_C.F5EError, match="CTC head"):
        plain.ctc_prefix_beam_search(feats, lens, 4)
    for bad in (0, 17, 41):
        with pytest.raises(_C.F5EError, match="beam_size"):
            with_ctc.ctc_prefix_beam_search(feats, lens, bad)
    assert check_beam(16, 40) == 16 and check_beam(3, 3) == 3
    with pytest.raises(_C.F5EError, match="attention decoder"):
        with_ctc.attention_rescoring(feats, lens, 4)
    with pytest.raises(_C.F5EError, match="attention decoder"):
        with_ctc.forward_attention_decoder(torch.zeros(2, 3, dtype=torch.long), torch.tensor([3, 2]), torch.zeros(1, 9, 64))
    uni = ConformerPPG(**KW, ctc=True, decoder="transformer", decoder_conf=DEC)
    with pytest.raises(_C.F5EError, match="bitransformer"):
        uni.attention_rescoring(feats, lens, 4, reverse_weight=0.3)
    check_hyps([3, 1], 3, 40, [[39, 1, 2], [39, 39, 39]])
    for n in ([0], [4]):
        with pytest.raises(_C.F5EError, match="length"):
            check_hyps(n, 3, 40)
    with pytest.raises(_C.F5EError, match="ids outside"):
        check_hyps([2], 3, 40, [[39, 40, 0]])


def test_transcribe_rejects_an_unknown_mode_and_rescoring_without_a_decoder():
    from f5e_tts_amd import _C
    from f5e_tts_amd.ppg.ctc_align import CTCAligner, DECODE_MODES
    from f5e_tts_amd.ppg.ppg_model import ConformerPPG
    assert DECODE_MODES == ("ctc_greedy_search", "ctc_prefix_beam_search", "attention_rescoring")
    al = CTCAligner(model=ConformerPPG(**KW, ctc=True), symbol_table={"<blank>": 0, "a": 1}, device="cpu")
    wav = torch.zeros(1, 1600)
    with pytest.raises(_C.F5EError, match="unknown mode"):
        al.transcribe(wav, 16000, mode="attention")
    with pytest.raises(_C.F5EError, match="attention decoder"):
        al.transcribe(wav, 16000, mode="attention_rescoring")
