"""CPU side of the attention decoder's beam search: the restatement (tests/asr_attention_ref.py) reproduces every case of
tests/golden/asr_attention.npz -- the reference's own ``recognize`` outputs --, the new entry points are declared and
exported, and the host-side refusals of ``ConformerPPG.recognize``."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import asr_attention_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
NEW = ("f5e_attn_decode_f32", "f5e_beam_step")
KINDS = {"tf": "decoder.", "bi": "decoder.left_decoder."}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "asr_attention.npz"))


def test_fixture_is_small_and_complete(gold):
    assert os.path.getsize(os.path.join(GOLD, "asr_attention.npz")) < (1 << 20)
    assert int(gold["n_loops"]) == len(AR.LOOP_CASES) == 7
    shapes = [c[:4] for c in AR.LOOP_CASES[:5]]
    assert shapes == [(1, 12, 9, 1), (1, 20, 12, 4), (2, 30, 40, 10), (3, 25, 70, 16), (1, 6, 5, 5)]
    for tag in KINDS:
        assert gold[f"{tag}/lens"].tolist() == [61, 45] and gold[f"{tag}/feats"].shape == (2, 61, 80)


@pytest.mark.parametrize("case", range(len(AR.LOOP_CASES)))
def test_restatement_reproduces_the_loop_cases(gold, case):
    B, maxlen, V, beam, plant = AR.LOOP_CASES[case]
    table = AR.loop_table(maxlen, V, int(gold[f"loop{case}_seed"]), plant)
    res, delta, E, same = AR.margin(lambda dt: AR.table_fn(table.astype(dt)), B, beam, maxlen, V - 1, V - 1)
    assert same and AR.usable(delta, E, 100.0), f"delta {delta:.3e}, E {E:.3e}"
    hyps, scores = AR.best(res, B, beam)
    assert np.array_equal(hyps, gold[f"loop{case}_best"])                     # the reference's own output
    assert np.allclose(scores, gold[f"loop{case}_best_score"], rtol=1e-6, atol=0)
    assert np.array_equal(res["hyp"], gold[f"loop{case}_hyp"]) and np.array_equal(res["anc"], gold[f"loop{case}_anc"])
    assert np.array_equal(res["done_at"], gold[f"loop{case}_done_at"])
    assert np.allclose(res["score"], gold[f"loop{case}_score"], rtol=1e-12, atol=0, equal_nan=True)
    if plant == "early":
        assert (res["done_at"] >= 0).all() and res["steps"] == res["done_at"].max() + 1 <= maxlen // 2
    if plant == "never":
        assert (res["done_at"] < 0).all() and res["steps"] == maxlen
    # running on after the early stop appends eos at score + 0 and keeps the order: what a device loop that looks only
    # every few steps does
    full = AR.search(AR.table_fn(table.astype(np.float64)), B, beam, maxlen, V - 1, V - 1, early_stop=False)
    n = res["steps"]
    assert np.array_equal(full["hyp"][:, :n + 1], res["hyp"]) and (full["hyp"][:, n + 1:] == V - 1).all()
    assert np.array_equal(full["score"], res["score"]) and np.array_equal(full["done_at"], res["done_at"])


def test_beam_step_ties_go_to_the_lower_class_and_the_lower_parent():
    logp = np.log(np.full((2, 4), 0.25))
    score, hyp, anc, alive, gaps = AR.beam_step(logp, np.zeros(2), np.full((2, 3), 3), np.zeros((2, 3), np.int64), 0, 2, 3)
    assert hyp[:, 1].tolist() == [0, 1] and anc[:, 0].tolist() == [0, 0] and alive.tolist() == [2] and min(gaps) == 0.0


@pytest.mark.parametrize("tag", list(KINDS))
def test_restatement_reproduces_the_model_cases_from_the_stored_weights(gold, tag):
    """The encoder output comes from the PPG oracle's conformer; the stored beams and the reference's best hypotheses follow
    from it and the stored decoder weights."""
    from oracle import f5e_ppg_oracle as PO
    base = np.load(os.path.join(GOLD, "ppg_conformer.npz"))
    sd = {k[2:]: torch.from_numpy(base[k]) for k in base.files if k.startswith("w/encoder.")}
    sd.update({k[len(tag) + 3:]: torch.from_numpy(gold[k].astype(np.float32)) for k in gold.files if k.startswith(f"{tag}/w/")})
    with torch.no_grad():
        enc, masks = PO.conformer_encoder(sd, torch.from_numpy(gold[f"{tag}/feats"]), torch.from_numpy(gold[f"{tag}/lens"]))
    enc, n = enc.numpy(), masks.squeeze(1).sum(1).numpy()
    for beam in (10, 4):
        mem_len = None if int(n.min()) == enc.shape[1] else n
        for reorder, name in ((False, "stale"), (True, "reorder")):
            r = AR.search(AR.CachedDecoder(sd, KINDS[tag], enc, mem_len, 4, beam, enc.shape[1], torch.float64, reorder), 2, beam,
                          enc.shape[1], 39, 39)
            assert np.array_equal(r["hyp"], gold[f"{tag}/b{beam}/{name}_hyp"])
            assert np.allclose(r["score"], gold[f"{tag}/b{beam}/{name}_score"], rtol=1e-5, atol=0)
            if not reorder:
                hyps, scores = AR.best(r, 2, beam)
                assert np.array_equal(hyps, gold[f"{tag}/b{beam}/best"])
                assert np.allclose(scores, gold[f"{tag}/b{beam}/best_score"], rtol=1e-5, atol=0)


def test_stale_and_reordered_caches_differ_and_rows_finish_at_different_steps(gold):
    differ = ragged = False
    for tag in KINDS:
        for beam in (10, 4):
            s, r = gold[f"{tag}/b{beam}/stale_hyp"], gold[f"{tag}/b{beam}/reorder_hyp"]
            differ |= s.shape != r.shape or not np.array_equal(s, r)
            ragged |= len({int((row[1:] == 39).argmax()) for row in s if (row[1:] == 39).any()}) > 1
    assert differ and ragged


def test_new_functions_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    from f5e_tts_amd import _C
    for name in NEW:
        assert re.search(r"F5E_API int " + name + r"\(", header), name
        assert name in _C.SIGNATURES
    # argument counts of the ctypes signatures match the declarations
    for name in NEW:
        decl = re.search(r"F5E_API int " + name + r"\((.*?)\);", header, re.S).group(1)
        assert len(decl.split(",")) == len(_C.SIGNATURES[name]), name
    assert re.search(r"#define F5E_ABI_VERSION 2\b", header) and _C.ABI_VERSION == 2
    lib = os.path.join(ROOT, "f5e-tts_amd", "libf5e_hip.so")
    if os.path.exists(lib):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(r" T " + name + r"$", syms, re.M), f"{name} is not exported"
    mk = open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "Makefile")).read()
    assert "attn_decode.hip" in mk
    emap = open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "exports.map")).read()
    assert "f5e_*" in emap or all(n in emap for n in NEW)


def test_recognize_refuses_a_model_without_decoder_and_a_bad_beam():
    from f5e_tts_amd._C import F5EError
    from f5e_tts_amd.ppg.ppg_model import ConformerPPG
    feats, lens = torch.zeros(1, 20, 80), torch.tensor([20])
    with pytest.raises(F5EError, match="attention decoder"):
        ConformerPPG(80, 40, 64, 4, 128, 2, 15, ctc=True).recognize(feats, lens, 4)
    m = ConformerPPG(80, 40, 64, 4, 128, 2, 15, decoder="transformer",
                     decoder_conf=dict(attention_heads=4, linear_units=64, num_blocks=2))
    for bad in (0, 17, 41):
        with pytest.raises(F5EError, match="beam_size"):
            m.recognize(feats, lens, bad)
    with pytest.raises(F5EError, match="sync_every"):
        m.recognize(feats, lens, 4, sync_every=0)


def test_decode_modes_are_unchanged():
    from f5e_tts_amd.ppg.ctc_align import DECODE_MODES, CTCAligner
    assert DECODE_MODES == ("ctc_greedy_search", "ctc_prefix_beam_search", "attention_rescoring")
    assert callable(CTCAligner.recognize)
