"""Generates tests/golden/asr_attention.npz from the reference's own ``ASRModel.recognize`` (ppg/asr_model.py:309-414).
It pins tests/asr_attention_ref.py, csrc/attn_decode.hip and ``ConformerPPG.recognize``.

Usage (build container only; the reference never travels to the GPU box):
    python tests/golden/make_asr_attention_golden.py <checkout of the reference>

LOOP cases (``asr_attention_ref.LOOP_CASES``): the reference's ``recognize`` with ``_forward_encoder`` and
``decoder.forward_one_step`` of a tiny model instance replaced by a stub that returns log-probabilities from a seeded table
indexed by (step, last token) -- the loop itself is the reference's.  The table is NOT stored (``asr_attention_ref.loop_table``
rebuilds it from ``loop<i>_seed``); stored per case: the reference's ``loop<i>_best`` / ``loop<i>_best_score`` and the
restatement's whole beam ``loop<i>_hyp`` / ``_anc`` / ``_score`` / ``_done_at``, ``_delta``, ``_E``.

MODEL cases: the tiny ASR model of the sibling fixtures (make_ctc_beam_golden.decoder_model's seeds and perturbations; the
encoder is ppg_conformer.npz's, asserted identical) with ``decoder: transformer`` (2 blocks) resp. ``bitransformer`` (3 + 1
blocks).  The output layer is multiplied by 4 and the eos bias raised by 2 resp. 2.5 so that rows finish at different
steps.  Every tensor outside ``encoder.*`` is rounded to fp16 BEFORE the reference runs and stored as fp16, which is exact
(the six decoder blocks would not fit the fixture size limit in fp32).  Two utterances of 61 and 45 frames; beam 10 and 4.
Stored per decoder kind <k> in {tf, bi}: ``<k>/w/<name>`` weights, ``<k>/keys``, ``<k>/feats``, ``<k>/lens``; per beam <n> the reference's
``recognize`` at batch 2 (``<k>/b<n>/best``, ``best_score``) and for each utterance alone (``<k>/b<n>/u<j>_best``,
``u<j>_best_score``), and the restatement's beams at batch 2 in both cache modes (``<k>/b<n>/stale_hyp``, ``stale_score``,
``reorder_hyp``, ``reorder_score``).

Asserted for every stored case: the restatement's fp64 run in stale mode equals the reference's hypotheses exactly and its
scores to 1e-6 relative; its fp32 run gives the same tables; the margin rule delta >= 100 x max(E, 1e-6) (the factor
make_ctc_beam_golden.py uses where the device recomputes through the encoder).  Also: stale and reordered modes give
different best hypotheses in at least one model case; rows finish at different steps in at least one; in reorder mode the
cached restatement equals a cache-free recompute with ``asr_decoder_ref.decoder_forward`` at every step.  The table seed /
feature seed is searched until all hold; do not loosen the rule."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import asr_attention_ref as AR  # noqa: E402
import asr_decoder_ref as DR  # noqa: E402

BEAMS = (10, 4)
FRAMES = (61, 45)
KINDS = (("tf", "transformer", 2, 0, 2.0), ("bi", "bitransformer", 3, 1, 2.5))


def build_model(ref_root, kind, blocks, r_blocks, eos_bias):
    import make_ppg_stream_golden as PS
    asr, cmvn_mod = PS.load_reference_ppg(ref_root)
    dec = dict(attention_heads=4, linear_units=64, num_blocks=blocks)
    model_conf = dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False, sv_conf=dict(use_sv=False))
    if kind == "bitransformer":
        dec["r_num_blocks"], model_conf["reverse_weight"] = r_blocks, 0.3
    cfg = dict(cmvn_file=None, is_json_cmvn=True, input_dim=80, output_dim=40, encoder="conformer", decoder=kind,
               encoder_conf=dict(output_size=64, attention_heads=4, linear_units=128, num_blocks=2), decoder_conf=dec,
               model_conf=model_conf)
    torch.manual_seed(4242)
    model = asr.init_asr_model(cfg)
    g = torch.Generator().manual_seed(4243)
    model.encoder.global_cmvn = cmvn_mod.GlobalCMVN(torch.randn(80, generator=g), 0.5 + torch.rand(80, generator=g))
    left = model.decoder if kind == "transformer" else model.decoder.left_decoder
    with torch.no_grad():
        for _, p in model.named_parameters():
            if p.ndim == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        left.output_layer.weight.mul_(4.0)
        left.output_layer.bias.mul_(4.0)
        left.output_layer.bias[-1] += eos_bias
        for name, p in model.named_parameters():
            if not name.startswith("encoder."):
                p.copy_(p.half().float())
    base = np.load(os.path.join(HERE, "ppg_conformer.npz"))
    enc = {k[2:]: torch.from_numpy(base[k]) for k in base.files if k.startswith("w/encoder.")}
    model.load_state_dict(enc, strict=False)
    sd = model.state_dict()
    assert enc and all(np.array_equal(sd[k].numpy(), v.numpy()) for k, v in enc.items()), "the encoder is not ppg_conformer's"
    return model.eval()


def tiny_model(ref_root):
    import make_ctc_beam_golden as CB
    return CB.tiny_model(ref_root)


def ref_loop(model, table, B, maxlen, beam):
    """The reference's loop on a table of log-probabilities f32 [maxlen, V, V]."""
    V = table.shape[1]
    tab = torch.from_numpy(table)
    old = model.sos, model.eos
    model.sos = model.eos = V - 1
    model._forward_encoder = lambda *a, **k: (torch.zeros(B, maxlen, 4), torch.ones(B, 1, maxlen, dtype=torch.bool))
    model.decoder.forward_one_step = lambda mem, mm, tgt, tm, cache=None: (tab[tgt.shape[1] - 1][tgt[:, -1]], cache)
    try:
        with torch.no_grad():
            hyps, scores = model.recognize(torch.zeros(B, 4, 80), torch.full((B,), 4), beam)
    finally:
        del model._forward_encoder, model.decoder.forward_one_step
        model.sos, model.eos = old
    return hyps.numpy(), scores.numpy()


def same_as_reference(name, res, B, beam, want_hyps, want_scores):
    hyps, scores = AR.best(res, B, beam)
    assert hyps.shape == want_hyps.shape and np.array_equal(hyps, want_hyps), f"{name}: hypotheses differ from the reference's"
    rel = float(np.max(np.abs(scores - want_scores) / np.maximum(np.abs(want_scores), 1e-30)))
    assert rel < 1e-6, f"{name}: scores differ from the reference by {rel:.2e} relative"


def make_loops(ref_root, out):
    model = tiny_model(ref_root)
    for i, (B, maxlen, V, beam, plant) in enumerate(AR.LOOP_CASES):
        for seed in range(9100 + 100 * i, 9200 + 100 * i):
            table = AR.loop_table(maxlen, V, seed, plant)
            res, delta, E, same = AR.margin(lambda dt: AR.table_fn(table.astype(dt)), B, beam, maxlen, V - 1, V - 1)
            if same and AR.usable(delta, E, 100.0):
                break
            print(f"loop {i}: seed {seed}: margin rule fails (delta {delta:.2e}, E {E:.2e})")
        else:
            raise SystemExit(f"loop {i}: no seed satisfies the rules")
        want_hyps, want_scores = ref_loop(model, table, B, maxlen, beam)
        same_as_reference(f"loop {i}", res, B, beam, want_hyps, want_scores)
        if plant == "early":
            assert (res["done_at"] >= 0).all() and res["steps"] <= maxlen // 2, "early: rows do not all finish early"
        if plant == "never":
            assert (res["done_at"] < 0).all() and res["steps"] == maxlen and not (res["hyp"][:, 1:] == V - 1).any()
        print(f"loop {i} (B={B} maxlen={maxlen} V={V} beam={beam} {plant}): seed {seed}, steps {res['steps']}, delta {delta:.3e}, "
              f"E {E:.3e}, done_at {res['done_at'].tolist()}")
        pre = f"loop{i}_"
        out.update({pre + "seed": np.asarray(seed), pre + "best": want_hyps, pre + "best_score": want_scores,
                    pre + "hyp": res["hyp"].astype(np.int32), pre + "anc": res["anc"].astype(np.int32),
                    pre + "score": res["score"], pre + "done_at": res["done_at"].astype(np.int32),
                    pre + "delta": np.asarray(delta), pre + "E": np.asarray(E)})
    out["n_loops"] = np.asarray(len(AR.LOOP_CASES))


def checked_recompute(sd, pre, enc, mem_len, beam, maxlen):
    """A reorder-mode callback that also asserts, at every step, equality with the cache-free full decoder."""
    dec = AR.CachedDecoder(sd, pre, enc, mem_len, 4, beam, maxlen, torch.float64, reorder=True)
    mem = torch.as_tensor(enc).double().repeat_interleave(beam, 0)
    lens = None if mem_len is None else torch.as_tensor(mem_len).repeat_interleave(beam)

    def fn(p, hyp, anc):
        mine = dec.logits(p, hyp, anc)
        full = DR.decoder_forward(sd, pre, mem, hyp[:, :p + 1], np.full(hyp.shape[0], p + 1), 4, mem_len=lens)[:, -1]
        # asr_decoder_ref builds its positional table in fp64, the reference (and the cached restatement) in fp32: 6e-8 per
        # entry, amplified by the x 4 output layer; a wrong ancestor moves logits by O(1)
        assert float((mine - full).abs().max()) < 1e-5, f"step {p}: the reordered cache differs from a full recompute"
        return torch.log_softmax(mine, -1).numpy()
    return fn


def make_model(ref_root, tag, kind, blocks, r_blocks, eos_bias, out):
    model = build_model(ref_root, kind, blocks, r_blocks, eos_bias)
    sd = {k: v for k, v in model.state_dict().items()}
    pre = "decoder." if kind == "transformer" else "decoder.left_decoder."
    V, eos = 40, 39
    lens = torch.tensor(FRAMES)
    for seed in range(7001, 7401):
        g = torch.Generator().manual_seed(seed)
        feats = 4.0 * torch.randn(2, FRAMES[0], 80, generator=g) + 8.0
        feats[1, FRAMES[1]:] = 0.0
        res, ok, flags = {}, True, dict(differ=False, ragged_finish=False)
        for beam in BEAMS:
            runs = [("", feats, lens), ("u0_", feats[:1, :FRAMES[0]], lens[:1]), ("u1_", feats[1:, :FRAMES[1]], lens[1:])]
            for name, f_, l_ in runs:
                with torch.no_grad():
                    want_hyps, want_scores = model.recognize(f_, l_, beam)
                    enc, mask = model._forward_encoder(f_, l_)
                B, maxlen = enc.shape[0], enc.shape[1]
                n = mask.squeeze(1).sum(1)
                mem_len = None if int(n.min()) == maxlen else n.numpy()
                r, delta, E, same = AR.margin(AR.model_fn(sd, pre, enc.numpy(), mem_len, 4, beam, maxlen), B, beam, maxlen, eos, eos)
                if not (same and AR.usable(delta, E, 100.0)):
                    print(f"{kind}: feature seed {seed} beam {beam} {name or 'batch '}: margin rule fails (delta {delta:.2e}, E {E:.2e})")
                    ok = False
                    break
                same_as_reference(f"{kind} seed {seed} beam {beam} {name}", r, B, beam, want_hyps.numpy(), want_scores.numpy())
                res[f"b{beam}/{name}best"], res[f"b{beam}/{name}best_score"] = want_hyps.numpy(), want_scores.numpy()
                if name:
                    continue
                flags["ragged_finish"] |= len({int((r["hyp"][q, 1:] == eos).argmax()) for q in range(B * beam)
                                               if (r["hyp"][q, 1:] == eos).any()}) > 1
                ro, d2, E2, same2 = AR.margin(AR.model_fn(sd, pre, enc.numpy(), mem_len, 4, beam, maxlen, reorder=True), B, beam,
                                              maxlen, eos, eos)
                if not (same2 and AR.usable(d2, E2, 100.0)):
                    print(f"{kind}: feature seed {seed} beam {beam} reorder: margin rule fails (delta {d2:.2e}, E {E2:.2e})")
                    ok = False
                    break
                chk = AR.search(checked_recompute(sd, pre, enc.numpy(), mem_len, beam, maxlen), B, beam, maxlen, eos, eos)
                assert np.array_equal(chk["hyp"], ro["hyp"])
                b_s, b_r = AR.best(r, B, beam)[0], AR.best(ro, B, beam)[0]
                flags["differ"] |= b_s.shape != b_r.shape or not np.array_equal(b_s, b_r)
                print(f"{kind}: seed {seed} beam {beam}: stale delta {delta:.3e} E {E:.3e} steps {r['steps']}; reorder delta "
                      f"{d2:.3e} E {E2:.3e} steps {ro['steps']}; best differ {flags['differ']}")
                res[f"b{beam}/stale_hyp"], res[f"b{beam}/stale_score"] = r["hyp"].astype(np.int32), r["score"]
                res[f"b{beam}/reorder_hyp"], res[f"b{beam}/reorder_score"] = ro["hyp"].astype(np.int32), ro["score"]
            if not ok:
                break
        if not ok:
            continue
        if not (flags["differ"] and flags["ragged_finish"]):
            print(f"{kind}: feature seed {seed}: flags {flags}: next seed")
            continue
        out.update({f"{tag}/{k}": v for k, v in res.items()})
        out.update({f"{tag}/w/{k}": v.numpy().astype(np.float16) for k, v in sd.items() if not k.startswith("encoder.")})
        for k, v in sd.items():
            if not k.startswith("encoder."):
                assert np.array_equal(v.numpy().astype(np.float16).astype(np.float32), v.numpy()), k
        out[f"{tag}/keys"] = np.asarray(list(sd.keys()))
        out[f"{tag}/feats"], out[f"{tag}/lens"], out[f"{tag}/seed"] = feats.numpy(), lens.numpy(), np.asarray(seed)
        return flags
    raise SystemExit(f"{kind}: no feature seed satisfies the rules")


def main(ref_root: str):
    out = {}
    make_loops(ref_root, out)
    for tag, kind, blocks, r_blocks, eos_bias in KINDS:
        make_model(ref_root, tag, kind, blocks, r_blocks, eos_bias, out)
    path = os.path.join(HERE, "asr_attention.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
