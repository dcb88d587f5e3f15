"""Generates tests/golden/ctc_beam.npz from the reference's own ``ASRModel._ctc_prefix_beam_search`` (ppg/asr_model.py:461-546).
It pins tests/ctc_beam_ref.py, csrc/ctc_beam.hip and ``ConformerPPG.ctc_prefix_beam_search``.

Usage (build container only; the reference never travels to the GPU box):
    python tests/golden/make_ctc_beam_golden.py <checkout of the reference>

PLANTED cases: ``ctc_ref.planted`` logits (unit-variance noise plus a boost on a seeded random valid alignment) times
boost / 4, log-softmaxed, handed to the reference's loop by replacing ``_forward_encoder`` and ``ctc.log_softmax`` of a tiny
model instance -- the loop itself is the reference's.  Stored per case: ``logp_<i>`` f32 [T, V], ``beam_<i>``, the n-best as
``ids_<i>`` i32 [K, Lmax] (-1 padded), ``len_<i>``, ``score_<i>`` f64.

MODEL case: the tiny ASR model of ctc_asr.npz (make_ctc_golden.make_asr: same seeds, CTC head x 8; its weights, features and
log-probabilities are already stored there), utterance 0, beam 10: ``asr_ids``, ``asr_len``,
``asr_score``.

asr_decoder_transformer.npz / asr_decoder_bitransformer.npz: the same tiny model (encoder weights = ppg_conformer.npz, asserted)
built with ``decoder: transformer`` resp. ``bitransformer`` (r_num_blocks 1, reverse_weight 0.3), the CTC head x 8 as above.
Stored: the reference's state_dict key list (``keys``), every tensor outside ``encoder.*`` (``w/``: decoder, CTC head, linear, ce), ``feats`` / ``lens``
(two utterances, the second shorter), and for utterance 0 at batch 1 the reference's ``encoder_out``, ``logp``, n-best at
beam 10 (``ids``, ``len``, ``score``), ``decoder_out`` / ``r_decoder_out`` as log-softmax (``forward_attention_decoder``), the
per-hypothesis rescoring scores at ctc_weight 0 and 0.5 (``scores_w0``, ``scores_w5``: the reference's double loop on those
outputs, whose winner and best score are asserted equal to what ``attention_rescoring`` itself returns) and the winners.
Asserted besides the margin rule (factor 100): the winner's lead over the runner-up exceeds 100 x 2e-4 x RMS(decoder
logits) x (U + 2) at both weights, 2e-4 being the relative-L2 gate tests/test_ppg_gpu.py puts on this encoder family.  The
feature seed is searched until both hold.

Asserted for every stored case (tests/ctc_beam_ref.py, "the margin rule"): the restatement's fp64 run equals the reference's
list exactly and its scores to 1e-9 relative, its fp32 run gives the same list, and delta >= 20 x max(E, 1e-6) -- factor 100
for the model case, whose scores the device recomputes through the encoder.  If a seed fails, pick another; do not loosen the
rule."""
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

import ctc_beam_ref as BR  # noqa: E402
import ctc_ref as R  # noqa: E402

# (T, L, V, K, boost, seed)
PLANTED = [
    (40, 7, 12, 4, 6.0, 8101),
    (90, 20, 41, 10, 8.0, 8102),
    (70, 30, 20, 8, 8.0, 8103),
    (130, 30, 70, 16, 8.0, 8104),
    (1100, 300, 12, 4, 8.0, 8105),
    (1, 1, 9, 5, 6.0, 8106),
]
ASR_BEAM = 10


def planted_logits(T, L, V, boost, seed):
    labels = np.random.default_rng(seed + 50).integers(1, V, size=L)
    return (R.planted(T, labels, V, seed, boost=boost) * np.float32(boost / 4.0)).astype(np.float32)


def tiny_model(ref_root):
    import make_ppg_stream_golden as PS
    asr, _ = PS.load_reference_ppg(ref_root)
    cfg = dict(cmvn_file=None, is_json_cmvn=True, input_dim=80, output_dim=40, encoder="conformer", decoder="transformer",
               encoder_conf=dict(output_size=64, attention_heads=4, linear_units=128, num_blocks=2),
               decoder_conf=dict(attention_heads=4, linear_units=64, num_blocks=1),
               model_conf=dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False, sv_conf=dict(use_sv=False)))
    torch.manual_seed(1)
    return asr.init_asr_model(cfg).eval()


def ref_search(model, logp, beam):
    """The reference's loop on given log-probabilities f32 [T, V]."""
    lp = torch.from_numpy(np.asarray(logp, np.float32))[None]
    model._forward_encoder = lambda *a, **k: (lp, torch.ones(1, 1, lp.shape[1], dtype=torch.bool))
    model.ctc.log_softmax = lambda x: x
    try:
        with torch.no_grad():
            hyps, _ = model._ctc_prefix_beam_search(torch.zeros(1, 4, 80), torch.tensor([4]), beam)
    finally:
        del model._forward_encoder, model.ctc.log_softmax
    return [(tuple(int(i) for i in p), float(s)) for p, s in hyps]


def check_case(name, logp, beam, want, factor):
    mine, delta, E, same = BR.margin(logp, beam, normalised=True)
    assert [p for p, _ in mine] == [p for p, _ in want], f"{name}: the restatement's list differs from the reference's"
    rel = max(abs(a[1] - b[1]) / max(abs(b[1]), 1e-30) for a, b in zip(mine, want))
    assert rel < 1e-9, f"{name}: scores differ from the reference by {rel:.2e} relative"
    assert same, f"{name}: the fp32 run gives another list: new seed"
    print(f"{name}: delta {delta:.3e}, E {E:.3e}, need {factor * max(E, 1e-6):.3e}, best {want[0][1]:.4f} len {len(want[0][0])}")
    assert BR.usable(delta, E, factor), f"{name}: margin rule fails: new seed"


def decoder_model(ref_root, kind):
    """make_ctc_golden.make_asr's model (same seeds: the encoder is the one of ppg_conformer.npz) with the decoder ``kind``."""
    import make_ppg_stream_golden as PS
    asr, cmvn_mod = PS.load_reference_ppg(ref_root)
    dec = dict(attention_heads=4, linear_units=64, num_blocks=1)
    model_conf = dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False, sv_conf=dict(use_sv=False))
    if kind == "bitransformer":
        dec["r_num_blocks"], model_conf["reverse_weight"] = 1, 0.3
    cfg = dict(cmvn_file=None, is_json_cmvn=True, input_dim=80, output_dim=40, encoder="conformer", decoder=kind,
               encoder_conf=dict(output_size=64, attention_heads=4, linear_units=128, num_blocks=2), decoder_conf=dec,
               model_conf=model_conf)
    torch.manual_seed(4242)
    model = asr.init_asr_model(cfg)
    g = torch.Generator().manual_seed(4243)
    model.encoder.global_cmvn = cmvn_mod.GlobalCMVN(torch.randn(80, generator=g), 0.5 + torch.rand(80, generator=g))
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.ndim == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        for name, b in model.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.1 * torch.randn(b.shape, generator=g))
            if name.endswith("running_var"):
                b.copy_(1.0 + 0.2 * torch.rand(b.shape, generator=g))
        model.ctc.ctc_lo.weight.mul_(8.0)
        model.ctc.ctc_lo.bias.mul_(8.0)
    # the seeded draws above depend on how many parameters precede a tensor (the batch-norm statistics come after the
    # decoder's): the encoder is SET to the stored one, so that both decoder fixtures share ppg_conformer.npz's encoder
    base = np.load(os.path.join(HERE, "ppg_conformer.npz"))
    model.load_state_dict({k[2:]: torch.from_numpy(base[k]) for k in base.files if k.startswith("w/encoder.")}, strict=False)
    return model.eval()


def make_decoder(ref_root, kind, rw):
    import asr_decoder_ref as DR
    model = decoder_model(ref_root, kind)
    sd = model.state_dict()
    base = np.load(os.path.join(HERE, "ppg_conformer.npz"))
    shared = [k[2:] for k in base.files if k.startswith("w/encoder.")]
    assert shared and all(np.array_equal(sd[k].numpy(), base["w/" + k]) for k in shared), "the encoder is not ppg_conformer's"
    V, K = 40, ASR_BEAM
    for seed in range(6001, 6101):
        g = torch.Generator().manual_seed(seed)
        feats = 4.0 * torch.randn(2, 101, 80, generator=g) + 8.0
        lens = torch.tensor([101, 77])
        feats[1, 77:] = 0.0
        f0, l0 = feats[:1], lens[:1]
        with torch.no_grad():
            hyps, encoder_out = model._ctc_prefix_beam_search(f0, l0, K)
            logp = model.ctc.log_softmax(encoder_out)[0].numpy()
        hyps = [(tuple(int(i) for i in p), float(s)) for p, s in hyps]
        mine, delta, E, same = BR.margin(logp, K, normalised=True)
        if not (same and BR.usable(delta, E, 100.0) and [p for p, _ in mine] == [p for p, _ in hyps]):
            print(f"{kind}: feature seed {seed}: margin rule fails (delta {delta:.2e}, E {E:.2e})")
            continue
        ids = [p for p, _ in hyps]
        ys, r_ys, ys_len = DR.inputs(ids, V - 1, V - 1)
        with torch.no_grad():
            out, r_out = model.forward_attention_decoder(ys, ys_len, encoder_out, rw)
            raw, _, _ = model.decoder(encoder_out.repeat(K, 1, 1), torch.ones(K, 1, encoder_out.shape[1], dtype=torch.bool),
                                      ys, ys_len, r_ys, rw)
        rms = float(raw.pow(2).mean().sqrt())
        U = ys.shape[1] - 1
        bound = 100 * 2e-4 * rms * (U + 2)
        ok, res = True, {}
        for tag, cw in (("w0", 0.0), ("w5", 0.5)):
            sc = DR.rescoring_scores(ids, [s for _, s in hyps], out.numpy(), r_out.numpy() if rw > 0 else None, V - 1, cw, rw)
            win = DR.winner(sc)
            lead = sc[win] - max(v for i, v in enumerate(sc) if i != win)
            with torch.no_grad():
                best_ids, best = model.attention_rescoring(f0, l0, K, ctc_weight=cw, reverse_weight=rw)
            # the reference adds np.float32 terms to a Python float: double precision before NumPy 2, single since; the
            # restatement sums in double -> equal within the fp32 rounding of U + 2 terms of the sum's size
            assert tuple(int(i) for i in best_ids) == ids[win]
            assert abs(float(best) - sc[win]) <= (U + 2) * 2.0 ** -24 * abs(sc[win]), (best, sc[win])
            print(f"{kind}: seed {seed} ctc_weight {cw}: winner {win}, lead {lead:.4f}, bound {bound:.4f} (RMS {rms:.3f}, U {U})")
            ok &= lead > bound
            res[f"scores_{tag}"], res[f"winner_{tag}"] = np.asarray(sc), np.asarray(win)
        if not ok:
            continue
        # the restatement equals the reference's decoder outputs
        pre = "decoder." if kind == "transformer" else "decoder.left_decoder."
        mine_out = torch.log_softmax(DR.decoder_forward(sd, pre, encoder_out, ys, ys_len, 4), -1)
        assert float((mine_out - out).abs().max()) < 2e-5
        out_d = {"w/" + k: v.numpy() for k, v in sd.items() if not k.startswith("encoder.")}
        out_d["keys"] = np.asarray(list(sd.keys()))
        L = max(1, max(len(p) for p in ids))
        out_d["ids"], out_d["len"], out_d["score"] = BR.pack(hyps, K, L)
        out_d.update(feats=feats.numpy(), lens=lens.numpy(), encoder_out=encoder_out.numpy(), logp=logp,
                     decoder_out=out.numpy(), reverse_weight=np.asarray(rw), **res)
        if rw > 0:
            out_d["r_decoder_out"] = r_out.numpy()
        print(f"{kind}: delta {delta:.3e}, E {E:.3e}, {len(sd)} state_dict keys")
        return out_d
    raise SystemExit(f"{kind}: no feature seed satisfies the rules")


def main(ref_root: str):
    model = tiny_model(ref_root)
    out = {"n_cases": np.asarray(len(PLANTED))}
    for i, (T, L, V, K, boost, seed) in enumerate(PLANTED):
        logp = R.log_softmax(planted_logits(T, L, V, boost, seed))
        want = ref_search(model, logp, K)
        check_case(f"planted {i} (T={T} L={L} V={V} K={K})", logp, K, want, 20.0)
        out[f"logp_{i}"], out[f"beam_{i}"] = logp, np.asarray(K)
        out[f"ids_{i}"], out[f"len_{i}"], out[f"score_{i}"] = BR.pack(want, K, max(1, max(len(p) for p, _ in want)))
    z = np.load(os.path.join(HERE, "ctc_asr.npz"))
    n = int(z["enc_len"][0])
    logp = z["logp"][0, :n]
    want = ref_search(model, logp, ASR_BEAM)
    check_case(f"asr utterance 0 (T'={n} K={ASR_BEAM})", logp, ASR_BEAM, want, 100.0)
    out["asr_ids"], out["asr_len"], out["asr_score"] = BR.pack(want, ASR_BEAM, max(1, max(len(p) for p, _ in want)))
    for name, arrays in (("ctc_beam.npz", out), ("asr_decoder_transformer.npz", make_decoder(ref_root, "transformer", 0.0)),
                         ("asr_decoder_bitransformer.npz", make_decoder(ref_root, "bitransformer", 0.3))):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **arrays)
        print("wrote", path, os.path.getsize(path) // 1024, "KiB")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
