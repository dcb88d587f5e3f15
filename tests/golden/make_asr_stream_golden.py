"""Generates tests/golden/asr_stream_decode.npz: what the reference's decode methods return when the encoder runs chunk by
chunk (``simulate_streaming=True``, ppg/asr_model.py:281-307 -> ``BaseEncoder.forward_chunk_by_chunk``,
ppg/wenet/transformer/encoder.py:293-355).  It pins ``ConformerPPG.{ctc_greedy_search, ctc_prefix_beam_search,
attention_rescoring}(..., simulate_streaming=True)`` and ``StreamingRecognizer`` (ppg/streaming_asr.py).

Usage (where the reference checkout is at hand; it is never needed to run the tests):
    python tests/golden/make_asr_stream_golden.py <reference checkout>

A REFERENCE BUG this script works round: ``ASRModel._forward_encoder`` passes ``embs=`` to
``encoder.forward_chunk_by_chunk`` (ppg/asr_model.py:293-298), which takes no such argument (encoder.py:293-298), so every
decode method raises ``TypeError`` with ``simulate_streaming=True`` as shipped.  ``drop_embs`` wraps the method so that the
stray keyword is dropped; everything else that runs is the reference's.

The model is ``make_ppg_stream_golden.build_model`` (seed 5151, ``causal=True``, ``use_dynamic_chunk=True``): its encoder is
the one tests/golden/ppg_stream_common.npz holds (asserted), so only the extra tensors are stored here -- ``w/ctc.*`` (the CTC
head x 8, as make_ctc_beam_golden.py does, so that an untrained head decides anything at all) and ``w/decoder.*`` -- rounded
to fp16-representable values BEFORE the reference runs and stored as float16 (exact); ``feats`` likewise.

For (chunk, left) in {(16, -1), (4, 2)}, tags ``c16`` / ``c4``:
    logp_<tag>                          the reference's CTC log-probabilities on the chunk-by-chunk encoder output, f32 [T', V]
    greedy_<tag>                        ctc_greedy_search ids
    ids_/len_/score_<tag>               ctc_prefix_beam_search's n-best at beam 10 (-1 padded)
    resc_w0_/resc_w5_<tag>, resc_score_w0_/w5_<tag>   attention_rescoring's winner and score at ctc_weight 0 and 0.5
Asserted for every stored decision, the feature seed being searched until all hold (pick another range if none does; do not
loosen a rule): the margin rule of tests/ctc_beam_ref.py at factor 100 for the n-best lists; for the greedy ids the same
rule on the per-frame decision, the gap between a frame's two best log-probabilities >= 100 x max(E, 1e-6) with E the
largest fp32 / fp64 difference of the normalised log-probabilities; for the rescoring winners the lead rule of
make_ctc_beam_golden.py (lead over the runner-up > 100 x 2e-4 x RMS(decoder logits) x (U + 2))."""
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

import asr_decoder_ref as DR  # noqa: E402
import ctc_beam_ref as BR  # noqa: E402
import make_ppg_stream_golden as PS  # noqa: E402

PAIRS = (("c16", 16, -1), ("c4", 4, 2))
BEAM, V, FRAMES, FACTOR = 10, 40, 165, 100.0


def drop_embs(encoder):
    """``forward_chunk_by_chunk`` without the stray ``embs`` keyword of ``ASRModel._forward_encoder`` (see above)."""
    orig = encoder.forward_chunk_by_chunk
    encoder.forward_chunk_by_chunk = lambda xs, decoding_chunk_size, num_decoding_left_chunks=-1, embs=None: \
        orig(xs, decoding_chunk_size, num_decoding_left_chunks)


def greedy_gap(logp):
    """(smallest gap between a frame's two best log-probabilities, E = largest fp32 / fp64 difference of the normalised rows)."""
    l64, l32 = BR.normalise(logp, np.float64), BR.normalise(logp, np.float32)
    top = np.sort(l64, -1)
    return float((top[:, -1] - top[:, -2]).min()), float(np.abs(l64 - l32).max())


def decode(model, feats, chunk, left):
    """Every stored entry of one (chunk, left) pair, or None when a decision is fragile."""
    lens = torch.tensor([feats.shape[1]])
    kw = dict(decoding_chunk_size=chunk, num_decoding_left_chunks=left, simulate_streaming=True)
    with torch.no_grad():
        greedy, _ = model.ctc_greedy_search(feats, lens, **kw)
        hyps, encoder_out = model._ctc_prefix_beam_search(feats, lens, BEAM, **kw)
        best = model.ctc_prefix_beam_search(feats, lens, BEAM, **kw)
        logp = model.ctc.log_softmax(encoder_out)[0].numpy()
    hyps = [(tuple(int(i) for i in p), float(s)) for p, s in hyps]
    assert tuple(int(i) for i in best[0]) == hyps[0][0]
    mine, delta, E, same = BR.margin(logp, BEAM, normalised=True)
    gap, Eg = greedy_gap(logp)
    print(f"  chunk {chunk} left {left}: T' {len(logp)}, delta {delta:.2e}, E {E:.2e}; greedy gap {gap:.2e}, E {Eg:.2e}")
    if not (same and BR.usable(delta, E, FACTOR) and [p for p, _ in mine] == [p for p, _ in hyps]):
        return None
    if not BR.usable(gap, Eg, FACTOR):
        return None
    ids = [p for p, _ in hyps]
    ys, r_ys, ys_len = DR.inputs(ids, V - 1, V - 1)
    with torch.no_grad():
        out, _ = model.forward_attention_decoder(ys, ys_len, encoder_out, 0.0)
        raw, _, _ = model.decoder(encoder_out.repeat(BEAM, 1, 1), torch.ones(BEAM, 1, encoder_out.shape[1], dtype=torch.bool),
                                  ys, ys_len, r_ys, 0.0)
    rms, U = float(raw.pow(2).mean().sqrt()), ys.shape[1] - 1
    bound = FACTOR * 2e-4 * rms * (U + 2)
    res = dict(logp=logp, greedy=np.asarray(greedy[0], np.int32))
    res["ids"], res["len"], res["score"] = BR.pack(hyps, BEAM, max(1, max(len(p) for p in ids)))
    for tag, cw in (("w0", 0.0), ("w5", 0.5)):
        sc = DR.rescoring_scores(ids, [s for _, s in hyps], out.numpy(), None, V - 1, cw, 0.0)
        win = DR.winner(sc)
        lead = sc[win] - max(v for i, v in enumerate(sc) if i != win)
        with torch.no_grad():
            best_ids, best_score = model.attention_rescoring(feats, lens, BEAM, ctc_weight=cw, **kw)
        assert tuple(int(i) for i in best_ids) == ids[win]
        print(f"  ctc_weight {cw}: winner {win}, lead {lead:.4f}, bound {bound:.4f}")
        if not lead > bound:
            return None
        res[f"resc_{tag}"], res[f"resc_score_{tag}"] = np.asarray(ids[win], np.int32), np.asarray(float(best_score))
    return res


def main(ref_root: str):
    asr, cmvn_mod = PS.load_reference_ppg(ref_root)
    model = PS.build_model(asr, cmvn_mod, True)
    with torch.no_grad():
        model.ctc.ctc_lo.weight.mul_(8.0)
        model.ctc.ctc_lo.bias.mul_(8.0)
        for p in model.parameters():
            p.copy_(p.half().float())
    drop_embs(model.encoder)
    sd = model.state_dict()
    common = np.load(os.path.join(HERE, "ppg_stream_common.npz"))
    shared = [k[2:] for k in common.files if k.startswith("w/")]
    assert shared and all(np.array_equal(sd[k].numpy(), common["w/" + k].astype(np.float32)) for k in shared), \
        "the encoder is not the one of ppg_stream_common.npz"
    out = {"w/" + k: v.half().numpy() for k, v in sd.items() if k.startswith(("ctc.", "decoder."))}
    assert all(torch.equal(sd[k[2:]], torch.from_numpy(v).float()) for k, v in out.items())
    for seed in range(7001, 7401):
        print(f"feature seed {seed}")
        feats = (4.0 * torch.randn(1, FRAMES, 80, generator=torch.Generator().manual_seed(seed)) + 8.0).half().float()
        got = {}
        for tag, chunk, left in PAIRS:
            res = decode(model, feats, chunk, left)
            if res is None:
                break
            got.update({f"{k}_{tag}": v for k, v in res.items()})
        else:
            out.update(got, feats=feats.half().numpy(), seed=np.asarray(seed))
            path = os.path.join(HERE, "asr_stream_decode.npz")
            np.savez_compressed(path, **out)
            print("wrote", path, os.path.getsize(path) // 1024, "KiB")
            assert os.path.getsize(path) < (1 << 20)
            return
    raise SystemExit("no feature seed satisfies the rules")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
