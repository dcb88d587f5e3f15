"""Generates tests/golden/ctc_align.npz and tests/golden/ctc_asr.npz from the reference's own CTC code:
``ppg/wenet/utils/ctc_util.py::forced_align`` and ``ppg/asr_model.py::ASRModel.ctc_greedy_search`` (asr_model.py:416-459).
They pin tests/ctc_ref.py, csrc/ctc.hip and ``ConformerPPG(ctc=True)``.

Usage (build container only; the reference never travels to the GPU box):
    python tests/golden/make_ctc_golden.py /root/reference

ctc_align.npz: PLANTED cases -- log-softmax of unit-variance noise plus 4.0 on the class of a seeded random valid alignment
(``ctc_ref.planted``) -- as ``logp_<i>`` f32 [T, V], ``labels_<i>`` and the reference's output ``align_<i>``.  The reference
reads ``log_alpha[t-1, s-1]`` with s-1 = -1 at state 0, i.e. the LAST state; on scores that are not peaky its "best" path may
leave the final blank and run through the labels again.  On planted scores that wrap never wins, and the script asserts
  1. the reference equals tests/ctc_ref.py (CTC proper: state 0 can only stay) on every stored case,
  2. the alignment survives uniform noise of +-1e-3 on the scores (5 draws),
  3. the raw planted logits (before log-softmax) give the same alignment through ctc_ref.
It also prints, for one UNPLANTED case, that the reference equals the literal restatement (``wrap=True``) and not the
correct one: that is the documented deviation, not a fixture.

ctc_asr.npz: the tiny ASR model of ``make_golden.make_ppg_case`` (same config, seeds 4242 / 4243) with the CTC head
(``ctc.ctc_lo.weight`` AND ``.bias``) multiplied by 8 before the reference runs -- with the weight alone the minimum logit gap is
0.025 against a bound of 0.093 and the assertion below fails; with the whole layer scaled it is 0.31 -- its ``ctc.ctc_lo.*`` tensors
(the other weights are those of ppg_conformer.npz, asserted equal), the same features and lengths, and the reference's
``ctc_greedy_search`` hyps and ``scores.values``, ``encoder_out`` and ``ctc.log_softmax(encoder_out)``.  Asserted: every
frame's top-1 / top-2 logit gap exceeds 100 x 2e-4 x RMS(logits) (2e-4 is the relative-L2 gate tests/test_ppg_gpu.py puts on
this encoder; the factor 100 keeps a parity error from flipping an argmax).  If a seed fails, pick another; do not loosen
the check."""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ctc_ref as R  # noqa: E402

NOISE, DRAWS = 1e-3, 5
# (T, labels or L, V, seed): an adjacent repeat, many slack frames, larger, almost no slack, a single label
ALIGN_CASES = [
    (40, [3, 5, 5, 2, 9, 9, 4], 12, 7101),
    (90, 6, 16, 7102),
    (120, 20, 41, 7103),
    (25, 12, 9, 7104),
    (30, 1, 10, 7105),
]


def case_labels(spec, V, seed):
    if isinstance(spec, list):
        return np.asarray(spec, np.int64)
    return np.random.default_rng(seed + 50).integers(1, V, size=spec).astype(np.int64)


def ref_align(ctc_util, logp, labels, blank=0):
    return np.asarray([int(v) for v in ctc_util.forced_align(torch.from_numpy(logp), torch.from_numpy(labels), blank)],
                      np.int32)


def make_align(ctc_util):
    out = {}
    for i, (T, spec, V, seed) in enumerate(ALIGN_CASES):
        labels = case_labels(spec, V, seed)
        logits = R.planted(T, labels, V, seed)
        logp = R.log_softmax(logits)
        want = ref_align(ctc_util, logp, labels)
        mine, _, start, stop, score = R.align_one(logp, labels)
        assert np.array_equal(want, mine), f"case {i}: the reference differs from ctc_ref: new seed"
        assert R.is_ctc_path(want, labels) and (stop > start).all()
        rng = np.random.default_rng(seed + 1)
        for d in range(DRAWS):
            noisy = (logp + rng.uniform(-NOISE, NOISE, logp.shape)).astype(np.float32)
            assert np.array_equal(R.align_one(noisy, labels)[0], want), f"case {i}: flips under noise (draw {d}): new seed"
        assert np.array_equal(R.align_one(logits, labels)[0], want), f"case {i}: raw logits align differently: new seed"
        out[f"logp_{i}"], out[f"labels_{i}"], out[f"align_{i}"] = logp, labels.astype(np.int32), want
        print(f"align case {i}: T={T} L={len(labels)} V={V} score {float(score):.4f}")
    out["n_cases"] = np.asarray(len(ALIGN_CASES))
    # the documented deviation, shown once on pure noise (not stored)
    rng = np.random.default_rng(7999)
    for _ in range(20):
        labels = rng.integers(1, 8, size=5).astype(np.int64)
        logp = R.log_softmax(rng.standard_normal((30, 8)).astype(np.float32))
        want = ref_align(ctc_util, logp, labels)
        assert np.array_equal(want, R.align_one(logp, labels, wrap=True)[0])
        if not np.array_equal(want, R.align_one(logp, labels)[0]):
            print("unplanted noise: the reference equals the wrap-around restatement and differs from CTC proper")
            break
    return out


def make_asr(ref_root):
    import make_ppg_stream_golden as PS
    asr, cmvn_mod = PS.load_reference_ppg(ref_root)
    cfg = dict(cmvn_file=None, is_json_cmvn=True, input_dim=80, output_dim=40, encoder="conformer", decoder="transformer",
               encoder_conf=dict(output_size=64, attention_heads=4, linear_units=128, num_blocks=2),
               decoder_conf=dict(attention_heads=4, linear_units=64, num_blocks=1),
               model_conf=dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False, sv_conf=dict(use_sv=False)))
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
    model.eval()
    feats = 4.0 * torch.randn(2, 101, 80, generator=g) + 8.0
    lens = torch.tensor([101, 77])
    feats[1, 77:] = 0.0
    with torch.no_grad():
        hyps, scores = model.ctc_greedy_search(feats, lens)
        encoder_out, mask = model._forward_encoder(feats, lens, -1, -1, False)
        logits = model.ctc.ctc_lo(encoder_out)
        logp = model.ctc.log_softmax(encoder_out)
    rms = float(logits.pow(2).mean().sqrt())
    top = logits.topk(2, dim=-1).values
    gap = float((top[..., 0] - top[..., 1]).min())
    bound = 100 * 2e-4 * rms
    print(f"asr: logits RMS {rms:.3f}, bound {bound:.4f}, minimum top-1 / top-2 gap {gap:.4f}, hyps {[len(h) for h in hyps]}")
    assert gap > bound, "a frame's logit gap is below the bound: new seed"
    assert hyps[1][-1] == cfg["output_dim"] - 1          # the eos tail of the shorter utterance
    # everything but the CTC head is the model of ppg_conformer.npz (same seeds): only ctc.ctc_lo.* is stored here
    base = np.load(os.path.join(HERE, "ppg_conformer.npz"))
    sd = model.state_dict()
    shared = [k[2:] for k in base.files if k.startswith("w/")]
    assert shared and all(np.array_equal(sd[k].numpy(), base["w/" + k]) for k in shared)
    assert np.array_equal(feats.numpy(), base["feats"]) and np.array_equal(lens.numpy(), base["lens"])
    out = {"w/" + k: v for k, v in sd.items() if k.startswith("ctc.ctc_lo.")}
    H = max(len(h) for h in hyps)
    hyp_arr = np.full((len(hyps), H), -1, np.int32)
    for b, h in enumerate(hyps):
        hyp_arr[b, :len(h)] = h
    out.update({"feats": feats, "lens": lens, "hyps": hyp_arr, "hyp_len": np.asarray([len(h) for h in hyps], np.int32),
                "scores": scores.values, "encoder_out": encoder_out, "enc_len": mask.squeeze(1).sum(1).to(torch.int32),
                "logp": logp})
    return out


def main(ref_root: str):
    import make_golden as MG
    import make_ppg_stream_golden as PS
    PS.load_reference_ppg(ref_root)
    ctc_util = importlib.import_module("f5_tts.ppg.wenet.utils.ctc_util")
    for name, arrays in (("ctc_align.npz", make_align(ctc_util)), ("ctc_asr.npz", make_asr(ref_root))):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **MG._np(arrays))
        print("wrote", path, os.path.getsize(path) // 1024, "KiB")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
