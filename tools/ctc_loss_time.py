#!/usr/bin/env python3
"""Yardstick for f5e_ctc_loss (csrc/ctc.hip) and for best-of-N synthesis ranked by it.
(a) ms per launch of f5e_ctc_loss (both launches: the frame normaliser and the recursion) at the candidate-ranking shape
    (N = 4 candidates, T' = 250 encoder frames, L = 60 labels; V = 218 and 4233 classes) and at one long case (T' = 3000,
    L = 500), against the copy-to-host route: D2H of the [N, T', V] logits plus torch.nn.functional.ctc_loss on the CPU
    (log_softmax included, fp32, reduction "none").  The copy is also timed alone: it bounds that route from below.
(b) one C2-shaped chunk (2 s prompt, 5 s total, NFE 32, F5TTS_v1_Base on synthetic weights, Vocos) through
    infer_batch_process at best_of 1 and 4 with a CTCAligner on a synthetic conformer (6 blocks, 256 wide, V = 218): wall ms
    per call, and the share of the best_of = 4 call that scorer.score_batch takes (measured in a pass of its own with a
    synchronising wrapper around the scorer, which the other passes do not carry).
Kernel: 10 launches per graph (f5e_graph_*), HIP events around 5 replays.  Host route and (b): wall clock, synchronised.
GPU box only:  python tools/ctc_loss_time.py [--out profiles/ctc_loss_time.txt]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from f5e_tts_amd import ops  # noqa: E402
from tools.mas_time import LAUNCHES, REPLAYS, time_graph, wall  # noqa: E402
from tools.src_hash import csrc_sha256  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctc_ref  # noqa: E402

I32 = torch.int32


def kernel_lines():
    side = torch.cuda.Stream()
    out = []
    for name, B, T, L, V in (("4 candidates", 4, 250, 60, 218), ("4 candidates", 4, 250, 60, 4233),
                             ("long recording", 1, 3000, 500, 218)):
        rng = np.random.default_rng(21)
        labels = rng.integers(1, V, size=(B, L)).astype(np.int32)
        host = np.stack([ctc_ref.planted(T, labels[b], V, 22 + b) for b in range(B)])
        scores, lab = torch.from_numpy(host).cuda(), torch.from_numpy(labels).cuda()
        t_len = torch.full((B,), T, dtype=I32, device="cuda")
        l_len = torch.full((B,), L, dtype=I32, device="cuda")
        logp = torch.empty(B, device="cuda")
        ws = torch.empty(ops.ctc_loss_workspace_bytes(B, T), dtype=torch.uint8, device="cuda")
        ms = time_graph(lambda: ops.ctc_loss(scores, lab, t_len, l_len, 0, logp=logp, workspace=ws), side)
        d2h_ms, on_host = wall(lambda: scores.cpu())
        tl, ll = torch.full((B,), T, dtype=torch.long), torch.full((B,), L, dtype=torch.long)

        def host_loss():
            return -F.ctc_loss(F.log_softmax(on_host, -1).transpose(0, 1), torch.from_numpy(labels).long(), tl, ll,
                               reduction="none")
        host_loss()
        cpu_ms, want = wall(host_loss)
        err = float((logp.cpu().double() - want.double()).abs().max() / want.double().abs().max())
        out.append(f"{name}: N={B} T'={T} L={L} V={V} ({B * T * V * 4 / 1e6:.2f} MB of logits)  f5e_ctc_loss {ms:8.4f} ms  |  "
                   f"host route: D2H {d2h_ms:7.3f} ms + torch CPU ctc_loss {cpu_ms:8.3f} ms = {(d2h_ms + cpu_ms) / ms:6.1f} x the "
                   f"kernel; the copy alone = {d2h_ms / ms:5.1f} x;  max relative difference {err:.1e}")
        print(out[-1], flush=True)
    return out


class TimedScorer:
    def __init__(self, inner):
        self.inner, self.ms = inner, 0.0

    def score_batch(self, *a, **kw):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = self.inner.score_batch(*a, **kw)
        torch.cuda.synchronize()
        self.ms += (time.perf_counter() - t) * 1e3
        return out


def best_of_lines():
    from f5e_tts_amd.infer import utils_infer as U
    from f5e_tts_amd.model import CFM, DiT
    from f5e_tts_amd.ppg import ConformerPPG
    from f5e_tts_amd.ppg.ctc_align import CTCAligner
    from f5e_tts_amd.vocoder import Vocos
    from tools import synth as SY
    dit = DiT(dim=1024, depth=22, heads=16, ff_mult=2, text_dim=512, conv_layers=4, text_num_embeds=2545)
    dit.load_state_dict(SY.init_dit_state(SY.DiTConfig(), 1234), strict=True)
    cfm = CFM(transformer=dit, vocab_char_map={chr(32 + k): k for k in range(95)}).cuda().eval()
    voc = Vocos()
    voc.load_state_dict(SY.init_vocos_state(), strict=False)
    voc = voc.cuda().eval()
    torch.manual_seed(5)
    asr = ConformerPPG(ctc=True).cuda().eval()                  # the reference's PPG extractor shape, random weights
    scorer = CTCAligner(model=asr, symbol_table={ch: 1 + k for k, ch in enumerate("abcdefghijklmnopqrstuvwxyz")})
    ref = (SY.synthetic_ref_wave(188), 24000)
    text = "here we generate something just for the test of it"
    kw = dict(nfe_step=32, fix_duration=5.0, device="cuda")

    def go(**more):
        return next(U.infer_batch_process(ref, "Some call me nature, others call me mother nature. ", [text], cfm, voc, **kw, **more))

    for n in (1, 4):                                            # graphs captured, scratch allocated
        go(best_of=n, scorer=scorer, seed=1)
    one = min(wall(lambda: go(best_of=1, seed=1))[0] for _ in range(3))
    four = min(wall(lambda: go(best_of=4, scorer=scorer, seed=1))[0] for _ in range(3))
    timed = TimedScorer(scorer)
    report = []
    go(best_of=4, scorer=timed, seed=1, report=report)
    line = (f"C2-shaped chunk (2 s prompt, 5 s total, NFE 32, v1_Base synthetic, Vocos): best_of=1 {one:8.2f} ms, best_of=4 "
            f"{four:8.2f} ms = {four / one:4.2f} x; scorer.score_batch (resample, fbank, conformer at batch 4, f5e_ctc_loss) "
            f"{timed.ms:6.2f} ms = {100 * timed.ms / four:4.1f} % of the best_of=4 call; scores {report[0]['scores']}")
    print(line, flush=True)
    return [line]


def main():
    ops.require_device()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = [f"# python tools/ctc_loss_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# kernel: ms per launch, {LAUNCHES}-launch graph, HIP events over {REPLAYS} replays; host route and best-of-N: "
             f"wall ms (synchronised)"]
    lines += kernel_lines()
    lines += best_of_lines()
    if out_path:
        with open(os.path.join(ROOT, out_path) if not os.path.isabs(out_path) else out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
