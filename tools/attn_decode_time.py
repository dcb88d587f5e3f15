#!/usr/bin/env python3
"""Yardstick for the attention decoder's beam search (csrc/attn_decode.hip, ``ConformerEngine.decode_step``): wall ms per
utterance of the cached search against the route available without it -- ``ConformerEngine.decode`` on the WHOLE prefix at
every step plus torch log-softmax / top-k / gather for the two prunes (the reference's own tensor code, asr_model.py:374-403,
on the device, with its per-step ``end_flag.sum()`` read).

The decoder's real size: D = 256, 4 heads, 2048 units, 6 blocks, V = 4233 classes; beam 10; one utterance of T' = 250
encoder frames; U = 40 decode steps.  The weights are random, so the eos bias is pushed down: no row finishes and both routes
run exactly U steps (the cached search through ``beam_loop`` with a cache of U positions).  ``sync_every`` in {1, 4, 16}.
Looking less often only pays while nothing finishes, so a second block lets every row finish: the eos bias is raised once F
tokens are out, for F = 33..36 (every residue of 4), with room for 60 steps; a search then runs F + 1 steps rounded up to
its ``sync_every``.  The mean over the four F is what decides the default.
Wall time (the search is launch-bound: the host's launch cost is the cost), best of 3 after one warm run.
GPU box only:  python tools/attn_decode_time.py [--out profiles/attn_decode_time.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from f5e_tts_amd import ops  # noqa: E402
from tools.mas_time import wall  # noqa: E402
from tools.src_hash import csrc_sha256  # noqa: E402

I32 = torch.int32
V, BEAM, T2, U = 4233, 10, 250, 40


def set_eos_bias(eng, value):
    eng.dec["left"]["out"][1][-1] = value


def recompute_search(eng, mem, beam, sos, eos, steps, finish_at=None):
    """The reference's loop with the full decoder on the whole prefix at every step."""
    set_eos_bias(eng, -1.0e4)
    dev = mem.device
    hyps = torch.full((beam, 1), sos, dtype=torch.long, device=dev)
    scores = torch.tensor([0.0] + [-float("inf")] * (beam - 1), device=dev).unsqueeze(1)
    end_flag = torch.zeros_like(scores, dtype=torch.bool)
    for i in range(1, steps + 1):
        if int(end_flag.sum()) == beam:
            break
        if finish_at is not None and i - 1 == finish_at:
            set_eos_bias(eng, 1.0e4)
        lens = torch.full((beam,), i, dtype=I32, device=dev)
        logits = eng.decode("left", mem, None, hyps.to(I32).contiguous(), lens, beam).view(beam, i, -1)[:, -1]
        top_v, top_i = torch.log_softmax(logits, -1).topk(beam)
        top_v = torch.where(end_flag, torch.tensor([0.0] + [-float("inf")] * (beam - 1), device=dev)[None, :], top_v)
        top_i = torch.where(end_flag, torch.full_like(top_i, eos), top_i)
        scores, idx = (scores + top_v).view(1, beam * beam).topk(beam)
        scores = scores.view(-1, 1)
        idx = idx.view(-1)
        hyps = torch.cat((hyps[idx // beam], top_i.reshape(-1)[idx].view(-1, 1)), 1)
        end_flag = (hyps[:, -1] == eos).view(-1, 1)
    return hyps[:, 1:], scores.view(-1)


def best_of(fn, n=3):
    fn()
    runs = [wall(fn) for _ in range(n)]
    return min(r[0] for r in runs), runs[-1][1]


def main():
    from f5e_tts_amd.ppg.ppg_model import ConformerPPG, beam_loop
    ops.require_device()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    torch.manual_seed(11)
    m = ConformerPPG(vocab_size=V, num_blocks=1, ctc=True, decoder="transformer")
    with torch.no_grad():
        m.decoder.output_layer.weight.mul_(4.0)
        m.decoder.output_layer.bias[-1] = -1.0e4
    m = m.cuda().eval()
    eng = m.engine()
    mem = torch.randn(1, T2, eng.dim, generator=torch.Generator().manual_seed(12)).cuda()
    lines = [f"# python tools/attn_decode_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# wall ms per utterance, best of 3: D={eng.dim} 4 heads 2048 units 6 blocks V={V}, beam {BEAM}, T'={T2}, {U} steps"]
    ref_ms, (want, want_s) = best_of(lambda: recompute_search(eng, mem, BEAM, m.sos, m.eos, U))
    lines.append(f"full decoder on the whole prefix + torch top-k, a host read per step: {ref_ms:9.2f} ms  ({ref_ms / U:6.3f} ms / step)")
    print(lines[-1], flush=True)
    for reorder in (True, False):
        for sync_every in (1, 4, 16):
            def cached():
                S = eng.decode_state("left", mem, None, BEAM, m.sos, m.eos, umax=U)
                return beam_loop(S, lambda st: eng.decode_step(st, reorder), sync_every)
            ms, (hyps, scores) = best_of(cached)
            same = bool(torch.equal(hyps[0].long(), want)) if reorder else None
            lines.append(f"cached search reorder_cache={reorder!s:5} sync_every={sync_every:2d}: {ms:9.2f} ms  ({ms / U:6.3f} ms / step, "
                         f"{ref_ms / ms:5.2f} x)" + (f";  beam equal to the recompute route: {same}, max |score difference| "
                                                    f"{float((scores[0] - want_s).abs().max()):.1e}" if reorder else ""))
            print(lines[-1], flush=True)
    lines.append("# every row finishes after F + 1 steps, F = 33..36, room for 60: mean wall ms over the four F (steps run)")
    fs = (33, 34, 35, 36)

    def finishing(sync_every, F):
        def step(st):
            if st.p == F:
                set_eos_bias(eng, 1.0e4)
            return eng.decode_step(st, True)
        set_eos_bias(eng, -1.0e4)
        S = eng.decode_state("left", mem, None, BEAM, m.sos, m.eos, umax=60)
        out = beam_loop(S, step, sync_every)
        return out + (S.p,)
    ref = [best_of(lambda: recompute_search(eng, mem, BEAM, m.sos, m.eos, 60, finish_at=F)) for F in fs]
    lines.append(f"full decoder on the whole prefix + torch top-k: {sum(r[0] for r in ref) / len(fs):9.2f} ms  "
                 f"(widths {[r[1][0].shape[1] for r in ref]})")
    print(lines[-1], flush=True)
    for sync_every in (1, 4, 16):
        runs = [best_of(lambda: finishing(sync_every, F)) for F in fs]
        ok = all(torch.equal(r[1][0][0, 0].long(), w[1][0][0]) for r, w in zip(runs, ref))
        lines.append(f"cached search reorder_cache=True  sync_every={sync_every:2d}: {sum(r[0] for r in runs) / len(fs):9.2f} ms  "
                     f"(steps run {[r[1][2] for r in runs]}, widths {[r[1][0].shape[2] for r in runs]}; best hypothesis equal "
                     f"to the recompute route's: {ok})")
        print(lines[-1], flush=True)
    set_eos_bias(eng, -1.0e4)
    if out_path:
        with open(os.path.join(ROOT, out_path) if not os.path.isabs(out_path) else out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
