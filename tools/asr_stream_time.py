#!/usr/bin/env python3
"""Yardstick for streaming recognition (f5e_tts_amd/ppg/streaming_asr.py): what one chunk step of ``StreamingRecognizer``
costs, against the only route to a partial transcript without it -- the whole-utterance
``ctc_prefix_beam_search(..., simulate_streaming=True)`` on everything heard so far.

Model: the default extractor size (D = 256, 4 heads, 6 blocks, 2048 units, V = 218; the size of tools/ctc_beam_time.py),
causal and chunk-trained, seeded weights.  Audio: seeded noise at 16 kHz, fed in blocks of 5120 samples = 320 ms = one chunk
of 16 encoder frames at 20 ms.

Per audio length (5, 20, 60 s):
  * the recogniser: wall ms per ``accept_waveform`` call that ran a chunk (fbank + forward_chunk + CTC projection + search
    chunk, synchronised), mean over the utterance and mean over its LAST ten chunks (with ``num_decoding_left_chunks = -1``
    the encoder's caches grow with the utterance), without and with one ``partial()`` per chunk;
  * the re-decode route: wall ms of ONE fbank + ``ctc_prefix_beam_search(simulate_streaming=True)`` over the whole length,
    which that route pays again for every new chunk.
No threshold: these are figures.  GPU box only:  python tools/asr_stream_time.py [--out profiles/asr_stream_time.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from f5e_tts_amd import ops  # noqa: E402
from tools.mas_time import wall  # noqa: E402
from tools.src_hash import csrc_sha256  # noqa: E402

BLOCK, CHUNK, BEAM, V = 5120, 16, 10, 218


def stream_ms(m, wav, with_partial):
    rec = m.streaming_recognizer(BEAM, CHUNK, -1, max_seconds=wav.shape[0] / 16000.0 + 1.0)
    steps = []
    for t in range(0, wav.shape[0], BLOCK):
        def step():
            n = rec.accept_waveform(wav[t:t + BLOCK])
            if n and with_partial:
                rec.partial()
            return n
        ms, n = wall(step)
        if n:
            steps.append(ms)
    ms, nbest = wall(rec.finish)
    return steps, ms, nbest


def main():
    from f5e_tts_amd.ppg.ppg_model import ConformerPPG, kaldiFbank
    ops.require_device()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    torch.manual_seed(11)
    m = ConformerPPG(vocab_size=V, global_cmvn=(torch.zeros(80), torch.ones(80)), causal=True, use_dynamic_chunk=True,
                     ctc=True).cuda().eval()
    fbank = kaldiFbank().eval()
    lines = [f"# python tools/asr_stream_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# D=256 6 blocks V={V} beam {BEAM} chunk {CHUNK} (320 ms of audio per chunk), left chunks -1; wall ms, synchronised"]
    warm = 0.1 * torch.randn(16000 * 2, generator=torch.Generator().manual_seed(1)).cuda()
    stream_ms(m, warm, True)
    for secs in (5, 20, 60):
        wav = (0.1 * torch.randn(16000 * secs, generator=torch.Generator().manual_seed(secs))).cuda()
        parts = []
        for with_partial in (False, True):
            steps, fin_ms, nbest = stream_ms(m, wav, with_partial)
            last = steps[-10:]
            parts.append(f"{'with' if with_partial else 'no'} partial(): {sum(steps) / len(steps):7.2f} ms per chunk over "
                         f"{len(steps)} chunks, last ten {sum(last) / len(last):7.2f}, worst {max(steps):7.2f}, finish() {fin_ms:6.2f}")

        def redecode():
            feats, n = fbank(wav[None])
            return m.ctc_prefix_beam_search(feats, n.cuda(), BEAM, decoding_chunk_size=CHUNK, simulate_streaming=True)
        redecode()
        re_ms, offline = wall(redecode)
        same = [h for h, _ in offline[0]][:1] == [h for h, _ in nbest][:1]
        lines.append(f"{secs:2d} s of audio  |  recogniser, " + "; ".join(parts) + f"  |  re-decode of everything so far: "
                     f"{re_ms:8.2f} ms per partial result ({re_ms / (sum(last) / len(last)):5.1f} x the last chunks' step); "
                     f"best hypothesis equal: {same}")
        print(lines[-1], flush=True)
    if out_path:
        with open(os.path.join(ROOT, out_path) if not os.path.isabs(out_path) else out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
