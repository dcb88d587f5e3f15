"""Host side of streaming recognition (f5e_tts_amd/ppg/streaming_asr.py and the reference's streaming parameters on the
decode methods): the window bookkeeping against the restatement of the reference's loop, the caller bugs that must raise
F5EError before anything touches a device, and the new fixture against the NumPy restatement of the search."""
import os

import numpy as np
import pytest
import torch

import ctc_beam_ref as BR
import ppg_stream_ref as PR

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_ready_windows_reproduce_the_reference_loop_for_every_total_and_block_pattern():
    from f5e_tts_amd.ppg.streaming_asr import ready_windows
    rng = np.random.default_rng(20240)
    for chunk in (1, 4, 16):
        window = 2 * (chunk - 1) + 3
        for total in range(0, 201):
            want = PR.stream_windows(total, chunk)
            assert ready_windows(total, 0, chunk, True) == want                      # the whole utterance at once
            assert want == [(c, min(c + window, total)) for c in range(0, total - 3 + 1, 2 * chunk)]
            for pattern in range(4):
                # blocks of 1, of random sizes up to 3 windows (zeros included), of exactly one stride, and one big block
                got, fed, cur = [], 0, 0
                while fed < total:
                    n = (1, int(rng.integers(0, 3 * window + 1)), 2 * chunk, total)[pattern]
                    fed = min(total, fed + n)
                    now = ready_windows(fed, cur, chunk, False)
                    assert all(b - a == window for a, b in now)                      # only complete windows before the end
                    got += now
                    cur = now[-1][0] + 2 * chunk if now else cur
                got += ready_windows(total, cur, chunk, True)
                assert got == want, (chunk, total, pattern)
    from f5e_tts_amd._C import F5EError
    with pytest.raises(F5EError, match="decoding_chunk_size"):
        ready_windows(10, 0, 0, True)


def models():
    from f5e_tts_amd.ppg.ppg_model import ConformerPPG
    conf = dict(attention_heads=4, linear_units=64, num_blocks=1)
    chunked = ConformerPPG(80, 40, 64, 4, 128, 2, 15, causal=True, use_dynamic_chunk=True, ctc=True, decoder="transformer",
                           decoder_conf=conf)
    plain = ConformerPPG(80, 40, 64, 4, 128, 2, 15, ctc=True, decoder="transformer", decoder_conf=conf)
    return chunked, plain


def decode_calls(m, feats, lens, **kw):
    return [lambda: m.ctc_greedy_search(feats, lens, **kw), lambda: m.ctc_prefix_beam_search(feats, lens, 4, **kw),
            lambda: m.attention_rescoring(feats, lens, 4, **kw), lambda: m.recognize(feats, lens, 4, **kw)]


def test_caller_bugs_of_the_streaming_parameters_raise_without_a_device():
    from f5e_tts_amd._C import F5EError
    chunked, plain = models()
    one, two = (torch.zeros(1, 40, 80), torch.tensor([40])), (torch.zeros(2, 40, 80), torch.tensor([40, 40]))
    for call in decode_calls(chunked, *one, decoding_chunk_size=0) + \
            decode_calls(chunked, *one, decoding_chunk_size=0, simulate_streaming=True):
        with pytest.raises(F5EError, match="must not be 0"):
            call()
    for call in decode_calls(chunked, *two, decoding_chunk_size=16, simulate_streaming=True):
        with pytest.raises(F5EError, match="one utterance at a time"):
            call()
    for call in decode_calls(plain, *one, decoding_chunk_size=16, simulate_streaming=True):
        with pytest.raises(F5EError, match="chunk-trained"):
            call()
    for call in decode_calls(chunked, *one, decoding_chunk_size=16):
        with pytest.raises(F5EError, match="out of scope"):
            call()


def test_caller_bugs_of_the_recogniser_raise_without_a_device():
    from f5e_tts_amd._C import F5EError
    from f5e_tts_amd.ppg.ctc_align import CTCAligner
    from f5e_tts_amd.ppg.streaming_asr import check_capacity, check_sample_rate
    chunked, plain = models()
    for beam in (0, 17, 41):
        with pytest.raises(F5EError, match="beam_size"):
            chunked.streaming_recognizer(beam_size=beam)
    with pytest.raises(F5EError, match="decoding_chunk_size"):
        chunked.streaming_recognizer(decoding_chunk_size=0)
    with pytest.raises(F5EError, match="chunk-trained"):
        plain.streaming_recognizer()
    with pytest.raises(F5EError, match="max_seconds"):
        chunked.streaming_recognizer(max_seconds=0.0)
    # running past max_seconds: the check every accept_* call makes before it launches anything
    check_capacity(5990, 10, 6000, 60.0)
    with pytest.raises(F5EError, match="max_seconds"):
        check_capacity(5990, 11, 6000, 60.0)
    check_sample_rate(16000)
    table = {"<blank>": 0, "a": 1}
    al = CTCAligner(model=chunked, symbol_table=table, device="cpu")
    for bad in (8000, 44100):
        with pytest.raises(F5EError, match="16000 Hz"):
            al.transcribe_stream([torch.zeros(160)], sr=bad)                       # raised at the call, not at the first next()
    with pytest.raises(F5EError, match="unknown mode"):
        al.transcribe_stream([], mode="ctc_greedy_search")
    with pytest.raises(F5EError, match="must not be 0"):
        al.transcribe(torch.zeros(1, 16000), 16000, decoding_chunk_size=0)


def stored(z, tag):
    return [tuple(int(v) for v in z[f"ids_{tag}"][i, :n]) for i, n in enumerate(z[f"len_{tag}"])]


@pytest.mark.parametrize("tag", ["c16", "c4"])
def test_the_fixture_lists_equal_the_restatement_on_the_stored_log_probabilities(tag):
    z = np.load(os.path.join(GOLD, "asr_stream_decode.npz"))
    logp, want = z[f"logp_{tag}"], stored(z, tag)
    frames = sum((b - a - 3) // 2 + 1 for a, b in PR.stream_windows(165, {"c16": 16, "c4": 4}[tag]))
    assert logp.shape == (frames, 40)
    mine, delta, E, same = BR.margin(logp, 10, normalised=True)
    assert same and BR.usable(delta, E, 100.0)
    assert [p for p, _ in mine] == want
    rel = max(abs(a[1] - float(s)) / max(abs(float(s)), 1e-30) for a, s in zip(mine, z[f"score_{tag}"]))
    assert rel < 1e-9
    # greedy: argmax per frame, repeats collapsed, blanks dropped
    best = logp.argmax(-1)
    keep = [int(v) for i, v in enumerate(best) if v != 0 and (i == 0 or v != best[i - 1])]
    assert keep == z[f"greedy_{tag}"].tolist()
    for w in ("w0", "w5"):
        assert tuple(z[f"resc_{w}_{tag}"].tolist()) in want
    # only the tensors ppg_stream_common.npz does not hold, stored exactly as float16
    keys = [k for k in z.files if k.startswith("w/")]
    assert keys and all(k.startswith(("w/ctc.", "w/decoder.")) and z[k].dtype == np.float16 for k in keys)
    assert z["feats"].dtype == np.float16 and z["feats"].shape == (1, 165, 80)
