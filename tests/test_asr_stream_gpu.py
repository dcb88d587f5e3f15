"""Streaming recognition on the GPU: the reference's streaming parameters on the decode methods of ``ConformerPPG`` against
what the REFERENCE's own methods return on its chunk-by-chunk encoder (tests/golden/asr_stream_decode.npz, written by
tests/golden/make_asr_stream_golden.py), and ``StreamingRecognizer`` (f5e_tts_amd/ppg/streaming_asr.py) against the
whole-utterance calls.  Lists are discrete, so every comparison of lists first asserts the margin rule of
tests/ctc_beam_ref.py on the device's own logits, as tests/test_ctc_beam_gpu.py does."""
import os

import numpy as np
import pytest
import torch

import ctc_beam_ref as BR
import ppg_stream_ref as PR

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
PAIRS = [("c16", 16, -1), ("c4", 4, 2)]
K = 10


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def asr():
    from f5e_tts_amd.ppg.ppg_model import ConformerPPG
    sd, _ = PR.load_stream_fixture(True)
    z = np.load(os.path.join(GOLD, "asr_stream_decode.npz"))
    extra = {k[2:]: torch.from_numpy(z[k]).float() for k in z.files if k.startswith("w/")}
    m = ConformerPPG(80, 40, 64, 4, 128, 2, 15, global_cmvn=(sd["encoder.global_cmvn.mean"], sd["encoder.global_cmvn.istd"]),
                     causal=True, use_dynamic_chunk=True, ctc=True, decoder="transformer",
                     decoder_conf=dict(attention_heads=4, linear_units=64, num_blocks=1))
    full = m.state_dict()
    assert set(extra) <= set(full) and any(k.startswith("decoder.") for k in extra) and "ctc.ctc_lo.weight" in extra
    full.update({k: v for k, v in sd.items() if k in full})
    full.update(extra)
    m.load_state_dict(full)
    feats = torch.from_numpy(z["feats"]).float().cuda()
    return m.cuda().eval(), z, feats, torch.tensor([feats.shape[1]]).cuda()


def stored(z, tag):
    return [tuple(int(v) for v in z[f"ids_{tag}"][i, :n]) for i, n in enumerate(z[f"len_{tag}"])]


def kw_of(chunk, left):
    return dict(decoding_chunk_size=chunk, num_decoding_left_chunks=left, simulate_streaming=True)


def device_rules(m, feats, lens, chunk, left):
    """The margin rule on the DEVICE's own logits (a condition of every list comparison) -> (restated list, E, T')."""
    logits, frame_lens, _ = m._ctc_scores(feats, lens, False, (chunk, left, True))
    host = logits[0, :int(frame_lens[0])].cpu().numpy()
    mine, delta, E, same = BR.margin(host, K)
    l64, l32 = BR.normalise(host, np.float64), BR.normalise(host, np.float32)
    top = np.sort(l64, -1)
    gap, Eg = float((top[:, -1] - top[:, -2]).min()), float(np.abs(l64 - l32).max())
    print(f"chunk {chunk} left {left}: device logits delta {delta:.3e}, E {E:.3e}; greedy gap {gap:.3e}, E {Eg:.3e}")
    assert same and BR.usable(delta, E) and BR.usable(gap, Eg)
    return mine, E, len(host)


@pytest.mark.parametrize("tag,chunk,left", PAIRS, ids=[p[0] for p in PAIRS])
def test_decode_methods_with_simulate_streaming_return_the_reference_results(asr, tag, chunk, left):
    m, z, feats, lens = asr
    kw, want = kw_of(chunk, left), stored(z, tag)
    mine, E, T2 = device_rules(m, feats, lens, chunk, left)
    hyps, _ = m.ctc_greedy_search(feats, lens, pad_id=-1, **kw)
    assert hyps[0] == z[f"greedy_{tag}"].tolist()
    assert m.ctc_greedy_search(feats, lens, **kw)[0][0] == z[f"greedy_{tag}"].tolist()        # every frame is valid: no eos fill
    nbest, = m.ctc_prefix_beam_search(feats, lens, K, **kw)
    assert [h for h, _ in nbest] == [h for h, _ in mine] == want
    assert np.abs(np.asarray([s for _, s in nbest]) - [s for _, s in mine]).max() <= 10 * max(E, 1e-6 * T2)
    for w, cw in (("w0", 0.0), ("w5", 0.5)):
        (ids, score), = m.attention_rescoring(feats, lens, K, ctc_weight=cw, **kw)
        print(f"ctc_weight {cw}: winner score {score:.4f}, reference {float(z[f'resc_score_{w}_{tag}']):.4f}")
        assert ids == tuple(z[f"resc_{w}_{tag}"].tolist())
    # recognize: the same encoder choice in front of the attention beam search
    eng = m.engine()
    hyp, sc = m.recognize(feats, lens, 4, nbest=True, **kw)
    enc = eng.forward_chunk_by_chunk(feats, chunk, left)
    want_hyp, want_sc = eng.attention_beam_search("left", enc, None, 4, m.sos, m.eos, False, 4)
    assert torch.equal(hyp, want_hyp.long()) and torch.equal(sc, want_sc)
    full_hyp, _ = m.recognize(feats, lens, 4, nbest=True)
    assert hyp.shape[:2] == full_hyp.shape[:2]


def feed(rec, feats, block):
    added = 0
    for t in range(0, feats.shape[1], block):
        added += rec.accept_features(feats[0, t:t + block])
    return added


@pytest.mark.parametrize("tag,chunk,left", PAIRS, ids=[p[0] for p in PAIRS])
def test_recogniser_fed_in_blocks_equals_the_whole_utterance_calls(asr, tag, chunk, left):
    m, z, feats, lens = asr
    kw = kw_of(chunk, left)
    device_rules(m, feats, lens, chunk, left)
    offline, = m.ctc_prefix_beam_search(feats, lens, K, **kw)
    (resc_ids, resc_score), = m.attention_rescoring(feats, lens, K, ctc_weight=0.5, **kw)
    whole = m.engine().forward_chunk_by_chunk(feats, chunk, left)
    assert [h for h, _ in offline] == stored(z, tag)
    for block in (1, 33, 100, feats.shape[1]):
        rec = m.streaming_recognizer(K, chunk, left, max_seconds=2.0)
        added = feed(rec, feats, block)
        nbest = rec.finish()
        assert added <= rec.offset == whole.shape[1]                               # finish() ran the last short window
        assert [h for h, _ in nbest] == [h for h, _ in offline], f"block {block}"
        assert np.abs(np.asarray([s for _, s in nbest]) - [s for _, s in offline]).max() < 1e-3
        e = rel_l2(rec.encoder_out(), whole)
        print(f"chunk {chunk} left {left} block {block}: encoder rel L2 {e:.3e}")
        assert e < 1e-5
        ids, score = rec.finish("attention_rescoring", ctc_weight=0.5)
        assert ids == resc_ids and abs(score - resc_score) < 1e-3
        assert rec.finish() == nbest                                                # asking again changes nothing
        from f5e_tts_amd._C import F5EError
        with pytest.raises(F5EError, match="finished"):
            rec.accept_features(feats[0, :3])


def test_incremental_fbank_is_bitwise_the_whole_utterance_fbank(asr):
    from f5e_tts_amd.ppg.ppg_model import kaldiFbank
    m = asr[0]
    wav = (0.1 * torch.randn(16000, generator=torch.Generator().manual_seed(77))).cuda()
    want = kaldiFbank().eval()(wav[None])[0][0]
    assert want.shape == (98, 80)
    for block in (1, 159, 160, 401, 16000):
        rec = m.streaming_recognizer(4, 16, -1, max_seconds=2.0)
        got, inner = [], rec._accept
        rec._accept = lambda f: (got.append(f.clone()), inner(f))[1]                # the frames handed to the encoder side
        host = wav.cpu() if block == 401 else wav                                   # host samples are taken too
        for t in range(0, 16000, block):
            rec.accept_waveform(host[t:t + block])
        rec.accept_waveform(wav[:0])                                                # nothing is fine
        built = torch.cat(got)
        assert built.shape == want.shape and torch.equal(built, want), f"block {block}"
        assert rec.num_frames == 98 and rec.samples.shape[0] == 16000 - 98 * 160


def test_a_partial_result_taken_where_the_hypothesis_is_decided_is_a_prefix_of_the_final_one(asr):
    m, z, feats, lens = asr
    logp, final = z["logp_c16"], stored(z, "c16")[0]
    # the point, from the fixture: the first chunk border from which the best prefix of the frames so far stays a prefix of
    # the final best hypothesis at every later border, and is not empty
    borders = list(range(16, len(logp), 16))
    best_at = {t: BR.margin(logp[:t], K, normalised=True) for t in borders}
    ok = [t for t in borders if all(final[:len(best_at[u][0][0][0])] == best_at[u][0][0][0] for u in borders if u >= t)]
    ok = [t for t in ok if len(best_at[t][0][0][0]) > 0 and best_at[t][3] and BR.usable(best_at[t][1], best_at[t][2])]
    assert ok, "no chunk border of the fixture has a decided, non-empty best prefix"
    t = ok[0]
    rec = m.streaming_recognizer(K, 16, -1, max_seconds=2.0)
    got = rec.accept_features(feats[0, :2 * t + 1])                                   # t / 16 complete windows
    assert got == t == rec.offset
    ids, score = rec.partial()
    print(f"after {t} of {len(logp)} encoder frames: {ids} of {final}")
    assert ids == best_at[t][0][0][0] and 0 < len(ids) and ids == final[:len(ids)]
    assert rec.partial() == (ids, score) and rec.nbest()[0] == (ids, score)           # a readout does not move the state
    rec.accept_features(feats[0, 2 * t + 1:])
    assert rec.finish()[0][0] == final


def test_reset_then_a_second_utterance_equals_a_fresh_recogniser(asr):
    from f5e_tts_amd._C import F5EError
    m, z, feats, lens = asr
    other = torch.flip(feats, dims=(1,))[:, :121].contiguous()
    rec = m.streaming_recognizer(K, 16, -1, max_seconds=2.0)
    feed(rec, feats, 50)
    first = rec.finish()
    rec.reset()
    assert rec.partial() == (tuple(), 0.0) and rec.offset == 0
    feed(rec, other, 50)
    fresh = m.streaming_recognizer(K, 16, -1, max_seconds=2.0)
    feed(fresh, other, 50)
    a, b = rec.finish(), fresh.finish()
    assert a == b and a != first                                                      # bit for bit: the same launches
    assert torch.equal(rec.encoder_out(), fresh.encoder_out())
    # running past max_seconds raises on the host and leaves the utterance as it was
    small = m.streaming_recognizer(K, 16, -1, max_seconds=0.5)
    small.accept_features(feats[0, :40])
    before = small.nbest()
    with pytest.raises(F5EError, match="max_seconds"):
        small.accept_features(feats[0, 40:51])
    with pytest.raises(F5EError, match="max_seconds"):
        small.accept_waveform(torch.zeros(16000))
    assert small.nbest() == before and small.num_frames == 40
    small.accept_features(feats[0, 40:50])
    assert small.num_frames == 50


def test_transcribe_stream_yields_partial_texts_and_ends_with_the_whole_utterance_result(asr):
    from f5e_tts_amd.ppg.ctc_align import CTCAligner
    m = asr[0]
    table = {"<blank>": 0, **{chr(96 + i): i for i in range(1, 27)}, **{f"<{i}>": i for i in range(27, 39)}, "<sos/eos>": 39}
    al = CTCAligner(model=m, symbol_table=table, device="cuda")
    wav = 0.1 * torch.randn(1, 16000, generator=torch.Generator().manual_seed(3))
    f, n, _ = al._feats(wav, 16000)
    device_rules(m, f, n, 16, -1)
    blocks = [wav[0, t:t + 3000] for t in range(0, 16000, 3000)]
    out = list(al.transcribe_stream(blocks, max_seconds=2.0))
    assert len(out) == len(blocks) + 1 and all(isinstance(s, str) for s in out)
    assert out[-1] == al.transcribe(wav, 16000, mode="ctc_prefix_beam_search", decoding_chunk_size=16, simulate_streaming=True)
    rec = al.stream(beam_size=4, max_seconds=2.0)
    rec.accept_waveform(wav)
    assert isinstance(rec.partial_text(), str) and isinstance(rec.finish_text("attention_rescoring"), str)
