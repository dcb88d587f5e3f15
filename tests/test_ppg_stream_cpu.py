"""Streaming (chunk-by-chunk) PPG extraction, CPU side: the fp32 restatement of the reference's cached loop
(tests/ppg_stream_ref.py) against the reference-generated fixtures (tests/golden/make_ppg_stream_golden.py), the one-pass
formulation the HIP path uses against that loop, the configuration / error paths of ConformerPPG, and the position-table
cache under threads.  No kernel is launched here."""
import threading

import pytest
import torch
import torch.nn.functional as F

import ppg_stream_ref as R
from oracle import f5e_ppg_oracle as P

TOL = dict(rtol=1e-4, atol=5e-5)   # fp32 vs fp32, same operation order: the gate of test_ppg_oracle_golden.py


@pytest.mark.parametrize("causal", [False, True])
def test_restatement_reproduces_the_reference_fixtures(causal):
    """extract(stream=True) of the reference on an utterance of 20 chunks + 2 frames (the 17-left-chunk limit is reached)
    and on one of 2 chunks + 5 frames; frame counts; and two consecutive forward_chunk calls with all their caches."""
    sd, g = R.load_stream_fixture(causal)
    assert P.encoder_depth(sd) == 2 and sd["encoder.encoders.0.conv_module.depthwise_conv.weight"].shape[-1] == 15
    for tag, frames in (("long", 322), ("short", 37)):
        feats = g["feats_" + tag]
        assert sum((e - c - 3) // 2 + 1 for c, e in R.stream_windows(feats.shape[1], 16)) == frames
        ppg, logits = R.asr_extract_stream(sd, feats, heads=4, causal=causal)
        assert ppg.shape == g["ppg_" + tag].shape == (1, frames, 64)
        torch.testing.assert_close(ppg, g["ppg_" + tag], **TOL)
        torch.testing.assert_close(logits, g["logits_" + tag], **TOL)
    cache = (None, None, None)
    for step, (cur, offset) in enumerate(((0, 0), (32, 16))):
        y, sub, att, cnn = R.forward_chunk(sd, g["feats_long"][:, cur:cur + 33], offset, 16 * 17, *cache, heads=4, causal=causal)
        cache = (sub, att, cnn)
        torch.testing.assert_close(y, g[f"step{step}_y"], **TOL)
        torch.testing.assert_close(sub, g[f"step{step}_sub"], **TOL)
        assert y.shape == (1, 16, 64) and sub.shape == (1, 16 * (step + 1), 64)
        for i in range(2):
            torch.testing.assert_close(att[i], g[f"step{step}_att{i}"], **TOL)
            assert cnn[i].shape == g[f"step{step}_cnn{i}"].shape == ((1, 64, 14) if causal else (1,))
            torch.testing.assert_close(cnn[i], g[f"step{step}_cnn{i}"], **TOL)


def one_pass_encoder(sd, feats, heads, causal, chunk, left):
    """The formulation of the HIP path in plain torch: ONE pass over the utterance with (a) the chunk band as attention mask
    and (b) a depthwise convolution that is causal with GLU(pointwise_conv1(0)) on its left (causal) or never reads across
    a chunk boundary (not causal).  Everything else in a layer is row-wise."""
    x = (feats - sd["encoder.global_cmvn.mean"]) * sd["encoder.global_cmvn.istd"]
    x, pos, _ = P.conv2d_subsampling2(sd, "encoder.embed.", x, torch.ones(1, 1, feats.shape[1], dtype=torch.bool))
    t = x.shape[1]
    c = torch.arange(t) // chunk
    band = c[None, :] <= c[:, None]
    if left >= 0:
        band &= c[None, :] >= c[:, None] - left
    for i in range(P.encoder_depth(sd)):
        p = f"encoder.encoders.{i}."
        ln = lambda n, v: F.layer_norm(v, (v.shape[-1],), sd[p + n + ".weight"], sd[p + n + ".bias"], eps=1e-5)   # noqa: E731
        ff = lambda n, v: F.linear(F.silu(F.linear(v, sd[p + n + ".w_1.weight"], sd[p + n + ".w_1.bias"])),           # noqa: E731
                                   sd[p + n + ".w_2.weight"], sd[p + n + ".w_2.bias"])
        x = x + 0.5 * ff("feed_forward_macaron", ln("norm_ff_macaron", x))
        x = x + P.rel_mha(sd, p + "self_attn.", ln("norm_mha", x), band[None], pos, heads)
        cm = p + "conv_module."
        w = sd[cm + "depthwise_conv.weight"]
        k = w.shape[-1]
        h = ln("norm_conv", x).transpose(1, 2)
        if causal:
            h = F.pad(h, (k - 1, 0))
        h = F.glu(F.conv1d(h, sd[cm + "pointwise_conv1.weight"], sd[cm + "pointwise_conv1.bias"]), dim=1)
        if causal:
            h = F.conv1d(h, w, sd[cm + "depthwise_conv.bias"], groups=w.shape[0])
        else:
            h = torch.cat([F.conv1d(part, w, sd[cm + "depthwise_conv.bias"], padding=(k - 1) // 2, groups=w.shape[0])
                           for part in h.split(chunk, dim=2)], dim=2)
        h = F.batch_norm(h, sd[cm + "norm.running_mean"], sd[cm + "norm.running_var"], sd[cm + "norm.weight"],
                         sd[cm + "norm.bias"], training=False, eps=1e-5)
        x = x + F.conv1d(F.silu(h), sd[cm + "pointwise_conv2.weight"], sd[cm + "pointwise_conv2.bias"]).transpose(1, 2)
        x = x + 0.5 * ff("feed_forward", ln("norm_ff", x))
        x = ln("norm_final", x)
    return F.layer_norm(x, (x.shape[-1],), sd["encoder.after_norm.weight"], sd["encoder.after_norm.bias"], eps=1e-5)


@pytest.mark.parametrize("causal,kernel", [(False, 15), (True, 15), (True, 8)])
@pytest.mark.parametrize("chunk,left", [(16, 17), (8, 2)])
def test_one_pass_formulation_equals_the_cached_loop(causal, kernel, chunk, left):
    """The equivalence the GPU path relies on, at 20 chunks + 9 frames of 16 (the left limit of 17 chunks is exceeded), an
    even causal kernel included.  fp32 on both sides; the two differ in summation order only (keys masked vs sliced)."""
    from f5e_tts_amd.ppg import ConformerPPG
    m = ConformerPPG(80, 40, 64, 4, 128, 2, kernel, global_cmvn=(torch.zeros(80), torch.ones(80)), causal=causal,
                     use_dynamic_chunk=True)
    sd = R.seeded_state(m, 31)
    feats = 3.0 * torch.randn(1, 2 * (20 * 16 + 9) + 1, 80, generator=torch.Generator().manual_seed(32)) + 6.0
    loop = R.forward_chunk_by_chunk(sd, feats, chunk, left, heads=4, causal=causal)
    one = one_pass_encoder(sd, feats, 4, causal, chunk, left)
    assert loop.shape == one.shape == (1, 329, 64)
    torch.testing.assert_close(one, loop, **TOL)
    # the band matters for this input: the full-context encoder is somewhere else
    full = one_pass_encoder(sd, feats, 4, causal, 10 ** 6, -1)
    assert float((full - loop).norm() / loop.norm()) > 1e-3


def test_from_config_accepts_streaming_settings_and_extract_checks_them():
    from f5e_tts_amd import _C
    from f5e_tts_amd.ppg import ConformerPPG
    base = dict(cmvn_file=None, is_json_cmvn=True, input_dim=80, output_dim=40, encoder="conformer")
    enc = dict(output_size=64, attention_heads=4, linear_units=128, num_blocks=2)
    m = ConformerPPG.from_config(dict(base, encoder_conf=dict(enc, causal=True, use_dynamic_chunk=True, cnn_module_kernel=8)))
    assert m.causal and m.use_dynamic_chunk and m.static_chunk_size == 0
    assert m.encoder.encoders[0].conv_module.depthwise_conv.weight.shape == (64, 1, 8)
    m = ConformerPPG.from_config(dict(base, encoder_conf=dict(enc, static_chunk_size=16)))
    assert not m.causal and not m.use_dynamic_chunk and m.static_chunk_size == 16
    with pytest.raises(_C.F5EError, match="one utterance at a time"):
        m.extract(torch.zeros(2, 50, 80), torch.tensor([50, 50]), stream=True)
    plain = ConformerPPG.from_config(dict(base, encoder_conf=enc))          # today's models: unchanged defaults
    assert not plain.causal and not plain.use_dynamic_chunk and plain.static_chunk_size == 0
    with pytest.raises(_C.F5EError, match="chunk-trained"):
        plain.extract(torch.zeros(1, 50, 80), torch.tensor([50]), stream=True)
    with pytest.raises(_C.F5EError, match="chunk-trained"):
        plain.forward_encoder_chunk(torch.zeros(1, 33, 80), 0, 272)
    with pytest.raises(_C.F5EError, match="unsupported encoder_conf"):
        ConformerPPG.from_config(dict(base, encoder_conf=dict(enc, causal=True, input_layer="conv2d4")))


def test_new_abi_entries_are_declared_and_no_cpu_path():
    from f5e_tts_amd import _C, ops
    lib = _C.lib()
    for name, nargs in (("f5e_relpos_attn", 20), ("f5e_dwconv_stream", 12)):
        assert hasattr(lib, name) and len(_C.SIGNATURES[name]) == nargs
    assert lib.f5e_abi_version() == 2
    z = torch.zeros(16, 64)
    with pytest.raises(_C.F5EError):
        ops.relpos_attn(torch.zeros(16, 128), z, z, z, z.clone(), 4, 0.25)
    with pytest.raises(_C.F5EError):
        ops.dwconv_stream(z[None], torch.zeros(15, 64), torch.zeros(64), z[None].clone(), causal=True)


def test_pos_table_is_race_free_across_threads():
    """Eight threads ask one engine for tables of distinct lengths (and offsets) at once: each gets its own rows every time.
    The engine is built without a device here; pos_table only needs its width, device and cache."""
    from f5e_tts_amd.ppg.ppg_model import ConformerEngine
    eng = object.__new__(ConformerEngine)
    eng.dim, eng.device, eng._pe = 64, torch.device("cpu"), {}
    errors, start = [], threading.Barrier(8)

    def worker(i):
        try:
            start.wait()
            for r in range(60):
                t = 40 + 37 * i + (r % 3)
                off = 0 if r % 2 == 0 else 16 * i
                pe = eng.pos_table(t, off)
                ref = P.rel_pos_table(off + t, 64)[0, off:]
                if pe.shape != (t, 64) or not torch.equal(pe, ref):
                    errors.append((i, r, tuple(pe.shape)))
        except Exception as e:      # noqa: BLE001  (a KeyError here is the race this test is about)
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors[:5]
