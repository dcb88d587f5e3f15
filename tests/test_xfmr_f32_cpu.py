"""The shared fp32 transformer layer's host side (f5e-tts_amd/xfmr_f32.py), without a GPU: ``fold_layer`` stacks exactly what the
models stacked by hand, the scratch planner aligns to 64 floats, and ``workspace_bytes`` of the three users did not move."""
import pytest
import torch
import torch.nn as nn

TINY = dict(conv_dim=(32,) * 7, encoder_embed_dim=64, encoder_layers=3, encoder_attention_heads=4, encoder_ffn_embed_dim=128)


def holders(D=8, FF=12, k_bias=True):
    torch.manual_seed(5)
    lin = lambda i, o, b=True: nn.Linear(i, o, bias=b)   # noqa: E731
    return dict(ln1=nn.LayerNorm(D), q=lin(D, D), k=lin(D, D, k_bias), v=lin(D, D), out=lin(D, D), ln_ff=nn.LayerNorm(D),
                fc1=lin(D, FF), fc2=lin(FF, D), ln_x=nn.LayerNorm(D), xq=lin(D, D), xk=lin(D, D, k_bias), xv=lin(D, D), xout=lin(D, D))


@pytest.mark.parametrize("k_bias", [True, False])
def test_fold_layer_stacks_holders_exactly(k_bias):
    """q | k | v and k | v by rows; a missing k bias (Whisper) is exact zeros in the k third / the k half."""
    from f5e_tts_amd.xfmr_f32 import fold_layer
    h = holders(k_bias=k_bias)
    extra = (torch.ones(2),)
    W = fold_layer("cpu", h["ln1"], h["q"], h["k"], h["v"], h["out"], h["ln_ff"], h["fc1"], h["fc2"], ln_x=h["ln_x"], xq=h["xq"],
                   xk=h["xk"], xv=h["xv"], xout=h["xout"], extra=extra)
    zero = torch.zeros(8)
    kb, xkb = (h["k"].bias, h["xk"].bias) if k_bias else (zero, zero)
    want = dict(ln1=(h["ln1"].weight, h["ln1"].bias),
                qkv=(torch.cat([h["q"].weight, h["k"].weight, h["v"].weight], 0), torch.cat([h["q"].bias, kb, h["v"].bias])),
                out=(h["out"].weight, h["out"].bias), ln_x=(h["ln_x"].weight, h["ln_x"].bias), xq=(h["xq"].weight, h["xq"].bias),
                xkv=(torch.cat([h["xk"].weight, h["xv"].weight], 0), torch.cat([xkb, h["xv"].bias])),
                xout=(h["xout"].weight, h["xout"].bias), ln_ff=(h["ln_ff"].weight, h["ln_ff"].bias),
                ff=(h["fc1"].weight, h["fc1"].bias, h["fc2"].weight, h["fc2"].bias))
    for name, ts in want.items():
        got = getattr(W, name)
        assert len(got) == len(ts), name
        for g, t in zip(got, ts):
            assert g.dtype == torch.float32 and g.is_contiguous() and not g.requires_grad and torch.equal(g, t.detach()), name
    assert W.extra is extra
    if not k_bias:
        assert not W.qkv[1][8:16].any() and not W.xkv[1][:8].any()


def test_fold_layer_takes_weight_bias_pairs_and_leaves_out_source_attention():
    """The wenet decoder folds from state-dict tensors: (weight, bias) pairs give what holders give; without ``ln_x`` the four
    source-attention fields are None."""
    from f5e_tts_amd.xfmr_f32 import fold_layer
    h = holders()
    pair = {k: (m.weight.detach().double(), m.bias.detach().double()) for k, m in h.items()}      # any dtype in, f32 out
    names = ("ln1", "q", "k", "v", "out", "ln_ff", "fc1", "fc2")
    cross = {k: h[k] for k in ("ln_x", "xq", "xk", "xv", "xout")}
    a = fold_layer("cpu", *(h[n] for n in names), **cross)
    b = fold_layer("cpu", *(pair[n] for n in names), **{k: pair[k] for k in cross})
    for name in a._fields[:-1]:
        assert all(torch.equal(x, y) and y.dtype == torch.float32 for x, y in zip(getattr(a, name), getattr(b, name))), name
    assert torch.equal(b.qkv[1], torch.cat([h[n].bias for n in "qkv"]).detach())                 # wenet's q | k | v and k | v
    assert torch.equal(b.xkv[0], torch.cat([h["xk"].weight, h["xv"].weight], 0).detach())
    c = fold_layer("cpu", *(h[n] for n in names))
    assert c.ln_x is None and c.xq is None and c.xkv is None and c.xout is None and c.extra is None
    assert torch.equal(c.qkv[0], a.qkv[0]) and torch.equal(c.ff[2], a.ff[2])


def test_plan_offsets_are_multiples_of_64_floats_and_disjoint():
    from f5e_tts_amd.xfmr_f32 import plan, view
    shapes = dict(a=(3,), b=(2, 65), c=(64,), d=(1, 1, 1), e=(7, 9, 5))
    pl = plan(shapes)
    assert list(pl) == list(shapes) + ["_total"]
    end = 0
    for name, shape in shapes.items():
        off, got = pl[name]
        assert got == shape and off % 64 == 0 and off >= end
        end = off + torch.Size(shape).numel()
    assert pl["_total"] == ((end + 63) // 64 * 64, ())
    ws = torch.arange(pl["_total"][0], dtype=torch.float32)
    v = view(ws, pl, "b")
    assert v.shape == (2, 65) and v[0, 0] == pl["b"][0] and v.data_ptr() == ws.data_ptr() + 4 * pl["b"][0]


def test_workspace_refusal_names_the_caller():
    from f5e_tts_amd._C import F5EError
    from f5e_tts_amd.xfmr_f32 import take
    with pytest.raises(F5EError, match=r"Wav2Vec2\.extract: workspace must be a contiguous 16-byte aligned f32 / uint8 GPU tensor "
                                       r"of at least 400 bytes \(workspace_bytes\)"):
        take(torch.empty(100), 100, "cpu", "Wav2Vec2.extract")            # not on the GPU


def test_workspace_bytes_did_not_move():
    """Host arithmetic; the numbers are those of the hand-written planners this module replaced (tiny configurations of
    tests/test_wavlm_cpu.py and tests/test_utmos_cpu.py, then the plans of the published WavLM-large / wav2vec2-base shapes)."""
    from f5e_tts_amd.eval.utmos import UTMOS22Strong
    from f5e_tts_amd.eval.wav2vec2 import Wav2Vec2, Wav2Vec2Config
    from f5e_tts_amd.eval.wavlm import WavLM, WavLMConfig
    wavlm, w2v = WavLM(WavLMConfig(**TINY)), Wav2Vec2(Wav2Vec2Config(**TINY))
    utmos = UTMOS22Strong(Wav2Vec2Config(**TINY), emb_dim=16, lstm_hidden=32, proj_hidden=128)
    assert (wavlm.workspace_bytes(2, 40000), wavlm.workspace_bytes(1, 400)) == (3939840, 32256)
    assert (w2v.workspace_bytes(2, 40000), w2v.workspace_bytes(1, 400)) == (3568384, 29952)
    assert (utmos.workspace_bytes(2, 40000), utmos.workspace_bytes(1, 400)) == (4394752, 33792)
    plan_, total = utmos._plan(2, 40000)
    assert total * 4 == 4394752 and plan_["_up"][0] * 4 + w2v.workspace_bytes(2, 40000) == 4394752
    assert all(off % 64 == 0 for off, _ in list(wavlm._plan(2, 40000).values()) + list(w2v._plan(2, 40000).values()))
    wavlm.cfg, w2v.cfg = WavLMConfig(), Wav2Vec2Config()                  # the plan reads the configuration alone
    assert (wavlm.workspace_bytes(2, 40000), wavlm.workspace_bytes(1, 400)) == (60196352, 480000)
    assert (w2v.workspace_bytes(2, 40000), w2v.workspace_bytes(1, 400)) == (56820992, 468480)


def test_wav2vec2_geometry_is_its_own():
    """Wav2Vec2 raises the layer-0 pitch over the shared geometry and borrows nothing from WavLM."""
    from f5e_tts_amd.eval.wav2vec2 import Wav2Vec2, Wav2Vec2Config
    from f5e_tts_amd.eval.wavlm import WaveEncoder, WavLM
    m = Wav2Vec2(Wav2Vec2Config(**TINY))
    assert isinstance(m, WaveEncoder) and not isinstance(m, WavLM)
    assert m._geometry(400) == (1, [79, 39, 19, 9, 4, 2, 1], [128, 64, 32, 16, 8, 4, 2])
    assert m._geometry(40000) == (124, [7951, 3975, 1987, 993, 496, 248, 124], [8000, 4000, 2000, 1000, 500, 250, 125])
    assert m.frame_count(40000) == 124 and m.min_samples() == 400
