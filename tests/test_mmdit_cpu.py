"""MMDiT (reference model/backbones/mmdit.py) on the host: the mirror's state_dict layout and checkpoint loading against
reference-generated fixtures (tests/golden/make_mmdit_golden.py), and the fp32 restatement (tests/mmdit_ref.py) the GPU
tests compare with, pinned to the reference's own outputs."""
import os

import numpy as np
import pytest
import torch

import mmdit_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = dict(rtol=1e-4, atol=2e-5)  # fp32 vs fp32, as tests/test_oracle_golden.py

# tag -> constructor arguments of the fixture (make_mmdit_golden.CASES)
ARCH = {
    "b1": dict(dim=64, depth=3, heads=2, dim_head=64, ff_mult=1, mel_dim=20, text_num_embeds=30, text_mask_padding=True,
               qk_norm=None),
    "b2_rms": dict(dim=64, depth=3, heads=2, dim_head=64, ff_mult=1, mel_dim=20, text_num_embeds=30,
                   text_mask_padding=False, qk_norm="rms_norm"),
}


def fixture(tag):
    z = np.load(os.path.join(GOLD, f"mmdit_{tag}.npz"), allow_pickle=False)
    g = {k: torch.from_numpy(z[k]) for k in z.files}
    sd = {k[2:]: v.float() for k, v in g.items() if k.startswith("w/")}
    return g, sd


@pytest.mark.parametrize("tag", sorted(ARCH))
def test_mmdit_state_dict_layout_matches_reference(tag):
    from f5e_tts_amd.model import MMDiT
    _, sd = fixture(tag)
    m = MMDiT(**ARCH[tag])
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    assert list(m.state_dict()) == list(sd)          # the reference's registration order too
    m.load_state_dict(sd, strict=True)


def test_mmdit_last_block_is_context_pre_only_and_zero_init():
    from f5e_tts_amd.model import MMDiT
    from f5e_tts_amd.model.modules import AdaLayerNorm, AdaLayerNorm_Final
    m = MMDiT(dim=512, depth=16, heads=16, ff_mult=2)     # the count script's size (scripts/count_params_gflops.py)
    blocks = m.transformer_blocks
    assert all(isinstance(b.attn_norm_c, AdaLayerNorm) and b.ff_c is not None for b in blocks[:-1])
    last = blocks[-1]
    assert last.context_pre_only and isinstance(last.attn_norm_c, AdaLayerNorm_Final)
    assert last.ff_norm_c is None and last.ff_c is None and not hasattr(last.attn, "to_out_c")
    sd = m.state_dict()
    for k in ("transformer_blocks.15.attn_norm_c.linear.weight", "transformer_blocks.0.attn_norm_x.linear.bias",
              "norm_out.linear.weight", "proj_out.weight", "proj_out.bias"):
        assert float(sd[k].abs().max()) == 0, k
    m.clear_cache()
    assert m.text_cond is None and m.text_uncond is None


@pytest.mark.parametrize("tag", sorted(ARCH))
def test_mmdit_restatement_matches_reference(tag):
    g, sd = fixture(tag)
    for da in (False, True):
        for dt in (False, True):
            out = R.mmdit_forward(sd, ARCH[tag]["heads"], g["x"], g["cond"], g["text"], g["time"], da, dt, g.get("mask"),
                                  text_mask_padding=ARCH[tag]["text_mask_padding"])
            torch.testing.assert_close(out, g[f"pred_a{int(da)}_t{int(dt)}"], **TOL)


@pytest.mark.parametrize("use_ema", [True, False])
def test_load_model_loads_an_mmdit_checkpoint_strictly(tmp_path, use_ema):
    from f5e_tts_amd.infer.utils_infer import load_model
    from f5e_tts_amd.model import MMDiT
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("".join(f"{chr(97 + i)}\n" for i in range(20)), encoding="utf-8")
    cfg = dict(dim=64, depth=2, heads=2, ff_mult=1)
    src = MMDiT(**cfg, text_num_embeds=20, mel_dim=100)
    g = torch.Generator().manual_seed(5)
    for p in src.parameters():
        p.data.copy_(torch.randn(p.shape, generator=g))
    state = {"transformer." + k: v for k, v in src.state_dict().items()}
    if use_ema:
        ckpt = {"ema_model_state_dict": {**{"ema_model." + k: v for k, v in state.items()},
                                         "initted": torch.tensor(True), "step": torch.tensor(7)}}
    else:
        ckpt = {"model_state_dict": state}
    path = tmp_path / "model.pt"
    torch.save(ckpt, path)
    model = load_model(MMDiT, cfg, str(path), vocab_file=str(vocab), use_ema=use_ema, device="cpu")
    assert isinstance(model.transformer, MMDiT)
    got = model.transformer.state_dict()
    assert list(got) == list(src.state_dict())
    for k, v in src.state_dict().items():
        assert torch.equal(got[k], v), k


def test_self_attention_members_are_unchanged():
    """Attention without context_dim (every DiT / UNetT block) keeps exactly its members; with context_dim the joint members
    follow in the reference's order (modules.py:360-416)."""
    from f5e_tts_amd.model.modules import Attention, AttnProcessor, JointAttnProcessor
    for qk_norm in (None, "rms_norm"):
        a = Attention(AttnProcessor(), dim=128, heads=2, qk_norm=qk_norm)
        norms = ["q_norm", "k_norm"] if qk_norm else []
        assert [n for n, _ in a.named_children()] == ["to_q", "to_k", "to_v", *norms, "to_out"]
        assert sorted(vars(a)) == sorted(vars(Attention(AttnProcessor(), dim=128, heads=2, qk_norm=qk_norm)))
        assert not hasattr(a, "context_dim") and not hasattr(a, "to_q_c") and not hasattr(a, "to_out_c")
        assert a.q_norm is None if qk_norm is None else a.q_norm is not None
        for pre_only in (False, True):
            j = Attention(JointAttnProcessor(), dim=128, heads=2, context_dim=64, context_pre_only=pre_only,
                          qk_norm=qk_norm)
            cnorms = ["c_q_norm", "c_k_norm"] if qk_norm else []
            assert [n for n, _ in j.named_children()] == ["to_q", "to_k", "to_v", *norms, "to_q_c", "to_k_c", "to_v_c",
                                                          *cnorms, "to_out", *([] if pre_only else ["to_out_c"])]
            assert j.to_q_c.weight.shape == (128, 64)
            if not pre_only:
                assert j.to_out_c.weight.shape == (64, 128)
