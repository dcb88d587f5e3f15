"""Monotonic alignment search on the GPU (csrc/mas.hip through ops.mas_path / model.monotonic_align) and the layers above it
(DiT.align_text_ppg, DiT.calc_align_loss, CFM.align) against
  * the REFERENCE's own search and DiT methods (tests/golden/mas_paths.npz, mas_dit.npz; tests/golden/make_mas_golden.py
    asserts that no stored decision flips under +-1e-3 noise), and
  * the NumPy restatement (tests/mas_ref.py, pinned by the same fixtures) on shapes the reference's Python loop cannot cover.
Paths are discrete: every comparison of a path is exact.  The loss is compared at the fp32-GEMM tolerance of
tests/test_ops_gpu.py::test_gemm_f32 (rtol 1e-5, atol 3e-5 for unit-size values), scaled by the size of the value."""
import os

import numpy as np
import pytest
import torch

import mas_ref as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
I32 = torch.int32


@pytest.fixture(scope="module")
def ops():
    import f5e_tts_amd.ops as ops_mod
    ops_mod.require_device()
    return ops_mod


def i32(v):
    return torch.as_tensor(np.asarray(v), dtype=I32).cuda()


def seeded(B, Ty, Tx, seed):
    return torch.randn(B, Ty, Tx, generator=torch.Generator().manual_seed(seed)) * 3.0 - 4.0


def check_against_restatement(ops, logp_dev, logp_host, ty, tx):
    """Kernel == restatement, exactly; durations consistent with token_of_frame; logp untouched."""
    B, Ty, Tx = logp_dev.shape
    before = logp_dev.clone()
    tok = torch.full((B, Ty), -7, dtype=I32, device="cuda")
    dur = torch.full((B, Tx), -7, dtype=I32, device="cuda")
    ops.mas_path(logp_dev, i32(ty), i32(tx), tok, dur)
    torch.cuda.synchronize()
    want_tok, want_dur = R.mas_index(logp_host.numpy(), ty, tx)
    tok, dur = tok.cpu().numpy(), dur.cpu().numpy()
    assert np.array_equal(tok, want_tok), f"token_of_frame differs in {(tok != want_tok).sum()} frames"
    assert np.array_equal(dur, want_dur)
    for b in range(B):
        assert dur[b].sum() == ty[b] and np.array_equal(dur[b], np.bincount(tok[b, :ty[b]], minlength=Tx))
    assert torch.equal(logp_dev, before)          # bit-unchanged (the reference accumulates in place; we do not)
    return tok, dur


# ------------------------------------------------------------------ the kernel against the reference's paths

def test_kernel_equals_the_reference_paths_dense_and_index_form(ops):
    from f5e_tts_amd.model import monotonic_align as MA
    for logp, ty, tx, path in R.load_paths(os.path.join(GOLD, "mas_paths.npz")):
        B, Ty, Tx = logp.shape
        dev = torch.from_numpy(logp).cuda()
        # index form, device lengths
        tok, dur = MA.maximum_path_index(dev, i32(ty), i32(tx))
        assert tok.dtype == I32 and dur.dtype == I32 and tok.shape == (B, Ty) and dur.shape == (B, Tx)
        assert np.array_equal(R.dense(tok.cpu().numpy(), Tx), path)
        want_tok, want_dur = R.mas_index(logp, ty, tx)
        assert np.array_equal(tok.cpu().numpy(), want_tok) and np.array_equal(dur.cpu().numpy(), want_dur)
        # index form, host lengths (validated there)
        tok_h, dur_h = MA.maximum_path_index(dev, torch.from_numpy(ty), tx.tolist())
        assert torch.equal(tok_h, tok) and torch.equal(dur_h, dur)
        # dense form, the reference's signature: lengths from the outer-product mask
        my = torch.arange(Ty)[None, :] < torch.from_numpy(ty)[:, None]
        mx = torch.arange(Tx)[None, :] < torch.from_numpy(tx)[:, None]
        mask = (my[:, :, None] & mx[:, None, :]).float().cuda()
        dense = MA.maximum_path(dev, mask)
        assert dense.shape == dev.shape and dense.dtype == dev.dtype and dense.device == dev.device
        assert np.array_equal(dense.cpu().numpy().astype(np.uint8), path)
        assert torch.equal(dev.cpu(), torch.from_numpy(logp))
        # half-precision input: searched in float32 like the reference, returned in the input's dtype
        half = MA.maximum_path(dev.half(), mask.half())
        ref_half, _ = R.mas_index(dev.half().float().cpu().numpy(), ty, tx)
        assert half.dtype == torch.float16 and np.array_equal(half.cpu().numpy().astype(np.uint8), R.dense(ref_half, Tx))


# ------------------------------------------------------------------ the kernel against the restatement, larger shapes

def test_kernel_equals_restatement_ragged_1000x180(ops):
    logp = seeded(3, 1000, 180, 61)
    check_against_restatement(ops, logp.cuda(), logp, [1000, 733, 181], [180, 97, 180])


def test_kernel_equals_restatement_4096x700(ops):
    logp = seeded(2, 4096, 700, 62)
    check_against_restatement(ops, logp.cuda(), logp, [4096, 3111], [700, 513])


def test_kernel_equals_restatement_4096x4096_square_and_wide(ops):
    """t_x = t_y = 4096: the band is one cell wide, the path is the diagonal and every decision is the forced one; the same
    matrix with 3000 tokens exercises all 16 waves with real decisions."""
    logp = seeded(1, 4096, 4096, 63)
    dev = logp.cuda()
    tok, _ = check_against_restatement(ops, dev, logp, [4096], [4096])
    assert np.array_equal(tok[0], np.arange(4096))
    check_against_restatement(ops, dev, logp, [4096], [3000])
    check_against_restatement(ops, dev, logp, [4000], [257])


@pytest.mark.parametrize("Tx", [63, 64, 65, 127, 128, 129, 255, 256, 257])
def test_kernel_equals_restatement_across_slot_and_wave_boundaries(ops, Tx):
    """Tx around 64, 128 and 256 columns: one, two and four slots per lane, then the step from one wave to several (the dispatch
    ladder of f5e_mas_path); the second sequence is shorter in both directions."""
    Ty = Tx + 37
    logp = seeded(2, Ty, Tx, 70 + Tx)
    check_against_restatement(ops, logp.cuda(), logp, [Ty, Ty - 5], [Tx, Tx - 1])


@pytest.mark.parametrize("Ty", [5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129])
def test_kernel_equals_restatement_across_prefetch_and_backtrack_rounds(ops, Ty):
    """Five tokens, Ty around the prefetch depth (8 rows per register set, 16 per turn of the row pipeline) and around the
    64 rows that one backtrack round resolves."""
    logp = seeded(2, Ty, 5, 400 + Ty)
    check_against_restatement(ops, logp.cuda(), logp, [Ty, Ty - 5 if Ty > 9 else Ty], [5, 4])


def test_kernel_on_a_strided_batch_with_ld_above_tx(ops):
    """A column-sliced view (ld = 200 > Tx = 130) of every other matrix of a batch (batch stride = 2 matrices)."""
    big = seeded(4, 300, 200, 64).cuda()
    view = big[::2, :, :130]
    assert view.stride() == (2 * 300 * 200, 200, 1)
    check_against_restatement(ops, view, view.cpu().contiguous(), [300, 250], [130, 64])
    big2 = seeded(2, 90, 72, 65).cuda()                       # one wave, two slots, ld not a multiple of 4 elements away
    view2 = big2[:, 3:, 1:70]
    check_against_restatement(ops, view2, view2.cpu().contiguous(), [87, 40], [69, 40])


def test_ties_stay_on_the_token(ops):
    """A constant matrix is all ties: the strict comparison leaves a token only where it must."""
    logp = torch.zeros(2, 300, 100)
    tok, dur = check_against_restatement(ops, logp.cuda(), logp, [300, 100], [100, 1])
    assert tok[0, :100].tolist() == list(range(100)) and (tok[0, 100:] == 99).all() and (tok[1, :100] == 0).all()


def test_degenerate_device_lengths_give_defined_rows_and_leave_the_rest_alone(ops):
    """t_x < 1, t_y < t_x and lengths beyond the matrix have no monotonic path: -1 / 0 rows; the valid sequences of the same
    batch get exactly what they get alone."""
    logp = seeded(6, 120, 90, 66)
    ty = [120, 0, 50, 121, 90, 77]
    tx = [90, 5, 51, 10, 91, 0]
    valid = [0]
    dev = logp.cuda()
    tok = torch.full((6, 120), -7, dtype=I32, device="cuda")
    dur = torch.full((6, 90), -7, dtype=I32, device="cuda")
    ops.mas_path(dev, i32(ty), i32(tx), tok, dur)
    torch.cuda.synchronize()
    want_tok, want_dur = R.mas_index(logp.numpy(), ty, tx)
    assert np.array_equal(tok.cpu().numpy(), want_tok) and np.array_equal(dur.cpu().numpy(), want_dur)
    for b in range(6):
        if b not in valid:
            assert (tok[b] == -1).all() and (dur[b] == 0).all()
    alone_tok = torch.empty(1, 120, dtype=I32, device="cuda")
    ops.mas_path(dev[:1], i32(ty[:1]), i32(tx[:1]), alone_tok)          # durations are optional
    assert torch.equal(alone_tok[0], tok[0]) and int(dur[0].sum()) == 120
    ty2, tx2 = [120, 100, 60, 120, 90, 77], [90, 5, 60, 1, 90, 33]       # all valid: every row changes, none is stale
    check_against_restatement(ops, dev, logp, ty2, tx2)


def test_wrapper_rejects_what_the_kernel_cannot_take(ops):
    from f5e_tts_amd import _C
    logp = torch.zeros(1, 8, 4, device="cuda")
    ty, tx = i32([8]), i32([4])
    with pytest.raises(_C.F5EError):
        ops.mas_path(logp.cpu(), ty, tx, torch.empty(1, 8, dtype=I32, device="cuda"))
    with pytest.raises(_C.F5EError):
        ops.mas_path(logp, ty.cpu(), tx, torch.empty(1, 8, dtype=I32, device="cuda"))
    with pytest.raises(_C.F5EError):
        ops.mas_path(logp, ty, tx, torch.empty(1, 7, dtype=I32, device="cuda"))
    with pytest.raises(_C.F5EError):
        ops.mas_path(logp, ty, tx, torch.empty(1, 8, dtype=I32, device="cuda"),
                     workspace=torch.empty(7, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_C.F5EError):
        ops.mas_path(torch.zeros(1, 8, 4097, device="cuda"), ty, tx, torch.empty(1, 8, dtype=I32, device="cuda"))


def test_captured_once_and_replayed_with_new_contents_and_lengths(ops):
    """One stream, a linear graph (f5e_graph_*): the launch reads matrix and lengths from the same buffers at replay time."""
    B, Ty, Tx = 2, 400, 150
    first, second = seeded(B, Ty, Tx, 67), seeded(B, Ty, Tx, 68)
    lens = (([400, 300], [150, 20]), ([222, 400], [150, 149]))
    logp = torch.empty(B, Ty, Tx, device="cuda")
    ty, tx = torch.zeros(B, dtype=I32, device="cuda"), torch.zeros(B, dtype=I32, device="cuda")
    tok, dur = torch.zeros(B, Ty, dtype=I32, device="cuda"), torch.zeros(B, Tx, dtype=I32, device="cuda")
    ws = torch.empty(ops.mas_workspace_bytes(B, Ty, Tx), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = ops.Graph()
        g.begin()
        try:
            ops.mas_path(logp, ty, tx, tok, dur, workspace=ws)
        finally:
            g.end()
        for mat, (a, b) in zip((first, second), lens):
            logp.copy_(mat)
            ty.copy_(torch.tensor(a, dtype=I32))
            tx.copy_(torch.tensor(b, dtype=I32))
            g.launch()
            s.synchronize()
            want_tok, want_dur = R.mas_index(mat.numpy(), a, b)
            assert np.array_equal(tok.cpu().numpy(), want_tok) and np.array_equal(dur.cpu().numpy(), want_dur)
        g.destroy()


# ------------------------------------------------------------------ DiT / CFM against the reference fixture

def dit_fixture():
    from f5e_tts_amd.model import CFM, DiT
    z = np.load(os.path.join(GOLD, "mas_dit.npz"))
    ppg_config = dict(use_ppg=True, ppg_dim=32, use_transformer=False, transformer_config=dict(), use_cross_mask=False)
    cb_config = dict(use_codebook=True, num_vars=20, temp_start=2, temp_stop=0.5, temp_decay=0.999995, groups=2,
                     combine_groups=False, weight_proj_depth=1, weight_proj_factor=1, use_align_loss=True,
                     align_loss_config=dict(align_loss_weight=float(z["align_loss_weight"])))
    torch.manual_seed(1)
    dit = DiT(dim=256, depth=1, heads=4, dim_head=64, ff_mult=1, mel_dim=20, text_num_embeds=30, text_dim=256,
              conv_layers=1, text_mask_padding=False, ppg_config=ppg_config, cb_config=cb_config)
    sd = dit.state_dict()
    ref = {k[2:]: torch.from_numpy(z[k]).to(sd[k[2:]].dtype) for k in z.files if k.startswith("w/")}
    assert ref and set(ref) <= set(sd)
    sd.update(ref)                    # the transformer blocks keep their own init: the alignment never reads them
    dit.load_state_dict(sd, strict=True)
    cfm = CFM(transformer=dit, mel_spec_kwargs=dict(n_mel_channels=20), ppg_config=ppg_config, cb_config=cb_config)
    return z, dit, cfm.cuda().eval()


def test_dit_align_text_ppg_equals_the_reference_attn(ops):
    z, dit, _ = dit_fixture()
    te, pe = torch.from_numpy(z["text_embed"]).cuda(), torch.from_numpy(z["ppg_embed"]).cuda()
    want = torch.from_numpy(z["attn"]).float()
    for lens in ((torch.from_numpy(z["text_len"]), torch.from_numpy(z["ppg_len"])),                   # host: the block
                 (torch.from_numpy(z["text_len"]).cuda(), torch.from_numpy(z["ppg_len"]).cuda())):    # device: all n
        attn = dit.align_text_ppg(te, lens[0], pe, lens[1])
        assert attn.shape == want.shape and attn.dtype == te.dtype and attn.is_cuda
        assert torch.equal(attn.cpu(), want)
    tok, dur = dit.align_index(te, torch.from_numpy(z["text_len"]), pe, torch.from_numpy(z["ppg_len"]))
    assert tok.shape == (2, int(z["ppg_len"].max())) and dur.shape == (2, int(z["text_len"].max()))
    assert torch.equal(dur.cpu().float(), want.sum(-1)[:, :dur.shape[1]])
    # the likelihood matrix itself, against the formula in fp64 (values are O(100): fp32-GEMM tolerance at that size)
    lp = dit.align_logp(te, pe, 48, 13).double().cpu()
    t64, p64 = torch.from_numpy(z["text_embed"]).double()[:, :13], torch.from_numpy(z["ppg_embed"]).double()
    ref = (-0.5 * np.log(2 * np.pi) * 256 - 0.5 * (p64 ** 2).sum(-1)[:, :, None] + p64 @ t64.transpose(1, 2)
           - 0.5 * (t64 ** 2).sum(-1)[:, None, :])
    err, size = float((lp - ref).abs().max()), float(ref.abs().max())
    print(f"align_logp: max abs err {err:.3e} at magnitude {size:.3e}")
    assert err <= (3e-5 + 1e-5) * size


def test_dit_calc_align_loss_matches_the_reference_value(ops):
    z, dit, _ = dit_fixture()
    dit = dit.cuda().eval()
    te, pe = torch.from_numpy(z["text_embed"]).cuda(), torch.from_numpy(z["ppg_embed"]).cuda()
    attn = torch.from_numpy(z["attn"]).float().cuda()
    loss = dit.calc_align_loss(attn, te, torch.from_numpy(z["text_len"]), pe)
    want = float(z["loss"])
    print(f"calc_align_loss: {float(loss):.9e} vs reference {want:.9e}, diff {abs(float(loss) - want):.3e}")
    assert loss.ndim == 0 and abs(float(loss) - want) <= 1e-5 * abs(want) + 3e-5 * abs(want)
    again = dit.calc_align_loss(dit.align_text_ppg(te, z["text_len"].tolist(), pe, z["ppg_len"].tolist()), te,
                                torch.from_numpy(z["text_len"]).cuda(), pe)
    assert float(again) == float(loss)
    dit.train()
    with pytest.raises(NotImplementedError):
        dit.calc_align_loss(attn, te, torch.from_numpy(z["text_len"]), pe)


def test_cfm_align_end_to_end_gives_the_reference_alignment(ops):
    """ids and PPGs in, alignment out: text / PPG embeddings by the HIP engine at seq_len = the PPG length, the likelihood
    matrix and the search on the device."""
    z, dit, cfm = dit_fixture()
    want = torch.from_numpy(z["attn"]).float()                                  # [b, token, frame]
    text, ppg = torch.from_numpy(z["text"]), torch.from_numpy(z["ppg"]).cuda()
    eng = dit.engine()
    for name, mine in (("text_embed", eng.text_embed(text, 2, 48, False)), ("ppg_embed", eng.ppg_embed(ppg, 2, 48, False))):
        ref = torch.from_numpy(z[name])
        print(f"{name}: rel L2 to the reference {float((mine.cpu() - ref).norm() / ref.norm()):.3e}")
    al = cfm.align(text, ppg, ppg_lens=torch.from_numpy(z["ppg_len"]))
    tok, dur, text_len, ppg_len = al
    assert text_len.tolist() == z["text_len"].tolist() and ppg_len.tolist() == z["ppg_len"].tolist()
    assert tok.dtype == I32 and dur.dtype == I32 and tok.is_cuda
    Tx = int(z["text_len"].max())
    assert np.array_equal(R.dense(tok.cpu().numpy(), Tx), want[:, :Tx, :tok.shape[1]].transpose(1, 2).numpy().astype(np.uint8))
    assert torch.equal(al.durations.cpu().float(), want.sum(-1)[:, :Tx])
    # device ids are passed through (lengths then stay on the device as well)
    al2 = cfm.align(text.cuda(), ppg, ppg_lens=torch.from_numpy(z["ppg_len"]).cuda())
    assert torch.equal(al2.token_of_frame[:, :tok.shape[1]], tok) and torch.equal(al2.durations[:, :Tx], dur)
    # a text longer than its PPG has no alignment: host lengths -> an error, not a row of -1
    from f5e_tts_amd import _C
    with pytest.raises(_C.F5EError, match="1 <= t_x <= t_y"):
        cfm.align(text, ppg, ppg_lens=[48, 5])
