"""Monotonic alignment search, host side: tests/mas_ref.py equals the reference's own search on every fixture of
tests/golden/mas_paths.npz (written by tests/golden/make_mas_golden.py); the new C-ABI entries are declared, exported and
bound; the product path fails loudly without a GPU; lengths that start on the host are validated there; the DiT mirror
picks up the align-loss settings without touching its state_dict.  No kernel is launched here."""
import os
import re

import numpy as np
import pytest
import torch

import mas_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_restatement_equals_every_reference_path():
    cases = R.load_paths(os.path.join(GOLD, "mas_paths.npz"))
    assert len(cases) >= 4
    seen = set()
    for logp, ty, tx, path in cases:
        B, Ty, Tx = logp.shape
        tok, dur = R.mas_index(logp, ty, tx)
        assert np.array_equal(R.dense(tok, Tx), path)
        for b in range(B):
            assert dur[b].sum() == ty[b] and (dur[b, :tx[b]] >= 1).all() and (tok[b, ty[b]:] == -1).all()
            seen |= {"tx1"} if tx[b] == 1 else set()
            seen |= {"square"} if tx[b] == ty[b] else set()
            seen |= {"short"} if ty[b] < Ty else set()
        seen |= {"ragged"} if len(set(ty.tolist())) > 1 else set()
        seen |= {"off32"} if Tx % 32 else set()
        seen |= {"off64"} if Tx % 64 else set()
    assert seen == {"tx1", "square", "short", "ragged", "off32", "off64"}


def test_restatement_handles_ties_and_sequences_without_a_path():
    """A constant matrix is all ties: the strict comparison stays on the token, so the path leaves a token only where it
    must (i == y), i.e. the diagonal first and then the last token.  Degenerate lengths give -1 / 0 rows."""
    tok, dur = R.mas_index(np.zeros((3, 6, 4), np.float32), [6, 2, 5], [3, 3, 0])
    assert tok[0].tolist() == [0, 1, 2, 2, 2, 2] and dur[0].tolist() == [1, 1, 4, 0]
    assert (tok[1:] == -1).all() and (dur[1:] == 0).all()


def test_new_entries_are_declared_exported_and_bound():
    from f5e_tts_amd import _C
    text = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    lib = _C.lib()
    for name, arity in (("f5e_mas_path", 13), ("f5e_mas_workspace_bytes", 4)):
        m = re.search(r"F5E_API int " + name + r"\((.*?)\);", text, flags=re.S)
        assert m, f"{name} is not declared in f5e_abi.h"
        assert len(m.group(1).split(",")) == arity == len(_C.SIGNATURES[name])
        assert hasattr(lib, name)
    assert lib.f5e_abi_version() == _C.ABI_VERSION == 2
    assert "mas.hip" in open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "Makefile")).read()


def test_workspace_query_and_argument_checks_without_launching():
    import ctypes as C
    from f5e_tts_amd import _C, ops
    lib = _C.lib()
    assert ops.mas_workspace_bytes(1, 250, 60) == 250 * 8                     # one bit per cell, rows of whole 64-bit words
    assert ops.mas_workspace_bytes(8, 4096, 4096) == 8 * 4096 * 64 * 8
    assert ops.mas_workspace_bytes(2, 10, 65) == 2 * 10 * 2 * 8
    n = C.c_ulonglong()
    assert lib.f5e_mas_workspace_bytes(1, 16, 4097, C.byref(n)) == -1 and b"4096" in lib.f5e_last_error()
    p = C.c_void_p(8)
    assert lib.f5e_mas_path(None, p, 0, 60, p, p, p, None, p, 10 ** 6, 1, 100, 0) == -1          # Tx = 0
    assert lib.f5e_mas_path(None, p, 0, 59, p, p, p, None, p, 10 ** 6, 1, 100, 60) == -1         # ld < Tx
    assert lib.f5e_mas_path(None, p, 100, 60, p, p, p, None, p, 10 ** 6, 2, 100, 60) == -1       # overlapping batch stride
    assert lib.f5e_mas_path(None, p, 0, 60, p, p, p, None, p, 100 * 8 - 1, 1, 100, 60) == -1     # workspace too small
    assert b"workspace" in lib.f5e_last_error()
    assert lib.f5e_mas_path(None, p, 0, 60, p, p, None, None, p, 10 ** 6, 1, 100, 60) == -1      # no output


def test_product_path_raises_on_cpu_tensors():
    from f5e_tts_amd import _C, ops
    from f5e_tts_amd.model import monotonic_align as MA
    logp = torch.zeros(1, 6, 4)
    ty, tx = torch.tensor([6], dtype=torch.int32), torch.tensor([3], dtype=torch.int32)
    with pytest.raises(_C.F5EError):
        ops.mas_path(logp, ty, tx, torch.empty(1, 6, dtype=torch.int32))
    with pytest.raises(_C.F5EError, match="GPU"):
        MA.maximum_path(logp, torch.ones(1, 6, 4))
    with pytest.raises(_C.F5EError, match="GPU"):
        MA.maximum_path_index(logp, ty, tx)


@pytest.mark.parametrize("ty,tx", [([6], [7]), ([3], [4]), ([6], [0]), ([7], [3]), ([6], [5]), ([6, 6], [3, -1])])
def test_host_lengths_are_validated_on_the_host(ty, tx):
    """t_x > t_y, t_x < 1, t_y > Ty, t_x > Tx: caller bugs when the lengths are host values (device lengths get -1 / 0 rows)."""
    from f5e_tts_amd import _C
    from f5e_tts_amd.model import monotonic_align as MA
    with pytest.raises(_C.F5EError, match="1 <= t_x <= t_y"):
        MA.maximum_path_index(torch.zeros(len(ty), 6, 4), torch.tensor(ty), torch.tensor(tx))
    with pytest.raises(_C.F5EError, match="1 <= t_x <= t_y"):
        MA.check_lengths(ty, tx, len(ty), 6, 4)


def test_host_length_check_passes_good_lengths_and_counts_entries():
    from f5e_tts_amd import _C
    from f5e_tts_amd.model import monotonic_align as MA
    ty, tx = MA.check_lengths([6, 4], torch.tensor([4, 1]), 2, 6, 4)
    assert ty.tolist() == [6, 4] and tx.tolist() == [4, 1]
    with pytest.raises(_C.F5EError, match="one entry per sequence"):
        MA.check_lengths([6], [4, 1], 2, 6, 4)


def test_a_host_length_is_validated_even_when_the_other_one_is_on_a_device():
    """Mixed lengths (what DiT._block_len admits): whatever is known on the host is checked there, without touching the
    device tensor (a meta tensor stands in for it: reading it would raise)."""
    from f5e_tts_amd import _C
    from f5e_tts_amd.model import monotonic_align as MA
    on_device = torch.empty(2, dtype=torch.int32, device="meta")
    for bad_tx in ([4, 0], [5, 1], [4, -2]):
        with pytest.raises(_C.F5EError, match="1 <= t_x <= t_y"):
            MA.check_lengths(on_device, bad_tx, 2, 6, 4)
    for bad_ty in ([7, 6], [0, 6]):
        with pytest.raises(_C.F5EError, match="1 <= t_x <= t_y"):
            MA.check_lengths(bad_ty, on_device, 2, 6, 4)
    ty, tx = MA.check_lengths(on_device, [4, 1], 2, 6, 4)
    assert ty.device.type == "meta" and tx.tolist() == [4, 1]
    ty, tx = MA.check_lengths([6, 1], on_device, 2, 6, 4)
    assert tx.device.type == "meta" and ty.tolist() == [6, 1]


def test_dense_path_expansion():
    from f5e_tts_amd.model import monotonic_align as MA
    tok = torch.tensor([[0, 0, 1, 2, -1]], dtype=torch.int32)
    want = torch.tensor([[[1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0]]], dtype=torch.float16)
    got = MA.dense_path(tok, 3, torch.float16)
    assert got.dtype == torch.float16 and torch.equal(got, want)


def test_dit_reads_the_align_loss_settings_and_keeps_its_state_dict():
    from f5e_tts_amd import _C
    from f5e_tts_amd.model import DiT
    arch = dict(dim=256, depth=1, heads=4, ff_mult=1, mel_dim=20, text_num_embeds=30, text_dim=256, conv_layers=1)
    ppg = dict(use_ppg=True, ppg_dim=32)
    cb = dict(use_codebook=True, num_vars=20, temp_start=2, temp_stop=0.5, temp_decay=0.999995, groups=2,
              combine_groups=False, weight_proj_depth=1, weight_proj_factor=1)
    plain = DiT(**arch, ppg_config=ppg, cb_config=cb)
    assert plain.use_align_loss is False
    with_loss = DiT(**arch, ppg_config=ppg,
                    cb_config=dict(cb, use_align_loss=True, align_loss_config=dict(align_loss_weight=0.25)))
    assert with_loss.use_align_loss is True and with_loss.align_loss_weight == 0.25
    assert list(with_loss.state_dict()) == list(plain.state_dict())
    assert DiT(**arch).use_align_loss is False                      # the default cb_config has neither key
    z = np.load(os.path.join(GOLD, "mas_dit.npz"))
    kept = {k[2:]: tuple(z[k].shape) for k in z.files if k.startswith("w/")}
    mine = {k: tuple(v.shape) for k, v in with_loss.state_dict().items()}
    assert kept and all(mine[k] == s for k, s in kept.items())      # the fixture's reference tensors fit this mirror
    assert {k for k in mine if k.startswith(("text_embed.", "ppg_embed.", "quantizer."))} == set(kept)
    with_loss.train()
    with pytest.raises(NotImplementedError):
        with_loss.calc_align_loss(torch.zeros(1, 4, 4), torch.zeros(1, 4, 256), torch.tensor([4]), torch.zeros(1, 4, 256))
    with pytest.raises(_C.F5EError):
        DiT(**arch).eval().calc_align_loss(torch.zeros(1, 4, 4), torch.zeros(1, 4, 256), torch.tensor([4]),
                                           torch.zeros(1, 4, 256))
    with pytest.raises(NotImplementedError):
        with_loss(torch.zeros(1))


def test_cfm_align_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from f5e_tts_amd import _C
    from f5e_tts_amd.model import CFM, DiT
    dit = DiT(dim=256, depth=1, heads=4, ff_mult=1, mel_dim=20, text_num_embeds=30, text_dim=256, conv_layers=1,
              ppg_config=dict(use_ppg=True, ppg_dim=32))
    cfm = CFM(transformer=dit, mel_spec_kwargs=dict(n_mel_channels=20), ppg_config=dict(use_ppg=True))
    with pytest.raises(_C.F5EError):
        cfm.align(torch.zeros(1, 3, dtype=torch.long), torch.zeros(1, 8, 32))
