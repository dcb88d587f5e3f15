"""MMDiT on the MI355X: f5e_joint_attn against an fp32 softmax over the concatenated audio + text keys, its numerics when a
late key towers over a wave's first step, and MMDiT.forward on the HIP kernels against the fp32 restatement
(tests/mmdit_ref.py, pinned to the reference by tests/test_mmdit_cpu.py)."""
import math

import pytest
import torch

import mmdit_ref as R
from test_ops_gpu import QSCALE, close, pack_qkv

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    import f5e_tts_amd.ops as ops_mod
    ops_mod.require_device()
    return ops_mod


def g(seed):
    return torch.Generator().manual_seed(seed)


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm())


def joint_ref(qx, kx, vx, qc, kc, vc, lens):
    """fp32 softmax over keys = audio (masked past lens) ++ text (never masked); q pre-scaled by log2(e) / 8."""
    S, H, N, _ = qx.shape
    Nt = qc.shape[2]
    q = torch.cat([qx, qc], 2).float()
    k = torch.cat([kx, kc], 2).float()
    v = torch.cat([vx, vc], 2).float()
    s = (q @ k.transpose(-1, -2)) * math.log(2.0)            # 2^(q' k) = e^(q k / 8)
    if lens is not None:
        km = torch.cat([torch.arange(N)[None, :] < lens[:, None], torch.ones(S, Nt, dtype=torch.bool)], 1)
        s = s.masked_fill(~km[:, None, None, :], float("-inf"))
    o = (torch.softmax(s, -1) @ v).transpose(1, 2)           # [S, N + Nt, H, 64]
    return o[:, :N].reshape(S * N, H * 64), o[:, N:].reshape(S * Nt, H * 64)


def stream(S, H, n, seed):
    q = (torch.randn(S, H, n, 64, generator=g(seed)) * QSCALE).to(BF)
    k = torch.randn(S, H, n, 64, generator=g(seed + 1)).to(BF)
    v = torch.randn(S, H, n, 64, generator=g(seed + 2)).to(BF)
    return q, k, v


def pad64(n):
    return (n + 63) // 64 * 64


def run_joint(ops, x, c, N, Nt, lens, waves, with_c, bufs=None):
    S, H = x[0].shape[:2]
    bx, bc = bufs if bufs else (pack_qkv(ops, *x, pad64(N)), pack_qkv(ops, *c, pad64(Nt)))
    out_x = torch.empty(S * N, H * 64, device="cuda", dtype=BF)
    out_c = torch.empty(S * Nt, H * 64, device="cuda", dtype=BF) if with_c else None
    ops.joint_attn(*bx, *bc, out_x, out_c, N, Nt, kv_len=lens.cuda() if lens is not None else None, waves=waves)
    return out_x, out_c


# (S, H, N, Nt, waves, ragged, with_c): every N, Nt, H, S, split count and both o_c forms appear
CASES = [(1, 2, 33, 1, 0, False, True), (2, 2, 33, 13, 1, True, True), (1, 16, 469, 200, 0, False, True),
         (2, 16, 469, 100, 4, True, False), (2, 2, 469, 32, 2, True, True), (1, 2, 938, 13, 4, False, True),
         (2, 16, 938, 200, 0, True, True), (2, 16, 938, 100, 0, True, False), (1, 16, 938, 200, 1, False, True),
         (2, 2, 33, 200, 4, True, True), (1, 2, 469, 1, 2, False, False), (2, 16, 33, 32, 0, True, True),
         (2, 2, 938, 1, 1, True, True), (1, 16, 469, 13, 2, False, True)]


@pytest.mark.parametrize("S,H,N,Nt,waves,ragged,with_c", CASES)
def test_joint_attn(ops, S, H, N, Nt, waves, ragged, with_c):
    x, c = stream(S, H, N, 40), stream(S, H, Nt, 50)
    lens = torch.tensor([N - 29 * i for i in range(S)], dtype=torch.int32) if ragged else None
    ref_x, ref_c = joint_ref(*x, *c, lens)
    out_x, out_c = run_joint(ops, x, c, N, Nt, lens, waves, with_c)
    close(out_x, ref_x, 2 ** -6, 6e-3, f"joint attention, audio queries ({waves} splits)")
    if with_c:
        close(out_c, ref_c, 2 ** -6, 6e-3, f"joint attention, text queries ({waves} splits)")


@pytest.mark.parametrize("waves", [0, 1, 2, 4])
def test_joint_attn_ignores_pad_rows(ops, waves):
    """Non-zero garbage in the pad rows of both streams' K and V buffers (positions past N / Nt, what a reused workspace
    may hold) must not change the output by a single bit: each segment masks its own tail before the softmax.  (Q pad rows
    are left zero, as the QKV GEMM leaves them: their lanes' row sums take part in the wave-wide fast-path test.)"""
    S, H, N, Nt = 2, 2, 100, 13
    x, c = stream(S, H, N, 60), stream(S, H, Nt, 70)
    lens = torch.tensor([N, 71], dtype=torch.int32)
    clean = run_joint(ops, x, c, N, Nt, lens, waves, True)
    bx, bc = pack_qkv(ops, *x, pad64(N)), pack_qkv(ops, *c, pad64(Nt))
    for bufs, n in ((bx, N), (bc, Nt)):
        n_pad = pad64(n)
        for t, index in ((bufs[1], ops.qk_frag_index), (bufs[2], ops.v_frag_index)):
            pad_idx = index(n_pad)[n:].reshape(-1).cuda()
            flat = t.view(S, H, n_pad * 64)
            flat[:, :, pad_idx] = (torch.rand(S, H, pad_idx.numel(), device="cuda") * 6 + 3).to(BF)
    dirty = run_joint(ops, x, c, N, Nt, lens, waves, True, bufs=(bx, bc))
    assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1], dirty[1])
    ref_x, ref_c = joint_ref(*x, *c, lens)
    close(dirty[0], ref_x, 2 ** -6, 6e-3, "audio queries, poisoned pads")
    close(dirty[1], ref_c, 2 ** -6, 6e-3, "text queries, poisoned pads")


@pytest.mark.parametrize("factor", [1.5, 4.0, 12.0])
def test_joint_attn_spike_forces_rescale(ops, factor):
    """The running maximum is taken from a wave's FIRST 64-key step (attention.hip); the text segment comes after the
    audio segment and can tower over it.  Spikes in the text segment, in the last (partial) audio step and in the masked
    audio tail: factor 1.5 (~17 octaves above the first step) stays on the fast path, 4 (~46) trips the 2^24 row-sum limit,
    12 (~138) overflows exp2 to inf first.  Every split count; the output stays finite and matches."""
    S, H, N, Nt = 1, 1, 300, 100
    x0 = torch.randn(S, H, N, 64, generator=g(80))
    c0 = torch.randn(S, H, Nt, 64, generator=g(81))
    kx = torch.randn(S, H, N, 64, generator=g(82)).to(BF)
    kc = torch.randn(S, H, Nt, 64, generator=g(83)).to(BF)
    vx = torch.randn(S, H, N, 64, generator=g(84)).to(BF)
    vc = torch.randn(S, H, Nt, 64, generator=g(85)).to(BF)
    qx, qc = (x0 * QSCALE).to(BF), (c0 * QSCALE).to(BF)
    kc[0, 0, 70] = (x0[0, 0, 17] * factor).to(BF)    # text key towering for audio query 17
    kc[0, 0, 5] = (c0[0, 0, 40] * factor).to(BF)     # text key towering for text query 40
    kx[0, 0, 290] = (x0[0, 0, 99] * factor).to(BF)   # last audio step (keys 256 .. 294 valid)
    kx[0, 0, 297] = (c0[0, 0, 3] * factor).to(BF)    # masked audio tail: must stay invisible
    lens = torch.tensor([295], dtype=torch.int32)
    ref_x, ref_c = joint_ref(qx, kx, vx, qc, kc, vc, lens)
    for splits in (1, 2, 4, 0):
        out_x, out_c = run_joint(ops, (qx, kx, vx), (qc, kc, vc), N, Nt, lens, splits, True)
        assert torch.isfinite(out_x.float()).all() and torch.isfinite(out_c.float()).all()
        close(out_x, ref_x, 2 ** -6, 6e-3, f"joint spike x{factor}, audio queries, {splits} splits")
        close(out_c, ref_c, 2 ** -6, 6e-3, f"joint spike x{factor}, text queries, {splits} splits")


def test_joint_attn_rejects_bad_arguments(ops):
    from f5e_tts_amd import _C
    x, c = stream(1, 2, 40, 90), stream(1, 2, 9, 91)
    bx, bc = pack_qkv(ops, *x, 64), pack_qkv(ops, *c, 64)
    out_x = torch.empty(40, 128, device="cuda", dtype=BF)
    with pytest.raises(_C.F5EError):
        ops.joint_attn(*bx, *bc, out_x, None, 40, 9, waves=3)
    with pytest.raises(_C.F5EError):
        ops.joint_attn(*bx, *bc, out_x, None, 40, 65)      # Nt past the text buffer's padding


# ---------------------------------------------------------------- MMDiT.forward

def make_mmdit(seed, **arch):
    from f5e_tts_amd.model import MMDiT
    torch.manual_seed(seed)
    m = MMDiT(**arch)
    gen = g(seed + 1)
    for p in m.parameters():   # the AdaLN-zero tensors (and proj_out) would make the output exactly 0
        if float(p.detach().abs().max()) == 0.0:
            p.data.copy_(torch.randn(p.shape, generator=gen) * 0.02)
    return m


def inputs(B, N, nt, mel, vocab, seed):
    gen = g(seed)
    x, cond = torch.randn(B, N, mel, generator=gen), torch.randn(B, N, mel, generator=gen)
    text = torch.randint(0, vocab, (B, nt), generator=gen)
    mask = None
    if B > 1:
        text[1, nt - 5:] = -1
        mask = torch.arange(N)[None] < torch.tensor([N, N - 23])[:, None]
    return x, cond, text, mask


@pytest.mark.parametrize("B,qk_norm,tmp", [(1, None, True), (2, None, True), (1, "rms_norm", False), (2, "rms_norm", True)])
def test_mmdit_forward(B, qk_norm, tmp):
    arch = dict(dim=256, depth=3, heads=4, dim_head=64, ff_mult=2, mel_dim=100, text_num_embeds=60,
                text_mask_padding=tmp, qk_norm=qk_norm)
    m = make_mmdit(71, **arch)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    N, nt = 90, 17
    x, cond, text, mask = inputs(B, N, nt, 100, 60, 72)
    m = m.cuda().eval()
    time = torch.tensor(0.3)
    for da, dt in ((False, False), (True, False), (False, True), (True, True)):
        ref = R.mmdit_forward(sd, 4, x, cond, text, time, da, dt, mask, text_mask_padding=tmp)
        out = m(x.cuda(), cond.cuda(), text.cuda(), time.cuda(), da, dt, mask.cuda() if mask is not None else None)
        assert out.shape == ref.shape
        assert rel_l2(out, ref) < 1e-2, (B, qk_norm, da, dt, rel_l2(out, ref))


def test_mmdit_forward_count_script_size_and_cache():
    """MMDiT(dim=512, depth=16, heads=16, ff_mult=2) (scripts/count_params_gflops.py) at N = 938 frames, nt = 200 tokens;
    cache=True reuses the text embedding per drop flag and must give the cache=False result."""
    arch = dict(dim=512, depth=16, heads=16, ff_mult=2, mel_dim=100, text_num_embeds=256)
    m = make_mmdit(73, **arch)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x, cond, text, _ = inputs(1, 938, 200, 100, 256, 74)
    m = m.cuda().eval()
    time = torch.tensor(0.55)
    ref = R.mmdit_forward(sd, 16, x, cond, text, time, False, False)
    xd, cd, td = x.cuda(), cond.cuda(), text.cuda()
    out = m(xd, cd, td, time.cuda(), False, False)
    assert rel_l2(out, ref) < 1e-2, rel_l2(out, ref)
    for drop in (False, True):
        plain = m(xd, cd, td, time.cuda(), False, drop)
        for _ in range(2):   # the first call fills the cache, the second reads it
            cached = m(xd, cd, td, time.cuda(), False, drop, cache=True)
            assert torch.equal(cached, plain), drop
    assert m.text_cond is not None and m.text_uncond is not None
    m.clear_cache()
    assert m.text_cond is None and m.text_uncond is None


def test_mmdit_forward_refuses_what_the_kernels_do_not_take():
    from f5e_tts_amd import _C
    m = make_mmdit(75, dim=64, depth=2, heads=2, ff_mult=1, mel_dim=20, text_num_embeds=30).cuda()
    x, cond, text, _ = inputs(1, 40, 9, 20, 30, 76)
    with pytest.raises(_C.F5EError, match="dim % 256"):
        m(x.cuda(), cond.cuda(), text.cuda(), torch.tensor(0.5).cuda(), False, False)
    m = make_mmdit(77, dim=256, depth=2, heads=4, ff_mult=1, mel_dim=20, text_num_embeds=30).cuda()
    x, cond, text, _ = inputs(2, 40, 9, 20, 30, 78)
    bad = torch.ones(2, 40, dtype=torch.bool)
    bad[1, 5] = False                                  # not of the lens_to_mask form
    with pytest.raises(_C.F5EError, match="lens_to_mask"):
        m(x.cuda(), cond.cuda(), text.cuda(), torch.tensor(0.5).cuda(), False, False, bad.cuda())
