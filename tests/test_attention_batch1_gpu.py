"""f5e_flash_attn's batch-1 kernel (4 KV splits, every wave owns at most two 64-key steps: N <= 512) against an fp32 softmax
on the CPU from the same bf16 inputs, at the key counts where its entry loads, its step gating and its four-wave tail can go
wrong.  Both of a wave's tiles are requested before kv_len is known, with clamped indices: a tile that was loaded but lies
past kv_len must never be used, so the K / V rows past kv_len hold large finite values here."""
import functools
import math

import pytest
import torch

from test_ops_gpu import QSCALE, close, pack_qkv

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
S, H = 2, 2
RTOL, ATOL = 2 ** -6, 6e-3      # test_ops_gpu.test_flash_attn: P rounded to bf16 before P.V, the output to bf16
PAST = 30000.0                  # K / V rows past kv_len (finite in bf16; one such key or value used would swamp a row)

# N: what it exercises
SHAPES = [33,    # one key tile: waves 1-3 own nothing, their clamped loads must be harmless
          256,   # exactly one full tile per wave
          257,   # wave 0 owns two tiles, the second with 1 key
          448,   # wave 3 owns one tile
          449,   # the last tile holds 1 key
          469,   # the workload's shape
          512,   # two full tiles each, no mask
          513]   # nine tiles: the general loop


@pytest.fixture(scope="module")
def ops():
    import f5e_tts_amd.ops as ops_mod
    ops_mod.require_device()
    return ops_mod


def g(seed):
    return torch.Generator().manual_seed(seed)


def reference(q, k, v, lens):
    """fp32 softmax attention, [S * N, H * 64]; q pre-scaled by log2(e) / 8, keys >= lens[s] masked."""
    N = q.shape[2]
    s = (q.float() @ k.float().transpose(-1, -2)) * math.log(2.0)           # 2^(q' k) = e^(q k / 8)
    if lens is not None:
        km = torch.arange(N)[None, :] < lens[:, None]
        s = s.masked_fill(~km[:, None, None, :], float("-inf"))
    return (torch.softmax(s, -1) @ v.float()).transpose(1, 2).reshape(S * N, H * 64)


@functools.lru_cache(maxsize=None)
def case(N, ragged):
    """Seeded inputs and their reference, computed once per (N, ragged) and shared by the tests below."""
    q = (torch.randn(S, H, N, 64, generator=g(30)) * QSCALE).to(BF)
    k = torch.randn(S, H, N, 64, generator=g(31)).to(BF)
    v = torch.randn(S, H, N, 64, generator=g(32)).to(BF)
    lens = None
    if ragged:
        lens = torch.tensor([N, max(1, N - 70)], dtype=torch.int32)   # sequence 1: a whole tile past its key count
        k[1, :, int(lens[1]):] = PAST
        v[1, :, int(lens[1]):] = -PAST
    return q, k, v, lens, reference(q, k, v, lens)


def run(ops, q, k, v, lens, waves, out=None):
    N = q.shape[2]
    n_pad = (N + 63) // 64 * 64
    qd, kd, vtd = pack_qkv(ops, q, k, v, n_pad)
    if out is None:
        out = torch.empty(S * N, H * 64, device="cuda", dtype=BF)
    ops.flash_attn(qd, kd, vtd, out, N, kv_len=lens.cuda() if lens is not None else None, waves=waves)
    return out


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("N", SHAPES)
def test_batch1_attention_matches_fp32_softmax(ops, N, ragged):
    q, k, v, lens, ref = case(N, ragged)
    auto, four, one = (run(ops, q, k, v, lens, w).cpu() for w in (0, 4, 1))
    for out, what in ((auto, "auto"), (four, "4 KV splits"), (one, "no split")):
        assert torch.isfinite(out.float()).all(), f"N {N} {what}: non-finite output"
        close(out, ref, RTOL, ATOL, f"N {N} ragged {ragged}, {what}")
    close(four, one.float(), RTOL, ATOL, f"N {N} ragged {ragged}: 4 KV splits against none")


@pytest.mark.parametrize("factor", [4.0, 12.0])
def test_batch1_attention_overflowing_fast_pass_is_rerun(ops, factor):
    """Keys whose score towers over a wave's first step (test_ops_gpu.test_flash_attn_spike_forces_rescale): in wave 0's
    first step (key 40), in its FULL second step, which runs unchecked (key 300: factor 4 stays finite at p ~ 2^46, factor
    12 overflows exp2 to inf and the wave repeats both steps in the checked form), and in wave 3's masked second step (key
    460, checked on the way)."""
    N = 469
    q0 = torch.randn(S, H, N, 64, generator=g(33))
    k = torch.randn(S, H, N, 64, generator=g(34)).to(BF)
    v = torch.randn(S, H, N, 64, generator=g(35)).to(BF)
    q = (q0 * QSCALE).to(BF)
    for s, h in ((0, 0), (1, 1)):
        for key, qi in ((300, 17), (40, 99), (460, 250)):
            k[s, h, key] = (q0[s, h, qi] * factor).to(BF)   # score ~ factor |q|^2 / 8 >> the others
    lens = torch.tensor([N, 465], dtype=torch.int32)
    ref = reference(q, k, v, lens)
    four, one = (run(ops, q, k, v, lens, w).cpu() for w in (4, 1))
    assert torch.isfinite(four.float()).all()
    close(four, ref, RTOL, ATOL, f"spike x{factor}, 4 KV splits")
    close(four, one.float(), RTOL, ATOL, f"spike x{factor}: 4 KV splits against none")


def test_batch1_attention_graph_replay_equals_eager(ops):
    q, k, v, lens, _ = case(469, True)
    n_pad = 512
    qd, kd, vtd = pack_qkv(ops, q, k, v, n_pad)
    ld = lens.cuda()
    eager = torch.empty(S * 469, H * 64, device="cuda", dtype=BF)
    ops.flash_attn(qd, kd, vtd, eager, 469, kv_len=ld, waves=4)
    replay = torch.zeros_like(eager)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        gr = ops.Graph()
        gr.begin()
        try:
            ops.flash_attn(qd, kd, vtd, replay, 469, kv_len=ld, waves=4)
        finally:
            gr.end()
        for _ in range(2):
            replay.zero_()
            gr.launch()
            st.synchronize()
            assert torch.equal(replay, eager)
        gr.destroy()
