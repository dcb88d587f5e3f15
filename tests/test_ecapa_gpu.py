"""ECAPA-TDNN speaker encoder on the GPU (csrc/ecapa.hip through f5e_tts_amd.ops and eval/ecapa_tdnn.py) against
  * the REFERENCE's own ``ECAPA_TDNN.forward`` (tests/golden/ecapa.npz, made by tests/golden/make_ecapa_golden.py): every
    stored tensor, both pooling variants.  Gate: relative L2 < 2e-4, the project's gate for its fp32 ASR chains against
    reference fixtures (tests/test_ppg_gpu.py);
  * the CPU restatement (tests/ecapa_ref.py, pinned by the same fixture) in float64 on shapes the fixture does not hold.

Bound of the per-kernel comparisons (KERNEL_TOL = 2e-5 relative L2): the longest chain is the Res2 block, seven chained dot
products of K = 3 * 64 = 192 fp32 FMAs; with one rounding of 2^-24 relative per operation the error grows like
sqrt(7 * 192) * 2^-24 = 2.2e-6 as a root mean square -- which is what a relative L2 measures -- and 2e-5 is ten times that.
The row-equals-its-own-batch-of-one comparisons use the 1e-5 the issue sets.

Measured on an MI355X (relative L2, printed by every test before it asserts): fixture out1..out4 2.0-2.4e-7,
pooled 1.9-3.0e-7, embedding 0.8-1.0e-6 (T = 2: pooled up to 5.8e-6, embedding up to 3.1e-6, the reference's own distance from
float64 there); per kernel at most 1.5e-6; rows of a ragged batch equal their own B = 1 run bit for bit."""
import threading

import numpy as np
import pytest
import torch

import ecapa_ref as ER
from test_ecapa_cpu import CHANNELS, EMB, FEAT_DIM, GOLD, SEED, TS, L, cfg_of, ragged_batch

pytestmark = pytest.mark.gpu

GATE, KERNEL_TOL = 2e-4, 2e-5
I32 = torch.int32
KEYS = ("out1", "out2", "out3", "out4", "pooled", "emb")


@pytest.fixture(scope="module")
def ops():
    import f5e_tts_amd.ops as ops_mod
    ops_mod.require_device()
    return ops_mod


@pytest.fixture(scope="module")
def models(ops):
    from f5e_tts_amd.eval.ecapa_tdnn import ECAPA_TDNN
    out = {}
    for tag in ("p", "g"):
        m = ECAPA_TDNN(FEAT_DIM, channels=CHANNELS, emb_dim=EMB, global_context_att=tag == "g", feat_num=L)
        m.load_state_dict(ER.synth_state_dict(cfg_of(tag), SEED))
        out[tag] = m.cuda()
    return out


def i32(v):
    return torch.as_tensor(np.asarray(v), dtype=I32).cuda()


def hashed(stream, shape, lo=-1.0, hi=1.0):
    return ER.hash_tensor(SEED + 9, stream, shape, lo, hi)


def run(model, hs, lengths=None):
    taps = {}
    emb = model(hs.cuda(), None if lengths is None else i32(lengths), intermediates=taps)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in taps.items()}
    got["emb"] = emb.cpu()
    return got


def check(tag, got, want, tol):
    e = ER.rel_l2(got, want)
    print(f"{tag}: relative L2 {e:.2e} (bound {tol:.0e})")
    assert torch.isfinite(torch.as_tensor(got)).all() and e < tol, (tag, e)
    return e


# ------------------------------------------------------------------ against the reference fixture

@pytest.mark.parametrize("tag", ["p", "g"])
def test_every_fixture_case_end_to_end(models, tag):
    for T in TS:
        got = run(models[tag], torch.from_numpy(GOLD[f"hs_{T}"])[:, None])
        for k in KEYS:
            check(f"{tag} T={T} {k}", got[k][0], GOLD[f"{tag}_{k}_{T}"], GATE)


# ------------------------------------------------------------------ per kernel against the restatement

@pytest.mark.parametrize("Lm,Fd", [(1, 16), (4, 16), (25, 16), (1, 1024), (4, 1024), (25, 1024)])
def test_layer_mix_inorm(ops, Lm, Fd):
    for T in (1, 2, 63, 64, 65):
        lengths = [T, max(1, T - 3)]
        hs = hashed(T, (Lm, 2, T, Fd), -2.0, 2.0) + hashed(100 + T, (Lm, 1, 1, Fd), -0.5, 0.5)
        hs[:, 1, lengths[1]:] = 1e4
        fw = hashed(7, (Lm,))
        x = torch.full((2, T, Fd), float("nan"), device="cuda")
        mask = torch.full((2, T), float("nan"), device="cuda")
        ops.layer_mix_inorm(hs.cuda(), fw.cuda(), i32(lengths), x, mask)
        want = ER.layer_mix_inorm(hs.double(), fw.double(), torch.tensor(lengths))
        check(f"layer mix L={Lm} F={Fd} T={T}", x.cpu(), want, KERNEL_TOL)
        assert torch.equal(mask.cpu(), (torch.arange(T)[None] < torch.tensor(lengths)[:, None]).float())
        assert float(x[1, lengths[1]:].abs().sum()) == 0.0
        if T > 1:           # lengths = None: every row has T frames
            x2, m2 = torch.empty_like(x), torch.empty_like(mask)
            ops.layer_mix_inorm(hs[:, :1].contiguous().cuda(), fw.cuda(), None, x2[:1], m2[:1])
            assert torch.equal(x2[0], x[0]) and float(m2[0].min()) == 1.0


def res2_inputs(w, B, T, lengths):
    x = hashed(3 * w + T, (B, T, 8 * w))
    for b, n in enumerate(lengths):
        x[b, n:] = 1e4                              # the kernel reads no frame at or beyond a row's length
    wt = hashed(11, (7, w, w, 3), -1.0, 1.0) * (3.0 / (3 * w)) ** 0.5
    bias, scale, shift = hashed(12, (7, w), -0.1, 0.1), hashed(13, (7, w), 0.5, 1.5), hashed(14, (7, w), -0.3, 0.3)
    return x, wt, bias, scale, shift


def res2_run(ops, x, wt, bias, scale, shift, lengths, d, steps=((0, 7),)):
    w = wt.shape[1]
    packed = wt.permute(0, 1, 3, 2).reshape(7, w, 3 * w).contiguous().cuda()
    y = torch.full(x.shape, float("nan"), device="cuda")
    xd, ln = x.cuda(), i32(lengths)
    for first, count in steps:
        ops.res2_dconv(xd, y, packed, bias.cuda(), scale.cuda(), shift.cuda(), ln, d, first, count)
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("w", [8, 32, 64])      # the generic kernel, the 16-aligned one, and its w = 64 instance
@pytest.mark.parametrize("d", [2, 3, 4])
def test_res2_chain(ops, w, d):
    tile = ops.RES2_TILE
    for T in (1, d, 2 * d - 1, 2 * d, 2 * d + 1, 2 * tile + 3):      # the last crosses two tile boundaries with a live halo
        lengths = [T, max(1, T - 2)]
        x, wt, bias, scale, shift = res2_inputs(w, 2, T, lengths)
        y = res2_run(ops, x, wt, bias, scale, shift, lengths, d)
        mask = (torch.arange(T)[None] < torch.tensor(lengths)[:, None]).double()[..., None]
        want = ER.res2_chain(x.double() * mask, [(wt[i].double(), bias[i].double()) for i in range(7)],
                             [(scale[i].double(), shift[i].double()) for i in range(7)], d, mask)
        check(f"res2 w={w} d={d} T={T}", y, want, KERNEL_TOL)
        assert float(y[1, lengths[1]:].abs().sum()) == 0.0


def test_res2_one_launch_equals_seven(ops):
    """Seven launches of one step each (no halo recomputed) give the bits of the single launch."""
    lengths = [77, 50]
    args = res2_inputs(64, 2, 77, lengths)
    one = res2_run(ops, *args, lengths, 3)
    seven = res2_run(ops, *args, lengths, 3, steps=[(i, 1) for i in range(7)])
    assert torch.equal(one, seven)


@pytest.mark.parametrize("shortcut", [False, True])
def test_se_gate(ops, shortcut):
    B, T, C, Cin, lengths = 2, 37, 64, (48 if shortcut else 64), [37, 20]
    mask = (torch.arange(T)[None] < torch.tensor(lengths)[:, None]).float()[..., None]
    x, xin = hashed(21, (B, T, C)) * mask, hashed(22, (B, T, Cin)) * mask
    w1, b1, w2, b2 = hashed(23, (128, C), -0.2, 0.2), hashed(24, (128,)), hashed(25, (C, 128), -0.2, 0.2), hashed(26, (C,))
    sw, sb = hashed(27, (C, Cin), -0.2, 0.2), hashed(28, (C,))
    dev = lambda t: t.cuda().contiguous()  # noqa: E731
    mean, z1, z2 = (torch.empty(B, n, device="cuda") for n in (C, 128, C))
    ops.time_stats(dev(x), i32(lengths), mean)
    ops.gemm_f32(mean, dev(w1), dev(b1), out=z1, act=ops.ACT_RELU)
    ops.gemm_f32(z1, dev(w2), dev(b2), out=z2)
    resid = dev(xin)
    if shortcut:
        resid = ops.gemm_f32(dev(xin).view(B * T, Cin), dev(sw), dev(sb), out=torch.empty(B * T, C, device="cuda"),
                             row_scale=dev(mask).view(B * T)).view(B, T, C)
    out = torch.full((B, T, C), float("nan"), device="cuda")
    ops.se_scale(dev(x), z2, resid, out)
    r64 = (xin.double() @ sw.double().T + sb.double()) * mask.double() if shortcut else xin.double()
    want = ER.se_gate(x.double(), r64, w1.double(), b1.double(), w2.double(), b2.double(), torch.tensor(lengths))
    check(f"SE gate shortcut={shortcut}", out.cpu(), want, KERNEL_TOL)
    assert float(out[1, 20:].abs().sum()) == 0.0


@pytest.mark.parametrize("C", [68, 1536])
def test_pooling_kernels(ops, C):
    for T in (1, 2, 65, 300):
        lengths = [T, max(min(T, 2), T - 5)]
        mask = (torch.arange(T)[None] < torch.tensor(lengths)[:, None]).float()[..., None]
        x = (hashed(31 + T, (2, T, C), 0.0, 2.0) * mask).contiguous()     # post-ReLU features: non-negative
        logits = hashed(32 + T, (2, T, C), -3.0, 3.0)
        logits[1, lengths[1]:] = 1e4
        out = torch.full((2, 2 * C), float("nan"), device="cuda")
        ops.attn_stats_pool(x.cuda(), logits.cuda(), i32(lengths), out)
        check(f"attentive pooling C={C} T={T}", out.cpu(), ER.attn_stats_pool(x.double(), logits.double(), torch.tensor(lengths)),
              KERNEL_TOL)
        if T >= 2:                            # the global context of the second variant: mean and unbiased std over time
            ctx = torch.full((2, 2 * C), float("nan"), device="cuda")
            ops.time_stats(x.cuda(), i32(lengths), ctx[:, :C], ctx[:, C:])
            mean, std = ER.context_stats(x.double(), torch.tensor(lengths))
            check(f"global context C={C} T={T}", ctx.cpu(), torch.cat([mean, std], 1), KERNEL_TOL)


@pytest.mark.parametrize("shift", [-80.0, 80.0])
def test_pooling_online_softmax_survives_shifted_logits(ops, shift):
    """exp(80) overflows nothing here and exp(-80) loses no row: the softmax is taken about the running maximum.  One row of
    logits also RISES by 60 over time, so the running maximum moves and the sums are rescaled again and again."""
    T, C, lengths = 300, 68, [300, 211]
    x = hashed(41, (2, T, C), 0.0, 2.0)
    logits = hashed(42, (2, T, C), -3.0, 3.0) + shift
    logits[0] += torch.linspace(0, 60, T)[:, None]
    out = torch.empty(2, 2 * C, device="cuda")
    ops.attn_stats_pool(x.cuda(), logits.cuda(), i32(lengths), out)
    want = ER.attn_stats_pool(x.double(), logits.double(), torch.tensor(lengths))     # from the SAME fp32 logits
    check(f"pooling with logits {shift:+.0f}", out.cpu(), want, KERNEL_TOL)
    plain = torch.empty_like(out)
    ops.attn_stats_pool(x.cuda(), (logits - shift).cuda(), i32(lengths), plain)
    check(f"pooling, shift {shift:+.0f} taken out", plain.cpu(), want, 1e-4)    # a shift of 80 rounds the logits to 7.6e-6


# ------------------------------------------------------------------ ragged batches

@pytest.mark.parametrize("tag", ["p", "g"])
def test_ragged_rows_equal_their_batch_of_one(models, tag):
    lengths = [150, 37, 9]
    got = run(models[tag], ragged_batch(lengths, 1e4, seed=0), lengths)
    other = run(models[tag], ragged_batch(lengths, 3e4, seed=1), lengths)
    for k in KEYS:
        assert torch.equal(got[k], other[k]), f"{k} depends on what lies beyond the lengths"
    for b, n in enumerate(lengths):
        one = run(models[tag], torch.from_numpy(GOLD[f"hs_{n}"])[:, None])
        for k in KEYS:
            row = got[k][b, :n] if got[k].ndim == 3 else got[k][b]
            check(f"{tag} row {b} (len {n}) {k} vs its own B = 1 run", row, one[k][0], 1e-5)
            check(f"{tag} row {b} (len {n}) {k} vs the fixture", row, GOLD[f"{tag}_{k}_{n}"], GATE)
            if got[k].ndim == 3:
                assert float(got[k][b, n:].abs().sum()) == 0.0


@pytest.mark.parametrize("tag", ["p", "g"])
def test_similarity_matches_the_fixture_cosine(models, tag):
    a, b = ragged_batch([150, 37]).cuda(), ragged_batch([37, 150]).cuda()
    sim = models[tag].similarity(a, i32([150, 37]), b, i32([37, 150]))
    assert sim.is_cuda and sim.shape == (2,)
    print(f"{tag}: similarity {sim.tolist()} fixture {float(GOLD[f'{tag}_cos']):.6f}")
    assert float((sim.cpu() - float(GOLD[f"{tag}_cos"])).abs().max()) < 1e-4


# ------------------------------------------------------------------ full size and behaviour

def test_full_size_against_the_restatement(ops):
    from f5e_tts_amd.eval.ecapa_tdnn import ECAPA_TDNN_SMALL
    cfg = ER.make_cfg(1024, 512, 256, False, 25)
    sd = ER.synth_state_dict(cfg, SEED + 1)
    model = ECAPA_TDNN_SMALL(1024)
    model.load_state_dict(sd)
    model.cuda()
    lengths = [100, 73]
    hs = ER.synth_hidden_states(SEED + 2, 25, 2, 100, 1024)
    got = run(model, hs, lengths)
    want = ER.forward(sd, cfg, hs, torch.tensor(lengths), dtype=torch.float64)
    for k in KEYS:
        check(f"full size {k}", got[k], want[k], GATE)


def test_twice_the_same_bits_and_graph_replay(models):
    m = models["g"]
    lengths, B, T = [150, 37, 9], 3, 150
    hs = ragged_batch(lengths).cuda()
    ln = i32(lengths)
    first, second = m(hs, ln).clone(), m(hs, ln).clone()
    assert torch.equal(first, second)
    ws = torch.empty(m.workspace_bytes(B, T), dtype=torch.uint8, device="cuda")
    out = torch.zeros(B, EMB, device="cuda")
    static_hs = torch.zeros_like(hs)
    m(static_hs, ln, workspace=ws, out=out)                  # warm: the fold, the LDS opt-in, code objects
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m(static_hs, ln, workspace=ws, out=out)
    static_hs.copy_(hs)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)
    ln.copy_(i32([150, 150, 150]))                            # lengths are read on the device at replay time
    static_hs.copy_(ragged_batch([150, 150, 150]).cuda())
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, m(static_hs, None))


def test_argument_errors_return_codes_and_fault_nothing(ops, models):
    from f5e_tts_amd import _C
    lib = _C.lib()
    x = torch.zeros(1, 8, 64, device="cuda")
    y = torch.zeros(1, 8, 64, device="cuda")
    par = torch.zeros(7 * 8 * 24, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731
    box = []

    def body():
        # f5e_last_error is thread-local and nothing clears it: calls that are meant to fail run on a thread of their own
        err = lib.f5e_last_error
        ok = lib.f5e_res2_dconv(st, None, 64, p(y), 64, p(par), p(par), p(par), p(par), None, 1, 8, 64, 2, 0, 7) == -1 \
            and b"null" in err()
        ok &= lib.f5e_res2_dconv(st, p(x), 64, p(y), 64, p(par), p(par), p(par), p(par), None, 1, 8, 60, 2, 0, 7) == -1 \
            and b"multiple of 8" in err()
        ok &= lib.f5e_layer_mix_inorm(st, p(x), None, None, p(y), p(par), 4, 1, 8, 16) == -1 and b"null" in err()
        ok &= lib.f5e_attn_stats_pool(st, p(x), 64, None, 64, None, p(y), 1, 8, 64) == -1 and b"null" in err()
        box.append(bool(ok))

    t = threading.Thread(target=body)
    t.start(), t.join()
    assert box == [True]
    m = models["p"]
    hs = torch.zeros(L, 2, 9, FEAT_DIM, device="cuda")
    with pytest.raises(_C.F5EError, match="hidden_states must be"):                   # L mismatch
        m(torch.zeros(L + 1, 2, 9, FEAT_DIM, device="cuda"))
    with pytest.raises(_C.F5EError, match="i32"):                                     # lengths of the wrong dtype
        m(hs, torch.tensor([9, 4], device="cuda"))
    with pytest.raises(_C.F5EError, match="i32"):
        ops.time_stats(x, torch.tensor([8.0], device="cuda"), torch.zeros(1, 64, device="cuda"))
    with pytest.raises(_C.F5EError, match="multiple of 8"):
        ops.res2_dconv(torch.zeros(1, 8, 60, device="cuda"), torch.zeros(1, 8, 60, device="cuda"), par[:7 * 7 * 21].view(7, 7, 21),
                       par[:49].view(7, 7), par[:49].view(7, 7), par[:49].view(7, 7), None, 2)
    with pytest.raises(_C.F5EError, match="workspace"):
        m(hs, workspace=torch.empty(64, dtype=torch.uint8, device="cuda"))
    assert torch.isfinite(m(hs + 1.0, i32([9, 4]))).all()                             # and the device is still in good health
    torch.cuda.synchronize()
