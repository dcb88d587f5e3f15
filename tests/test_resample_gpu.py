"""Device sample-rate conversion (csrc/resample.hip through ops.resample / infer.audio.resample_device) against an fp64
convolution with the same fp32 filter bank, computed on the CPU here.

The gate is derived, not measured: any fp32 evaluation order of a T-term dot product (fused or not) satisfies
|err| <= gamma_T * sum_k |h_k x_k| with gamma_T = T u / (1 - T u), u = 2^-24, T = taps -- so every output is held to
|y - y64| <= gamma_T * (|bank| * |x|), the same convolution over absolute values."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RATIOS = [(24000, 16000), (16000, 24000), (44100, 24000), (44100, 16000), (48000, 16000), (22050, 24000), (8000, 24000)]
GUARD = -7.25


@pytest.fixture(scope="module")
def ops():
    import f5e_tts_amd.ops as ops_mod
    ops_mod.require_device()
    return ops_mod


def conv64(x, orig_freq, new_freq):
    """(y64, bound): the resampling sum in fp64 with the fp32 bank, and gamma_T * (|bank| * |x|) per output."""
    from f5e_tts_amd.infer import audio as A
    bank, width, orig, new = A.sinc_resample_kernel(orig_freq, new_freq)
    taps = bank.shape[-1]
    n = x.shape[-1]
    n_out = -(-new * n // orig)
    xp = F.pad(x.double(), (width, width + orig))[:, None]
    y = F.conv1d(xp, bank.double(), stride=orig).transpose(1, 2).reshape(x.shape[0], -1)[:, :n_out]
    mag = F.conv1d(xp.abs(), bank.double().abs(), stride=orig).transpose(1, 2).reshape(x.shape[0], -1)[:, :n_out]
    u = 2.0 ** -24
    return y, taps * u / (1 - taps * u) * mag


def sizes(orig_freq, new_freq):
    from f5e_tts_amd.infer import audio as A
    orig, _new, width, _taps = A.resample_plan(orig_freq, new_freq)
    return [1, max(1, orig - 1), orig, orig + 1, width, 2 * width + orig + 1, 4099]


@pytest.mark.parametrize("orig_freq,new_freq", RATIOS)
def test_parity_with_the_fp64_convolution_in_strided_views(ops, orig_freq, new_freq):
    from f5e_tts_amd.infer import audio as A
    orig, new, _w, _t = A.resample_plan(orig_freq, new_freq)
    g = torch.Generator().manual_seed(orig * 1000 + new)
    worst = 0.0
    for n in sizes(orig_freq, new_freq):
        n_out = -(-new * n // orig)
        for B in (1, 3):
            x = torch.randn(B, n, generator=g)
            want, bound = conv64(x, orig_freq, new_freq)
            xbuf = torch.full((B + 1, n + 5), GUARD, device="cuda")
            ybuf = torch.full((B + 1, n_out + 3), GUARD, device="cuda")
            xbuf[:B, :n] = x.cuda()
            xv, yv = xbuf[:B, :n], ybuf[:B, :n_out]                 # ld_x > n, ld_y > n_out
            assert ops.resample(xv, orig_freq, new_freq, out=yv) is yv
            alloc = ops.resample(xv, orig_freq, new_freq)
            torch.cuda.synchronize()
            assert alloc.shape == (B, n_out) == want.shape and torch.equal(alloc, yv)
            err = (yv.cpu().double() - want).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max())
            worst = max(worst, ratio)
            assert bool((err <= bound).all()), f"n={n} B={B}: error / bound = {ratio:.3f}"
            # nothing outside the rows' own n_out elements was written, and the input is only read
            assert bool((ybuf[:B, n_out:] == GUARD).all()) and bool((ybuf[B] == GUARD).all())
            assert torch.equal(xbuf[:B, :n].cpu(), x) and bool((xbuf[:B, n:] == GUARD).all())
    print(f"{orig_freq} -> {new_freq}: worst error / bound {worst:.3f}")


def test_resample_device_keeps_the_host_routes_shape_rules(ops):
    from f5e_tts_amd.infer import audio as A
    x = torch.randn(2, 3, 1001, generator=torch.Generator().manual_seed(3))
    host = A.resample(x, 44100, 16000)
    dev = A.resample_device(x.cuda(), 44100, 16000)
    assert dev.is_cuda and dev.shape == host.shape == (2, 3, math.ceil(160 * 1001 / 441))
    want, bound = conv64(x.reshape(6, -1), 44100, 16000)
    assert bool(((dev.cpu().double().reshape(6, -1) - want).abs() <= bound).all())
    one = A.resample_device(x[0, 0].cuda(), 24000, 16000)                  # [n] -> [n_out]
    assert one.shape == (math.ceil(2 * 1001 / 3),)
    xc = x.cuda()
    assert A.resample_device(xc, 16000, 16000) is xc and ops.resample(xc[0], 24000, 24000) is not None


def test_same_rate_bad_shapes_and_cpu_tensors(ops):
    from f5e_tts_amd import _C
    x = torch.randn(2, 300, device="cuda")
    assert ops.resample(x, 16000, 16000) is x
    with pytest.raises(_C.F5EError):
        ops.resample(x.cpu(), 24000, 16000)
    with pytest.raises(_C.F5EError):
        ops.resample(x, 24000, 16000, out=torch.empty(2, 200))                              # CPU output
    with pytest.raises(_C.F5EError):
        ops.resample(x, 24000, 16000, out=torch.empty(2, 201, device="cuda"))               # n_out is 200
    with pytest.raises(_C.F5EError):
        ops.resample(x, 24000, 16000, out=torch.empty(3, 200, device="cuda"))               # batch mismatch
    with pytest.raises(_C.F5EError):
        ops.resample(x[:, :0], 24000, 16000)                                                # n < 1
    with pytest.raises(_C.F5EError):
        ops.resample(x[:, ::2], 24000, 16000)                                               # sample stride 2
    with pytest.raises(_C.F5EError):
        ops.resample(x[:1].expand(2, 300), 24000, 16000)                                    # row stride 0 < n
    with pytest.raises(_C.F5EError):
        ops.resample(x.double(), 24000, 16000)
    torch.cuda.synchronize()


def test_captured_once_and_replayed_with_new_contents(ops):
    """One stream, a linear graph (f5e_graph_*): each replay reads the input buffer afresh and equals the eager launch bit
    for bit.  The bank is uploaded by the eager call before the capture."""
    B, n = 2, 3000
    g = torch.Generator().manual_seed(11)
    first, second = torch.randn(B, n, generator=g).cuda(), torch.randn(B, n, generator=g).cuda()
    eager = [ops.resample(v, 44100, 16000).clone() for v in (first, second)]
    x = torch.zeros(B, n, device="cuda")
    y = torch.zeros(B, eager[0].shape[1], device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gr = ops.Graph()
        gr.begin()
        try:
            ops.resample(x, 44100, 16000, out=y)
        finally:
            gr.end()
        for v, want in zip((first, second), eager):
            x.copy_(v)
            gr.launch()
            s.synchronize()
            assert torch.equal(y, want)
        gr.destroy()
