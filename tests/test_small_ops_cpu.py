"""tests/small_ops_ref.py held to independent torch calls in fp64, at every shape tests/test_small_ops_gpu.py uses (shrunk
where the size only exists to pass a grid cap), and the shared INPUTS checked for the properties the GPU cases rely on.
The last section swaps in deliberately wrong references: each must be told apart on these inputs, otherwise the GPU case
built on them could not tell a kernel with that bug from a correct one."""
import math

import pytest
import torch
import torch.nn.functional as F

import small_ops_ref as R

F64 = torch.float64


def same(a, b, what, tol=1e-12):
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert a.shape == b.shape and err <= tol * max(1.0, float(b.abs().max())), f"{what}: max err {err:.3e}"


def mod_rows_loop(y, sc, sh, rows_per_seq):
    out = y.clone()
    for r in range(y.shape[0]):
        m = (r // rows_per_seq) % sc.shape[0]
        out[r] = y[r] * (1 + sc[m].double()) + sh[m].double()
    return out


# ------------------------------------------------------------------ references against independent torch calls

@pytest.mark.parametrize("D", R.LN_SMALL_D + R.LN_FIXED_D)
def test_layernorm_reference_fixed_widths(D):
    x, gam, bet, tab = R.ln_inputs(7, D)
    e, stride = 1, tab.stride(0)
    sc0, sh0 = tab[0, :, D:2 * D], tab[0, :, 0:D]
    ln = F.layer_norm(x.double(), (D,), eps=1e-6)
    same(R.layernorm(x, None, scale=sc0, shift=sh0, rows_per_seq=3, eval_ptr=e, eval_stride=stride),
         mod_rows_loop(ln, tab[e, :, D:2 * D], tab[e, :, 0:D], 3), "modulate, eval 1, row 6 wraps to modulation row 0")
    same(R.layernorm(x, None, gamma=gam, beta=bet, eps=1e-5), F.layer_norm(x.double(), (D,), gam.double(), bet.double(), 1e-5),
         "affine eps 1e-5")
    both = mod_rows_loop(F.layer_norm(x.double(), (D,), gam.double(), bet.double(), 1e-6), sc0, sh0, 3)
    same(R.layernorm(x, None, gamma=gam, beta=bet, scale=sc0, shift=sh0, rows_per_seq=3), both, "gamma/beta and scale/shift")


@pytest.mark.parametrize("D", R.LN_ANY_D)
def test_layernorm_reference_any_width(D):
    x, gam, bet, _ = R.ln_inputs(5, D)
    same(R.layernorm(x, None, eps=1e-5), F.layer_norm(x.double(), (D,), eps=1e-5), "plain")
    same(R.layernorm(x, None, gamma=gam, beta=bet, eps=1e-5), F.layer_norm(x.double(), (D,), gam.double(), bet.double(), 1e-5),
         "affine")


@pytest.mark.parametrize("D", R.ADALN_D)
def test_adaln_pre_reference(D):
    x, _, _, tab = R.ln_inputs(7, D)
    parts = D // 64
    for e in (None, 1):
        xs, st, rm = R.adaln_pre(x, None, tab[0, :, D:2 * D], parts, None, 3, e, tab.stride(0))
        xd = x.double()
        sc = tab[e or 0, :, D:2 * D].double()[(torch.arange(7) // 3) % 2]
        same(rm, xd.mean(1), "row mean")
        same(xs, (xd - xd.mean(1, keepdim=True)) * (1 + sc), "xs")         # as test_fused_adaln_chain computes them
        assert st.shape == (7, parts, 2) and float(st[:, :, 0].abs().max()) == 0
        same(st[:, :, 1].sum(1), ((xd - xd.mean(1, keepdim=True)) ** 2).sum(1), "M2")


@pytest.mark.parametrize("D", R.L2_D)
def test_l2norm_reference(D):
    x, gw = R.l2_inputs(7, D)
    ref = R.l2norm(x, None, gw)
    same(ref, F.normalize(x.double(), dim=-1) * math.sqrt(D) * gw.double(), "l2norm")
    assert float(x[3].abs().max()) == 0 and float(ref[3].abs().max()) == 0 and torch.isfinite(ref).all()


@pytest.mark.parametrize("case", R.GLU_CASES)
def test_glu_reference_and_saturating_gates(case):
    rows, C = R.shrunk(case)
    x, kind = R.glu_inputs(rows, C)
    ref = R.glu(x)
    same(ref, F.glu(x.double(), dim=-1), "glu")
    gate = x[:, C:]
    assert bool((gate[kind == 0].abs() <= 20.0).all())
    for i, val in enumerate(R.GLU_SPECIAL):
        assert (kind == i + 1).any() and bool((gate[kind == i + 1] == val).all()), val
    # what "saturated" means in fp32: 1 + exp(-30) rounds to 1, exp(100) overflows to inf
    assert torch.equal(R.glu(x, dtype=torch.float32)[(kind == 1) | (kind == 3)], x[:, :C][(kind == 1) | (kind == 3)])
    assert float(R.glu(x, dtype=torch.float32)[kind == 4].abs().max()) == 0 and torch.isfinite(ref).all()


@pytest.mark.parametrize("case", R.DWCONV_CASES)
def test_dwconv_reference_and_keep_masks(case):
    B, T, C, K = R.shrunk(case)
    x, w_t, bias, keep = R.dwconv_inputs(B, T, C, K)
    conv = lambda v: F.conv1d(v.double().transpose(1, 2), w_t.double().t().unsqueeze(1), bias.double(), padding=(K - 1) // 2,  # noqa: E731
                              groups=C).transpose(1, 2)
    same(R.dwconv(x, w_t, bias), conv(x), "no keep")
    same(R.dwconv(x, w_t, bias, None, keep), conv(x * keep[..., None]), "keep")
    # the inputs: masked frames hold data, both mask values occur, and every window of three or more frames (clipped to the
    # sequence) has a live and a dead frame, so an ignored, shifted or batch-swapped mask changes every such output frame
    assert float(x.abs().min()) > 0 and keep.min() == 0 and keep.max() == 1
    pad = (K - 1) // 2
    for b in range(B):
        for t in range(T):
            win = keep[b, max(0, t - pad):min(T, t + pad + 1)]
            if win.numel() >= 3:
                assert win.min() == 0 and win.max() == 1, (b, t)
    if T > 1:
        assert not torch.equal(keep[0], keep[1])


@pytest.mark.parametrize("L", R.SOFTMAX_L)
def test_softmax_rows_reference_and_lengths(L):
    buf, kv, scale = R.softmax_inputs(L)
    ld = buf.shape[1]
    assert ld == (L + 3) // 4 * 4 + 4 and bool((buf[:, L:] == R.SENTINEL).all())
    assert kv.tolist() == [0, 3, L, L + 9] and float((buf[:, :L] * scale).abs().max()) <= 10.0   # |exp argument| <= 20
    ref = R.softmax_rows(buf[:, :L], ld, L, scale, kv, R.SOFTMAX_RPS)
    ln = torch.clamp(kv.long()[torch.arange(R.SOFTMAX_ROWS) // R.SOFTMAX_RPS], max=L)
    assert ln.tolist() == [0, 0, min(3, L), min(3, L), L, L, L]
    dead = torch.arange(L)[None, :] >= ln[:, None]
    sm = torch.softmax((buf[:, :L].double() * scale).masked_fill(dead, -math.inf), -1).masked_fill(dead, 0.0)
    same(ref[:, :L], torch.nan_to_num(sm, nan=0.0), "masked softmax")
    assert ref.shape == (R.SOFTMAX_ROWS, ld) and float(ref[:, L:].abs().max()) == 0 and float(ref[:2].abs().max()) == 0
    same(ref[6], R.softmax_rows(buf[:, :L], ld, L, scale)[6], "kv_len > L is the unmasked row", 0.0)


def test_softmax_rows_large_magnitude_inputs():
    buf, kv, scale = R.softmax_inputs(200, big=True)
    s = buf[:, :200] * scale
    assert float(s.abs().max()) <= 1e4 and float(s.abs().max()) > 5e3
    ref = R.softmax_rows(buf[:, :200], buf.shape[1], 200, scale, kv, R.SOFTMAX_RPS)
    assert torch.isfinite(ref).all() and torch.allclose(ref[2:].sum(1), torch.ones(5, dtype=F64))


@pytest.mark.parametrize("V,G,vd,combine", R.VQ_CASES + ((2048, 1, 8, False),))
def test_vq_eval_reference_and_tie_rows(V, G, vd, combine):
    logits, vars_, ties = R.vq_inputs(V, G, vd, combine)
    tgt, q, code, prob = R.vq_eval(logits, vars_, combine, groups=G, num_vars=V)
    assert logits.shape[1] > G * V and float(logits[:, G * V:].min()) > R.VQ_TOP       # row stride > G V, poisoned pad
    lg = logits[:, :G * V].reshape(-1, G, V).double()
    assert torch.equal(tgt.long(), torch.max(lg, -1).indices)                          # torch.max: first maximal index
    hot = F.one_hot(tgt.long(), V).double()                                            # [rows, G, V]
    cb = vars_.double().reshape(1 if combine else G, V, vd)
    same(q, torch.einsum("rgv,gvd->rgd", hot, cb.expand(G, V, vd)).reshape(-1, G * vd), "one-hot gather", 0.0)
    ent = lambda p: torch.exp(-(p * torch.log(p + 1e-7)).sum(-1)).sum()                # noqa: E731
    same(code, ent(hot.mean(0)), "code perplexity")
    same(prob, ent(torch.softmax(lg, -1).mean(0)), "prob perplexity")
    # the tie rows hold what they say: exactly these maxima, nothing else as large, and the first one is expected
    want_sets = {(5, 6), tuple(range(V))} | ({(3, 67, 131), (70, 134), (70, 133)} if V > 134 else set())
    assert {idx for idx, _ in ties.values()} == want_sets
    for (r, gi), (idx, want) in ties.items():
        row = lg[r, gi]
        assert torch.nonzero(row == row.max()).flatten().tolist() == list(idx) and want == idx[0] and int(tgt[r, gi]) == want
    if V > 134:   # lane = index % 64 of the kernel's layout: same-lane ties, and a cross-lane tie whose winner sits in the higher lane
        assert 3 % 64 == 67 % 64 == 131 % 64 and 70 % 64 == 134 % 64 and 133 % 64 < 70 % 64


@pytest.mark.parametrize("with_pos,with_keep", [(True, True), (False, True), (True, False)])
def test_text_gather_reference_and_clamps(with_pos, with_keep):
    B, N, TD, max_pos, rows = R.shrunk(R.TEXT_GATHER_CASE)
    assert R.TEXT_GATHER_CASE[1] > max_pos < N and R.TEXT_GATHER_CASE[0] * R.TEXT_GATHER_CASE[1] * TD // 4 > R.GRID_CAP_ELEMENTWISE
    ids, table, pos, keep = R.text_gather_inputs(B, N, TD, max_pos, rows)
    assert int(ids.min()) < 0 and int(ids.max()) >= rows and {-1, rows} <= set(ids.flatten().tolist())
    ref = R.text_gather(ids, table, pos if with_pos else None, keep if with_keep else None)
    for b in range(B):
        for n in range(N):
            v = table[min(max(int(ids[b, n]), 0), rows - 1)].double()
            if with_pos:
                v = v + pos[min(n, max_pos - 1)].double()
            if with_keep:
                v = v * float(keep[b, n])
            assert torch.equal(ref[b, n], v), (b, n)
    assert torch.equal(ref.float().double(), ref) or with_pos    # a pure gather is exact in fp32; the one add is compared in fp32 below
    f32 = R.text_gather(ids, table, pos if with_pos else None, keep if with_keep else None, dtype=torch.float32)
    same(f32.double(), ref, "fp32 restatement", 2 ** -23)


@pytest.mark.parametrize("C,L", R.POST_CASES)
def test_conv_post_reference_and_range(C, L):
    a, w, bias = R.post_inputs(C, L)
    conv = lambda bb: F.conv1d(a.double().transpose(1, 2), w.double().t().unsqueeze(0), bb, padding=R.POST_K // 2)[:, 0]   # noqa: E731
    same(R.conv_post(a, w, bias, pre=True), conv(bias.double()), "pre-activation")
    same(R.conv_post(a, w, bias), conv(bias.double()).clamp(-1, 1), "clamp")
    same(R.conv_post(a, w, bias, use_tanh=True), torch.tanh(conv(bias.double())), "tanh")
    same(R.conv_post(a, w, None), conv(None).clamp(-1, 1), "no bias")
    if L >= 255:
        pre = R.conv_post(a, w, bias, pre=True)
        assert float(pre.max()) > 2 and float(pre.min()) < -2 and int((pre.abs() < 0.5).sum()) > 10


def test_elementwise_references():
    n = R.shrunk(R.BIG_N)
    assert R.BIG_N > R.GRID_CAP_ELEMENTWISE and R.STITCH_CASE[0] * R.STITCH_CASE[1] > R.GRID_CAP_ELEMENTWISE
    x, y = torch.randn(n, generator=R.g(1)), torch.randn(n, generator=R.g(2))
    same(R.axpby(x, y, None, 0.7, -1.3, 0.25), torch.add(torch.add(0.7 * x.double(), y.double(), alpha=-1.3), 0.25), "axpby")
    same(R.axpby(x, None, None, 0.7, 0.0, 0.25), torch.addcmul(torch.full((n,), 0.25, dtype=F64), x.double(), torch.tensor(0.7, dtype=F64)), "axpby y=None")
    pred, coef = torch.randn(3, n, generator=R.g(3)), torch.tensor([0.1, 0.25, 0.5])
    p = pred.double()
    for mode, v in ((0, p[0]), (1, p[0] + (p[0] - p[1]) * 2.0), (2, 2.0 * (p[2] - p[1]) + 3.0 * (p[1] - p[0]) + p[0])):
        same(R.ode_update(pred, n, mode, 2.0, 3.0, y, None, coef, 1), y.double() + coef.double()[1] * v, f"ode mode {mode}")
    rows, C = R.shrunk(R.STITCH_CASE)
    mask = (torch.rand(rows, generator=R.g(4)) > 0.5).to(torch.uint8)
    c, yy = torch.randn(rows, C, generator=R.g(5)), torch.randn(rows, C, generator=R.g(6))
    st = R.stitch(c, yy, mask)
    assert all(torch.equal(st[r], c[r] if mask[r] else yy[r]) for r in range(rows))


def test_cast_inputs_hold_the_edge_values():
    x = R.cast_inputs(4096)
    bits = x.view(torch.int32)
    low, bf = bits & 0xFFFF, x.to(torch.bfloat16)
    fin = torch.isfinite(x)
    assert int(((low == 0x8000) & fin).sum()) >= 8                                     # exact ties
    even = bf.view(torch.int16)[(low == 0x8000) & fin & (x.abs() > 1e-30)] & 1
    assert bool((even == 0).all())                                                     # ... which torch rounds to even
    assert torch.isinf(x).sum() == 4 and torch.isnan(x).sum() == 6 and torch.isnan(bf).sum() == 6
    assert torch.isinf(bf).sum() == 8                                                  # +-FLT_MAX round to +-inf
    assert int((bits == 0).sum()) >= 2 and int((bits == -(1 << 31)).sum()) >= 2        # +-0
    assert int(((x != 0) & (x.abs() < 2.0 ** -126)).sum()) >= 12                       # denormals
    assert torch.equal(x[:23].view(torch.int32), x[-23:].flip(0).view(torch.int32))


def test_fbank_inputs_and_the_oracle_noise_floor():
    """The gate of the GPU case (rtol 2e-4, atol 2e-3) is only fair where the fp32 oracle itself is well inside it: the
    oracle against its own fp64 evaluation on these inputs, silence excluded (exactly log(eps) on both sides)."""
    from oracle import f5e_ppg_oracle as P
    assert [1 + (nw - 400) // 160 for nw, _ in R.FBANK_CASES[::2]] == [1, 1, 2] and (559 - 400) % 160 == 159
    for nw, n_mels in R.FBANK_CASES:
        wav = R.fbank_inputs(nw)
        assert float(wav[1].abs().max()) == 0 and set(((wav[2] - 0.25)).tolist()) == {1.0, -1.0}
        sil = P.kaldi_fbank(wav[1], n_mels)
        assert bool((sil == math.log(torch.finfo(torch.float32).eps)).all()) or \
            bool((sil == torch.tensor(torch.finfo(torch.float32).eps).log()).all())
        for i in (0, 2):
            f32 = P.kaldi_fbank(wav[i], n_mels)
            x = wav[i].double() * 32768.0
            fr = x.unfold(0, 400, 160)
            fr = fr - fr.mean(1, keepdim=True)
            prev = torch.cat([fr[:, :1], fr[:, :-1]], 1)
            fr = F.pad((fr - 0.97 * prev) * P.povey_window(400).double(), (0, 112))
            spec = torch.fft.rfft(fr).abs() ** 2
            f64 = torch.clamp(spec @ P.kaldi_mel_banks(n_mels).double().T, min=torch.finfo(torch.float32).eps).log()
            err = (f32.double() - f64).abs()
            assert f32.shape == (1 + (nw - 400) // 160, n_mels) and bool((err <= 0.25 * (2e-3 + 2e-4 * f64.abs())).all()), \
                (nw, n_mels, i, float(err.max()))


# ------------------------------------------------------------------ deliberately wrong references must be told apart

def test_mutation_truncated_width_is_caught():
    """A kernel whose ``c < nv`` guards cut the row short normalises D' < D values: the last float4 dropped (an off-by-one
    guard), and the whole partial 64-lane group dropped where there is a full one before it."""
    for D in (252, 260, 516, 2044):
        x, _, _, _ = R.ln_inputs(5, D)
        good = F.layer_norm(x.double(), (D,), eps=1e-5)
        for cut in {D - 4, D // 4 // 64 * 64 * 4} - {0}:
            err = (R.layernorm(x[:, :cut], None, eps=1e-5) - good[:, :cut]).abs()
            assert float(err.max()) > 1e-3, (D, cut)            # two decades above the 1e-5 + 1e-5 |ref| gate


def test_mutation_ignored_keep_is_caught():
    for case in R.DWCONV_CASES:
        B, T, C, K = R.shrunk(case)
        x, w_t, bias, keep = R.dwconv_inputs(B, T, C, K)
        good, wrong = R.dwconv(x, w_t, bias, None, keep), R.dwconv(x, w_t, bias, None, None)
        assert float((wrong - good).norm() / good.norm()) > 1e-2, case      # gate: rel-L2 1e-6


def test_mutation_last_maximal_index_is_caught():
    for V, G, vd, combine in R.VQ_CASES:
        logits, vars_, ties = R.vq_inputs(V, G, vd, combine)
        tgt = R.vq_eval(logits, vars_, combine, groups=G, num_vars=V)[0]
        lg = logits[:, :G * V].reshape(-1, G, V)
        last = V - 1 - torch.max(lg.flip(-1), -1).indices
        assert not torch.equal(last, tgt.long()) and all(int(last[r, gi]) == idx[-1] for (r, gi), (idx, _) in ties.items())


def test_mutation_skipped_max_pos_clamp_is_caught():
    B, N, TD, max_pos, rows = R.shrunk(R.TEXT_GATHER_CASE)
    ids, table, pos, keep = R.text_gather_inputs(B, N, TD, max_pos, rows)
    longer = torch.cat([pos, torch.randn(N - max_pos, TD, generator=R.g(9))])            # what an unclamped read would see
    assert not torch.equal(R.text_gather(ids, table, longer, keep), R.text_gather(ids, table, pos, keep))
    assert torch.equal(R.text_gather(ids, table, longer, keep)[:, :max_pos], R.text_gather(ids, table, pos, keep)[:, :max_pos])
