"""tests/fp32_ops_ref.py held to independent torch calls, and the preconditions that tests/test_fp32_ops_gpu.py relies on:
the integer GEMM inputs really are exact in fp32 (so ``torch.equal`` is the right comparison), the inexact activations see
arguments within +-20, the restated host dispatch sends the case lists through every kernel / epilogue / ring state / tail
combination, and every condition of the vector epilogue is broken alone by some case."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

import fp32_ops_ref as R

F64 = torch.float64


def same(a, b, what, tol=1e-12):
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert a.shape == b.shape and err <= tol * max(1.0, float(b.abs().max())), f"{what}: max err {err:.3e}"


def unique(cases, key):
    seen = {}
    for c in cases:
        seen.setdefault(key(c), c)
    return list(seen.values())


# ------------------------------------------------------------------ the restatements against independent torch calls

def test_act_constants_match_the_library():
    from f5e_tts_amd import _C
    assert (R.ACT_NONE, R.ACT_SILU, R.ACT_GELU_ERF, R.ACT_GELU_TANH, R.ACT_RELU, R.ACT_MISH) == \
        (_C.ACT_NONE, _C.ACT_SILU, _C.ACT_GELU_ERF, _C.ACT_GELU_TANH, _C.ACT_RELU, _C.ACT_MISH)


def test_activation_restatements():
    v = torch.linspace(-25, 25, 2001, dtype=F64)
    for act, fn in ((R.ACT_SILU, F.silu), (R.ACT_GELU_ERF, F.gelu), (R.ACT_GELU_TANH, lambda t: F.gelu(t, approximate="tanh")),
                    (R.ACT_RELU, F.relu), (R.ACT_MISH, F.mish), (R.ACT_NONE, lambda t: t)):
        same(R.apply_act(v, act), fn(v), f"act {act}", 1e-9)
    # the exponent the kernel rounds: silu e^-x, tanh-gelu e^-2u, mish e^min(x, 20)
    u = math.sqrt(2 / math.pi) * (v + 0.044715 * v ** 3)
    same(v / (1 + torch.exp(R.act_exp_arg(v, R.ACT_GELU_TANH))), 0.5 * v * (1 + torch.tanh(u)), "tanh-gelu exponent", 1e-9)
    same(v / (1 + torch.exp(R.act_exp_arg(v, R.ACT_SILU))), F.silu(v), "silu exponent", 1e-9)
    assert float(R.act_exp_arg(v, R.ACT_MISH).max()) == 20.0 and float(R.act_exp_arg(v, R.ACT_GELU_ERF).abs().max()) == 0


def gemm_by_rows(c, t):
    """The header formula of csrc/gemm_f32.hip one output row at a time, on torch's own activations."""
    fn = {R.ACT_NONE: lambda v: v, R.ACT_RELU: F.relu, R.ACT_SILU: F.silu, R.ACT_GELU_ERF: F.gelu, R.ACT_MISH: F.mish,
          R.ACT_GELU_TANH: lambda v: F.gelu(v, approximate="tanh")}
    A, W = t["A"].double(), t["W"].double()
    out = torch.empty(c.M, c.N, dtype=F64)
    for m in range(c.M):
        v = F.linear(fn[c.a_act](A[m % A.shape[0]]), W, None if t["bias"] is None else t["bias"].double())
        v = fn[c.act](v)
        if t["cs"] is not None:
            v = v * t["cs"].double()
        if t["add"] is not None:
            v = v + t["add"].double()[m % t["add"].shape[0]]
        out[m] = v * (1.0 if t["rs"] is None else float(t["rs"][m]))
    return out


@pytest.mark.parametrize("c", R.WRAPS + R.INPLACE + R.ACT_CASES[:4] + R.ACT_CASES[-4:] + R.A_ACT_CASES[:2] +
                         (R.RING32[5], R.EDGES[0], R.FORMS["n67"][0]._replace(bias=False, rs=False)), ids=R.cid)
def test_gemm_reference(c):
    t = R.gemm_operands(c)
    same(R.gemm_ref(c, t), gemm_by_rows(c, t), R.cid(c), 1e-9)
    if c.a_rows:                                                # the wrap is visible: row 13 repeats row 0's product
        z = R.gemm_z(c.M, c.N, c.K, c.a_rows, c.randn, c.a_act)
        assert torch.equal(z[13], z[0]) and not torch.equal(z[1], z[0])
    if c.rs and c.M > 8:
        assert set(t["rs"].tolist()) == {0.0, 1.0, 2.0}


def test_gemm_operand_value_sets():
    t = R.gemm_operands(R.RING32[3])
    for k, lo, hi in (("A", -8, 8), ("W", -8, 8), ("bias", -16, 16), ("add", -64, 64)):
        assert float(t[k].min()) >= lo and float(t[k].max()) <= hi and torch.equal(t[k], t[k].round()) and t[k].dtype == torch.float32
    assert set(t["cs"].tolist()) == {0.25, 0.5, 1.0, 2.0, 4.0}
    assert R.SENTINEL == float(torch.tensor(R.SENTINEL).to(torch.bfloat16)) and abs(R.SENTINEL) > 64   # never an addend value


@pytest.mark.parametrize("B,T,C,kind", [R.grn_shrunk(c) for c in R.GRN_CASES])
def test_grn_reference(B, T, C, kind):
    x, gam, bet = R.grn_inputs(B, T, C, kind)
    xd = x.double()
    gx = torch.linalg.vector_norm(xd, ord=2, dim=1, keepdim=True)
    ref = gam.double() * (xd * (gx / (gx.mean(dim=-1, keepdim=True) + 1e-6))) + bet.double() + xd
    y, g1 = R.grn(x, gam, bet, want_gx=True)
    same(y, ref, "grn")
    same(g1, gx[:, 0], "gx")
    if kind == "zero":                                          # gx = 0: gamma * (0 * 0 / 1e-6) + beta + 0
        assert torch.equal(y[1], bet.double().expand(T, C)) and float(x[0].abs().min()) > 0


def test_grn_cases_reach_their_paths():
    paths = {c: R.grn_path(*c) for c in R.GRN_CASES}
    assert paths[(1, 1100, 1024, "")] == (True, 2) and paths[(1, 4100, 66, "")] == (False, 2)
    assert paths[(2, 33, 68, "x1")] == (False, 1) and paths[(2, 33, 68, "g1")] == (False, 1)
    assert all(paths[(2, T, 68, "")] == (True, 1) for T in R.GRN_T) and paths[(2, 17, 4, "")][0]
    assert 68 % 64 and 4 % 64                                   # a partial last block of 64 channels on the vector path
    # grn_norm4_kernel: 16 row groups, unrolled by 8: 0 / 1 / 2 rows per group, and one / two trips of the unrolled loop
    assert {(T + 15) // 16 for T in R.GRN_T} >= {1, 2, 7, 8, 9, 16}


@pytest.mark.parametrize("B,T,C", [c if c[1] < 100 else (2, 21, 1024) for c in R.DWCONV7_CASES])
def test_dwconv7_reference(B, T, C):
    x, w_t, bias = R.dwconv7_inputs(B, T, C)
    ref = F.conv1d(x.double().transpose(1, 2), w_t.double().t().unsqueeze(1), bias.double(), padding=3, groups=C).transpose(1, 2)
    assert torch.equal(R.dwconv7(x, w_t, bias), ref)
    assert torch.equal(R.dwconv7(x, w_t, bias, dtype=torch.float32).double(), ref)          # exact in fp32 too
    assert float(x.abs().min()) >= 1 and torch.equal(x, x.round())
    if B > 1:                                                   # a tap that reached across the batch boundary would show
        alone = R.dwconv7(x[1:2], w_t, bias)
        assert torch.equal(alone, ref[1:2]) and not torch.equal(x[0], x[1])


def test_dwconv7_big_case_passes_the_grid_cap():
    B, T, C = R.DWCONV7_CASES[-1]
    assert B * T * C // 4 > R.CONV_GRID_CAP and B * T * C * 4 < 18e6


@pytest.mark.parametrize("ksize", R.IM2COL_K)
def test_im2col_reference(ksize):
    for T, Cin in itertools.product(R.IM2COL_T, R.IM2COL_CIN):
        x = R.im2col_inputs(R.IM2COL_B, T, Cin)
        for pad in R.im2col_pads(ksize, T):
            xp = F.pad(x, (0, 0, pad, max(ksize - 1 - pad, 0) + pad))          # zeros before and (more than enough) after
            ref = torch.stack([xp[:, j:j + T] for j in range(ksize)], 2).reshape(R.IM2COL_B, T, ksize * Cin)
            assert torch.equal(R.im2col(x, ksize, pad), ref), (ksize, T, Cin, pad)
    B, T, Cin, k, pad = R.IM2COL_BIG
    assert B * T * Cin * k > R.CONV_GRID_CAP


# ------------------------------------------------------------------ exactness of the integer GEMM cases

@pytest.mark.parametrize("c", unique(R.EXACT_CASES, lambda c: (c.M, c.N, c.K, c.a_rows)), ids=R.cid)
def test_integer_gemm_is_exact_in_fp32(c):
    """The fp32 CPU matmul (whatever order it sums in) equals the int64 reference, and the largest value any epilogue step can
    reach, in units of ch_scale's 1/4, stays below 2^24."""
    t = R.gemm_inputs(c.M, c.N, c.K, c.a_rows, 0, False)
    idx = torch.arange(c.M) % (c.a_rows or c.M)
    z64 = t["A"].long()[idx] @ t["W"].long().T
    assert torch.equal(t["A"][idx] @ t["W"].T, z64.float())
    assert torch.equal(R.gemm_z(c.M, c.N, c.K, c.a_rows, False, R.ACT_NONE), z64.double())
    assert c.K <= 2048 and 64 * c.K >= int(z64.abs().max()) and R.exact_magnitude_bound(c.K) < 2 ** 24


@pytest.mark.parametrize("c", unique(R.EXACT_CASES, lambda c: c._replace(outs="f32")), ids=R.cid)
def test_integer_epilogue_is_exact_in_fp32(c):
    """Every epilogue step in fp32 gives the fp64 value, for NONE and RELU: no tolerance is needed on the GPU."""
    t = R.gemm_operands(c)
    for act in R.EXACT_ACTS:
        ca = c._replace(act=act)
        ref = R.gemm_ref(ca, t)
        assert torch.equal(R.gemm_ref(ca, t, dtype=torch.float32).double(), ref) and torch.equal(ref.float().double(), ref)
    assert float(ref.abs().max()) * 4 < 2 ** 24


@pytest.mark.parametrize("c", R.ACT_CASES, ids=R.cid)
def test_activation_arguments_stay_within_20(c):
    arg = R.gemm_pre(c, R.gemm_operands(c))
    assert 10.0 < float(arg.abs().max()) <= 20.0
    assert torch.equal(arg.float().double(), arg)               # the scaled argument is still exact in fp32
    assert float(arg.min()) < -5 and float(arg.max()) > 5


# ------------------------------------------------------------------ the dispatch: which case runs what

def test_dispatch_restatement():
    off = dict(A=0, W=0, bias=0, ch_scale=0, addend=0, out=0, out_bf16=0)
    lds = dict(ldo=1024, ldo_bf16=0, ld_add=0)
    assert R.gemm_f32_path(449, 1024, 68, 0, off, lds) == ("dma64", True, 2, True)           # 8 x 16 = 128 tiles
    assert R.gemm_f32_path(448, 1152, 132, 0, off, {**lds, "ldo": 1152}) == ("dma32", True, 3, True)   # 7 x 18 = 126
    assert R.gemm_f32_path(449, 1024, 64, R.ACT_SILU, off, lds) == ("plain", False, 4, False)
    assert R.gemm_f32_path(33, 68, 64, 0, {**off, "W": 4}, lds) == ("plain", False, 4, False)
    assert R.gemm_f32_path(33, 68, 64, 0, {**off, "out_bf16": 8}, lds)[1] is True            # bf16 needs 8 bytes only
    assert R.gemm_f32_path(33, 68, 64, 0, {**off, "out": 8}, lds)[1] is False
    assert R.gemm_f32_path(33, 3, 64, 0, off, {**lds, "ldo": 4})[1] is False                 # N < 4


def test_case_lists_are_the_listed_ones():
    assert [(c.M, c.N) for c in R.RING32] == [(33, 68)] * len(R.RING32_K)
    assert set(R.RING32_K) >= {4, 60, 64, 68, 128, 192, 196, 256, 260, 324, 516}
    assert [R.case_path(c)[2] for c in R.RING32[:11]] == [1, 1, 1, 2, 2, 3, 4, 4, 5, 6, 9]
    assert set(R.RING64_K) >= {4, 64, 68, 128, 132, 192, 196, 260, 388}
    assert [R.case_path(c)[2] for c in R.RING64[:9]] == [1, 1, 2, 2, 3, 3, 4, 5, 7]
    for c in R.RING64[:-1]:
        assert R.case_path(c)[0] == "dma64" and R.case_path(c)[1] == (c.N % 4 == 0)
    assert R.case_path(R.RING64[-1])[0] == "dma32" and (R.RING64[-1].M, R.RING64[-1].N, R.RING64[-1].K) == (448, 1152, 132)
    assert all(R.case_path(c)[:2] == ("dma32", True) for c in R.RING32)
    assert all(R.case_path(c)[:2] == ("dma32", False) for c in R.RING32_SCALAR)
    assert len(R.MISALIGNED) == 2 * len(R.MISALIGNED_K) and all(R.case_path(c)[0] == "plain" for c in R.MISALIGNED)
    for c in R.MISALIGNED:                                      # only the base is off: lda, ldw stay multiples of 4
        assert (c.K + R.A_PAD) % 4 == 0 and (c.K + R.W_PAD) % 4 == 0 and c.a_off + c.w_off == 1
    assert sorted(c.M for c in R.EDGES if c.N == 68 and c.M != 33) == [1, 31, 32, 63, 64, 65]
    assert sorted({c.N for c in R.EDGES if c.M == 33}) == [1, 3, 4, 5, 60, 63, 64, 65, 68] and {c.K for c in R.EDGES} == {68}
    assert {(c.add_rows, R.case_path(c)[1]) for c in R.WRAPS} == {(a, v) for a in (1, 3, 33) for v in (True, False)}
    assert all(c.a_rows == 13 and c.M % 13 for c in R.WRAPS)
    assert {(c.M, c.N, R.case_path(c)[1]) for c in R.INPLACE} == {(33, 68, True), (33, 67, False), (65, 68, True), (65, 67, False)}
    assert [R.case_path(c)[0] for c in R.ACT_SHAPES] == ["dma32", "dma64", "plain"]
    assert all(R.case_path(c)[0] == "plain" for c in R.A_ACT_CASES)
    assert all(c.K % 4 == 0 and c.K <= 2048 for c in R.ALL_GEMM_CASES)


def test_every_dispatch_cell_is_hit():
    """kernel x epilogue x ring state x tail.  gemm_f32_kernel has the scalar epilogue only, and its two LDS buffers make
    ``KT < NSTAGE - 1`` (no K step at all) impossible; every other cell must hold a case."""
    hit = {}
    for c in R.ALL_GEMM_CASES:
        kern, vec, KT, ragged = R.case_path(c)
        hit.setdefault((kern, vec, R.ring_state(kern, KT), ragged), c)
    rings = ("<NSTAGE-1", "=NSTAGE-1", "=NSTAGE", ">NSTAGE")
    want = {(k, v, r, t) for k in ("dma32", "dma64") for v in (True, False) for r in rings for t in (False, True)} | \
        {("plain", False, r, t) for r in rings[1:] for t in (False, True)}
    assert want - set(hit) == set(), sorted(want - set(hit))
    assert set(hit) - want == set(), sorted(set(hit) - want)
    exact = {R.case_path(c)[:2] + (R.ring_state(R.case_path(c)[0], R.case_path(c)[2]), R.case_path(c)[3]) for c in R.EXACT_CASES}
    assert exact >= {w for w in want if w[0] != "plain"}        # the DMA kernels' cells all hold a bit-exact case


def test_every_vector_condition_is_broken_alone():
    alone = {}
    for name, (c, cond) in R.FORMS.items():
        off, lds = R.case_layout(c)
        broken = R.vec_broken(c.N, off, lds)
        assert broken == ({cond} if cond else set()), (name, broken)
        assert R.case_path(c)[:2] == ("dma32", cond is None)
        alone[cond] = name
    assert set(alone) == set(R.VEC_CONDITIONS) | {None}
    c = R.FORMS["sliced_aligned"][0]                            # the cd[:, off:off + n] form: a slice inside a wider buffer
    assert c.out_off > 0 and c.out_pad > c.out_off and len(R.form_variants(c)) == 48


@pytest.mark.parametrize("c", [f[0] for f in R.FORMS.values()] + [R.MISALIGNED[0], R.MISALIGNED[-1], R.INPLACE[0]], ids=R.cid)
def test_placed_views_sit_where_the_case_claims(c):
    """``placed`` on the CPU: the view's distance from its buffer's start is the claimed offset, and the buffer has two
    rows of slack behind the view."""
    off, _ = R.case_layout(c)
    t = R.gemm_operands(c)
    for key, o, ld, tens in (("A", c.a_off, c.K + R.A_PAD, t["A"]), ("W", c.w_off, c.K + R.W_PAD, t["W"]),
                             ("out", c.out_off, c.N + c.out_pad, torch.zeros(c.M, c.N))):
        flat, spec = R.placed(tens, o, ld)
        v = R.view(flat, spec)
        assert (v.data_ptr() - flat.data_ptr()) % 16 == off[key] and torch.equal(v, tens) and v.stride() == (ld, 1)
        assert flat.numel() == (tens.shape[0] + 2) * ld
        mask = torch.ones_like(flat, dtype=torch.bool)
        mask.as_strided(*spec).fill_(False)
        assert bool((flat[mask] == R.SENTINEL).all())
