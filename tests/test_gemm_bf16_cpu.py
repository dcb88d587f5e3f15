"""CPU side of the bf16 GEMM parity tests: pins tests/gemm_bf16_ref.py (the integer reference against torch.matmul in fp64 and
the fp32 bound, the fragment-major index maps against the arithmetic in csrc/gemm_bf16_epilogue.h, the restated dispatch against
hand-read cases) and asserts that the case lists reach every cell of ``dispatch<EPI>()`` / ``launch_pp()``; the refusals of
f5e_tts_amd.ops that fire before any device is needed."""
import pytest
import torch

import gemm_bf16_ref as R

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def shapes(cases):
    return sorted({(c.M, c.N, c.K) for c in cases})


# ------------------------------------------------------------------ the integer reference

@pytest.mark.parametrize("M,N,K", shapes(R.ALL_CASES), ids=lambda v: str(v))
def test_integer_reference_is_exact_in_fp32(M, N, K):
    """max |acc| < 2^24 (with bias, gate and residual on top: |x| <= 64 + 2 (9 K + 8)), operands exact in bf16, and the
    reference equal to torch.matmul in fp64; where int64 is affordable, to the int64 product as well."""
    a, w, bias = R.int_operands(M, N, K)
    assert int(a.abs().max()) <= 3 and int(w.abs().max()) <= 3 and int(bias.abs().max()) <= 8
    assert torch.equal(a.to(BF).to(torch.int64), a) and torch.equal(w.to(BF).to(torch.int64), w)
    z = R.acc_i64(M, N, K)
    assert int(z.abs().max()) <= 9 * K <= 18432 and 64 + 2 * (9 * K + 8) < 2 ** 24
    assert torch.equal(z.double(), torch.matmul(a.double(), w.double().T))
    assert torch.equal(z.float().double(), z.double())                     # every entry is an fp32 number
    if M * N * K <= 1 << 27:
        assert torch.equal(z, a @ w.T)


@pytest.mark.parametrize("M,N,K", shapes(R.BIAS_CASES + R.QKV_CASES)[::7], ids=lambda v: str(v))
def test_planted_ties_tell_rounding_from_truncation(M, N, K):
    z = R.acc_i64(M, N, K)
    assert z[0, 0] == 259 and z[0, 1] == -259
    rne = z[0, :2].float().to(BF).float()
    trunc = (z[0, :2].float().view(torch.int32) & ~0xFFFF).view(F32)
    assert rne.tolist() == [260.0, -260.0] and trunc.tolist() == [258.0, -258.0]


def test_gelu_arguments_stay_within_6():
    for c in R.ALL_CASES:
        if c.epi == "gelu" and not c.fuse:
            s = R.gelu_scale(c)
            assert float(R.pre_activation(c).abs().max()) * s <= 6.0 and s == 2.0 ** round(torch.log2(torch.tensor(s)).item())


def test_exact_epilogues_are_exact_in_fp32():
    """gate + residual and the producer's xs argument are integers below 2^24; the tile means are multiples of 1/64."""
    for c in R.PRODUCER_CASES[:6] + R.GATE_CASES[:6]:
        x = R.gate_expect(c)
        assert torch.equal(x, x.round()) and float(x.abs().max()) < 2 ** 24
        if c.fuse == 2:
            _, xs, mean, _ = R.producer_expect(c)
            assert torch.equal(xs, xs.round()) and float(xs.abs().max()) < 2 ** 24
            assert torch.equal(mean * 64, (mean * 64).round()) and torch.equal(mean.float().double(), mean)
            _, _, mean32, _ = R.producer_expect(c, F32)
            assert torch.equal(mean32.double(), mean)


# ------------------------------------------------------------------ fragment-major layouts

@pytest.mark.parametrize("n_pad", [64, 128, 320])
def test_fragment_index_maps(n_pad):
    """ops.qk_frag_index / v_frag_index, the restated maps and the index arithmetic of the two epilogues (the inline one of
    gemm_bf16.hip and the generic one of gemm_bf16_epilogue.h) agree, and each map is a bijection onto [0, n_pad * 64)."""
    from f5e_tts_amd import ops
    qi, vi = R.frag_tables(n_pad)
    assert torch.equal(qi, ops.qk_frag_index(n_pad)) and torch.equal(vi, ops.v_frag_index(n_pad))
    for t in (qi, vi):
        assert torch.equal(t.reshape(-1).sort().values, torch.arange(n_pad * 64))
    for pos in range(n_pad):
        for d in range(0, 64, 4):
            # gemm_bf16.hip, inline epilogue
            q_inline = (pos >> 5) * 2048 + (pos & 31) * 16 + (d >> 4) * 512 + ((d >> 3) & 1) * 8 + (d & 7)
            k16 = pos & 15
            v_inline = (pos >> 4) * 1024 + (d >> 5) * 512 + (d & 31) * 16 + ((k16 >> 2) & 1) * 8 + (((k16 >> 3) << 2) | (k16 & 3))
            assert int(qi[pos, d]) == q_inline and int(vi[pos, d]) == v_inline
            # the quad's four columns: 8 bytes of q / k, elements 16 apart of v^T
            assert [int(qi[pos, d + r]) for r in range(4)] == [q_inline + r for r in range(4)]
            assert [int(vi[pos, d + r]) for r in range(4)] == [v_inline + 16 * r for r in range(4)]


def test_qkv_scatter_and_gather_are_inverse():
    c = R.QKV_CASES[3]
    vals = torch.arange(c.M * c.N).reshape(c.M, c.N).remainder(251).float()
    n_pad = 64
    bufs = R.qkv_scatter(c, vals, n_pad)
    assert torch.equal(R.qkv_gather(c, bufs, n_pad), vals)
    assert sum(int((b.float() == R.SENTINEL).sum()) for b in bufs) >= 3 * (c.N // 192) * (n_pad - c.rps) * 64


# ------------------------------------------------------------------ the dispatch restatement

def test_dispatch_restatement_against_hand_read_cases():
    """Shapes whose instantiation the comments of dispatch<EPI>() name."""
    P = R.path
    assert P("gate", 938, 1024, 1024, fuse=2).inst == R.PROD_RS6                     # 15 x 16 tiles on 256 CUs
    assert P("qkv", 938, 3072, 1024, fuse=1).inst == R.CONS_QKV
    assert P("gelu", 938, 2048, 1024, fuse=1).inst == R.CONS_WIDE
    assert P("qkv", 1280, 3072, 1024, fuse=1).inst == R.CONS_QKV_BIG
    assert P("gelu", 2048, 2048, 1024, fuse=1).inst == R.CONS_WIDE_BIG
    assert P("gate", 2048, 1024, 2048, fuse=2).inst == R.PROD_BIG6
    assert P("gate", 2600, 1024, 2048, fuse=2).inst == R.PROD_C3
    assert P("gate", 938, 1024, 2048, fuse=2, gate_rows=2).inst == R.PROD_C4
    assert P("gate", 938, 1024, 2048).inst == R.GATE_RS and P("gate", 938, 1024, 2048, gate_rows=2).inst == R.T64_4
    assert P("bf16", 938, 2048, 1024).inst == R.T64_3 and P("bf16", 938, 1024, 2048).inst == R.T64_4
    assert P("bf16", 11264, 1024, 1024).inst == R.PP and P("bf16", 11000, 1024, 64).inst == R.T128
    assert P("qkv", 100, 192, 64, qk_norm=True).inst == R.T128
    # pick_group_shift, from its comment: at M = 938 out-proj / FF2 (15 x 16 tiles) G = 4, FF1 (15 x 32) G = 8
    assert R.pick_group_shift(15, 16, 64, 64) == 2 and R.pick_group_shift(15, 32, 64, 64) == 3
    p = P("bf16", 4352, 4096, 128, hint=9)
    assert (p.n_tiles, p.grid, p.extra, p.walk, p.pp_ngroup) == (272, 256, 16, "grouped", 4)


def test_case_lists_hold_the_listed_sizes():
    Ms, Ns, Ks = {c.M for c in R.ALL_CASES}, {c.N for c in R.ALL_CASES}, {c.K for c in R.ALL_CASES}
    assert {1, 15, 16, 17, 63, 64, 65, 127, 129, 130, 257, 1088, 2112, 4352} <= Ms
    assert {4, 60, 64, 68, 100, 128, 192, 196, 260, 1024, 1300, 1536, 4096} <= Ns
    assert {64, 128, 192, 256, 320, 384, 448, 2048} <= Ks
    assert len(set(R.ALL_CASES)) == len(R.ALL_CASES)
    for c in R.ALL_CASES:
        assert c.K % 64 == 0 and c.N % 4 == 0 and 64 <= c.K <= 2048
        if c.epi in ("gate", "qkv"):
            assert c.rps >= 1 and (not c.masked or c.epi == "gate")
        if c.gate_rows > 1 and c.M > 1:
            assert R.cdiv(c.M, c.rps) >= c.gate_rows, R.cid(c)          # the second gate row is really used


def reached():
    cells = {}
    for c in R.ALL_CASES:
        p, states, flags, walk = R.case_cells(c)
        e = cells.setdefault(p.inst, dict(epis=set(), states=set(), flags=set(), walk=set()))
        e["epis"].add(c.epi)
        e["states"] |= states
        e["flags"] |= flags
        e["walk"] |= walk
    return cells


def test_every_instantiation_and_epilogue_pair_is_reached():
    """Every instantiation dispatch<EPI>() and launch_pp() can select, under every epilogue it is compiled for."""
    cells = reached()
    got = {(i, e) for i, v in cells.items() for e in v["epis"]}
    assert got == set(R.PAIRS), f"missing {[(R.NAME_OF[i], e) for i, e in set(R.PAIRS) - got]}, " \
                                f"unlisted {[(R.NAME_OF.get(i, i), e) for i, e in got - set(R.PAIRS)]}"


def test_every_ring_state_edge_flag_and_tile_walk_is_reached():
    """Per instantiation: every ring state and edge flag that R.possible_* calls reachable (the others are named there with
    the reason), the m-major walk and the grouped walk with at least two distinct shifts, and a grid that is no multiple of 8;
    for the ping-pong kernel all three walks, a narrower last column group, more tiles than workgroups and ``extra > 0``."""
    cells = reached()
    missing = []
    for name, inst in R.NAMES.items():
        v = cells[inst]
        want_s, never_s = R.possible_ring_states(inst)
        want_f, never_f = R.possible_edge_flags(inst, v["epis"])
        assert all(never_s.values()) and all(never_f.values())
        assert not (v["states"] & set(never_s)) and not (v["flags"] & set(never_f)), (name, v, never_s, never_f)
        missing += [(name, s) for s in sorted(want_s - v["states"])] + [(name, f) for f in sorted(want_f - v["flags"])]
        if inst.kernel == "pp":
            want_w = {"m_major", "grouped", "n_major", "n_main % 8 != 0", "pp_ngroup 4 with a narrower last group",
                      "more tiles than workgroups", "extra > 0"}
            missing += [(name, w) for w in sorted(want_w - v["walk"])]
        else:
            shifts = {w for w in v["walk"] if w.startswith("grouped")}
            if "m_major" not in v["walk"]:
                missing.append((name, "m_major"))
            if len(shifts) < 2:
                missing.append((name, f"two grouped shifts (have {sorted(shifts)})"))
            if "n_main % 8 != 0" not in v["walk"]:
                missing.append((name, "n_main % 8 != 0"))
    assert not missing, missing


# Cells that no problem the public entry points accept can reach; the reasons are in R.possible_ring_states / possible_edge_flags
UNREACHABLE = {
    ("PROD_RS6", "partial N tile"), ("PROD_RS4", "partial N tile"), ("PROD_BIG6", "M == 1"), ("PROD_BIG6", "partial N tile"),
    ("PROD_BIG4", "M == 1"), ("PROD_BIG4", "partial N tile"), ("PROD_C4", "KT < NPRO"), ("PROD_C4", "KT == NPRO"),
    ("PROD_C4", "partial N tile"), ("PROD_C3", "partial N tile"), ("CONS_QKV", "KT < NPRO"), ("CONS_QKV", "KT == NPRO"),
    ("CONS_QKV", "partial N tile"), ("CONS_QKV_BIG", "KT < NPRO"), ("CONS_QKV_BIG", "KT == NPRO"), ("CONS_QKV_BIG", "M == 1"),
    ("CONS_QKV_BIG", "partial N tile"), ("CONS_WIDE", "KT < NPRO"), ("CONS_WIDE", "KT/2 odd"), ("CONS_WIDE", "partial N tile"),
    ("CONS_WIDE_BIG", "KT < NPRO"), ("CONS_WIDE_BIG", "KT == NPRO"), ("CONS_WIDE_BIG", "M == 1"),
    ("CONS_WIDE_BIG", "partial N tile"), ("CONS_C3", "KT < NPRO"), ("CONS_C3", "KT == NPRO"), ("T128", "KT < NPRO"),
    ("T64_4", "KT < NPRO"), ("T64_4", "KT == NPRO"),
}


def test_unreachable_cells_are_the_named_ones():
    """The restatement's own list of unreachable cells is this one, each with a reason; the fused consumer's follow from
    K / 64 = parts in {4, 8, 12, 16}, which ops.gemm_bf16_bias / gemm_bf16_qkv_rope enforce (stats [M, K / 64, 2])."""
    named = set()
    for name, inst in R.NAMES.items():
        epis = {e for i, e in R.PAIRS if i == inst}
        for never in (R.possible_ring_states(inst)[1], R.possible_edge_flags(inst, epis)[1]):
            assert all(isinstance(r, str) and r for r in never.values())
            named |= {(name, k) for k in never}
    assert named == UNREACHABLE, named ^ UNREACHABLE


def test_group_shifts_under_test():
    """pick_group_shift returns every shift from 0 to 4 somewhere in the case lists (not only 0 and the maximum)."""
    shifts = {R.case_path(c).shift for c in R.ALL_CASES if R.case_path(c).walk == "grouped" and R.case_path(c).inst.kernel == "ring"}
    assert shifts >= {0, 1, 2, 3, 4}, shifts


# ------------------------------------------------------------------ refusals that need no device

def _t(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype)


LN_REFUSALS = {
    "consumer: parts 5": lambda ops: ops.ln_consumer(_t(8, 5, 2), _t(1, 64), _t(1, 64), 4, _t(8)),
    "consumer: parts 20": lambda ops: ops.ln_consumer(_t(8, 20, 2), _t(1, 64), _t(1, 64), 4, _t(8)),
    "consumer: stats not [rows, parts, 2]": lambda ops: ops.ln_consumer(_t(8, 4, 3), _t(1, 64), _t(1, 64), 4, _t(8)),
    "consumer: stats 2-D": lambda ops: ops.ln_consumer(_t(8, 8), _t(1, 64), _t(1, 64), 4, _t(8)),
    "consumer: stats not f32": lambda ops: ops.ln_consumer(_t(8, 4, 2, dtype=BF), _t(1, 64), _t(1, 64), 4, _t(8)),
    "consumer: row_mean not f32": lambda ops: ops.ln_consumer(_t(8, 4, 2), _t(1, 64), _t(1, 64), 4, _t(8, dtype=BF)),
    "consumer: c and d differ": lambda ops: ops.ln_consumer(_t(8, 4, 2), _t(1, 64), _t(1, 128), 4, _t(8)),
    "consumer: eval_ptr without cd_eval_stride": lambda ops: ops.ln_consumer(_t(8, 4, 2), _t(1, 64), _t(1, 64), 4, _t(8),
                                                                            eval_ptr=_t(1, dtype=torch.int32)),
    "producer: stats_out not [rows, N / 64, 2]": lambda ops: ops.ln_producer(_t(8, 64, dtype=BF), _t(1, 64), _t(8, 2), _t(8)),
    "producer: stats_out not f32": lambda ops: ops.ln_producer(_t(8, 64, dtype=BF), _t(1, 64), _t(8, 1, 2, dtype=BF), _t(8)),
    "producer: row_mean 2-D": lambda ops: ops.ln_producer(_t(8, 64, dtype=BF), _t(1, 64), _t(8, 1, 2), _t(8, 1)),
}


@pytest.mark.parametrize("name", list(LN_REFUSALS))
def test_ln_fuse_refusals(name):
    """Shape and type checks of ln_consumer / ln_producer fire before any pointer is taken, so they need no device; the message
    is about the shape, not about where the tensor lives."""
    from f5e_tts_amd import _C, ops
    with pytest.raises(_C.F5EError) as e:
        LN_REFUSALS[name](ops)
    assert "GPU" not in str(e.value), str(e.value)
