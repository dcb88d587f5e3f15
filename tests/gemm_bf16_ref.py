"""The bf16 GEMM family (csrc/gemm_bf16.hip, csrc/gemm_bf16_pp.hip, csrc/gemm_bf16_epilogue.h) restated for its tests: the
host dispatch in plain Python (which instantiation a problem reaches, in which ring state, over which tile walk), seeded
integer operands on which every summation order gives the same fp32 result, the expectations of the epilogues, and the case
lists.  tests/test_gemm_bf16_cpu.py pins the restatements and asserts that the case lists reach every cell of the dispatch;
tests/test_gemm_bf16_gpu.py compares the HIP kernels with them.  Nothing here imports f5e_tts_amd.

Exact inputs: A, W integers in [-3, 3] (exact in bf16), bias in [-8, 8], gate in [-2, 2], resid integers in [-64, 64], all
seeded.  |acc| <= 9 K <= 18432 < 2^24, so the int64 ``a @ w.T`` is the fp32 result in ANY order; its ``.to(bfloat16)`` (round
to nearest even) is the bf16 one.  Row 0 of A and rows 0, 1 of W are planted so that C[0][0] = 259 and C[0][1] = -259 (bias 0
there): bf16 ties that round AWAY from the truncated value (260 against 258)."""
import functools
import math
from collections import namedtuple

import torch

import fp32_ops_ref as F

F64, F32, BF, I64, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int64, torch.int32
SENTINEL = F.SENTINEL
g = F.g
EPIS = ("bf16", "gelu", "gate", "qkv", "f32")          # EPI_BF16, EPI_BF16_GELU, EPI_GATE_RES, EPI_QKV_ROPE, EPI_F32
QSCALE = float(torch.tensor(1.4426950408889634, dtype=F32) * 0.125)   # 0.125f * 1.4426950408889634f (f5e_gemm_bf16_qkv_rope_pf)


def cdiv(a, b):
    return -(-a // b)


# ================================================================== the host dispatch, restated

# one kernel instantiation: gemm_bf16_kernel<BM, BN, EPI, NSTAGE, DBG, WGM, WGN, FUSE, NLOAD, DSTEP, DBUF> or the ping-pong kernel
Inst = namedtuple("Inst", "kernel BM BN NSTAGE WGM WGN FUSE NLOAD DSTEP DBUF")


def ring(BM, BN, NSTAGE, WGM=2, WGN=2, FUSE=0, NLOAD=0, DSTEP=1, DBUF=1):
    return Inst("ring", BM, BN, NSTAGE, WGM, WGN, FUSE, NLOAD, DSTEP, DBUF)


PP = Inst("pp", 256, 256, 2, 2, 4, 0, 0, 1, 1)
# dispatch<EPI>() of gemm_bf16.hip, in source order
PROD_RS6, PROD_RS4 = ring(64, 64, 6, 2, 2, 2, 4, 2), ring(64, 64, 4, 2, 2, 2, 4, 1)
PROD_BIG6, PROD_BIG4 = ring(128, 64, 6, 4, 2, 2, 4, 2), ring(128, 64, 4, 4, 2, 2, 4, 1)
PROD_C4, PROD_C3 = ring(64, 64, 4, 2, 2, 2), ring(64, 64, 3, 2, 2, 2)
CONS_QKV, CONS_QKV_BIG = ring(64, 192, 4, 2, 6, 1, 4, 1), ring(128, 192, 3, 2, 6, 1, 4, 1, 0)
CONS_WIDE, CONS_WIDE_BIG = ring(64, 128, 6, 2, 4, 1, 4, 2), ring(128, 128, 4, 2, 4, 1, 4, 1, 0)
CONS_C3 = ring(64, 64, 3, 2, 2, 1)
T128, T128X64 = ring(128, 128, 2, 4, 2), ring(128, 64, 3)
GATE_RS = ring(64, 64, 4, 2, 2, 0, 4)
T64_4, T64_3 = ring(64, 64, 4), ring(64, 64, 3)
NAMES = dict(PROD_RS6=PROD_RS6, PROD_RS4=PROD_RS4, PROD_BIG6=PROD_BIG6, PROD_BIG4=PROD_BIG4, PROD_C4=PROD_C4, PROD_C3=PROD_C3,
             CONS_QKV=CONS_QKV, CONS_QKV_BIG=CONS_QKV_BIG, CONS_WIDE=CONS_WIDE, CONS_WIDE_BIG=CONS_WIDE_BIG, CONS_C3=CONS_C3,
             T128=T128, T128X64=T128X64, GATE_RS=GATE_RS, T64_4=T64_4, T64_3=T64_3, PP=PP)
NAME_OF = {v: k for k, v in NAMES.items()}
_BIAS_EPIS = ("bf16", "gelu", "f32")
# every (instantiation, epilogue) pair that dispatch<EPI>() and launch_pp() can select
PAIRS = tuple((i, "gate") for i in (PROD_RS6, PROD_RS4, PROD_BIG6, PROD_BIG4, PROD_C4, PROD_C3, GATE_RS)) + \
    tuple((i, "qkv") for i in (CONS_QKV, CONS_QKV_BIG, CONS_C3)) + \
    tuple((i, e) for i in (CONS_WIDE, CONS_WIDE_BIG, CONS_C3) for e in _BIAS_EPIS) + \
    tuple((i, e) for i in (T128, T128X64, T64_4, T64_3, PP) for e in EPIS)


@functools.lru_cache(maxsize=None)
def pick_group_shift(tiles_m, tiles_n, bm, bn):
    """pick_group_shift of gemm_bf16.hip: the G = 2^s dividing tiles_n that minimises the distinct operand panels over the
    eight XCDs' contiguous runs of logical tile ids; the first minimum wins."""
    n = tiles_m * tiles_n
    q8, r8 = n >> 3, n & 7
    best, best_s = -1, 0
    s = 0
    while s <= 4 and tiles_n % (1 << s) == 0 and (1 << s) <= tiles_n:
        cost, tid = 0, 0
        for x in range(8):
            cnt = q8 + (1 if x < r8 else 0)
            seen_m, seen_n = set(), set()
            for _ in range(cnt):
                per = tiles_m << s
                grp, r = divmod(tid, per)
                seen_m.add(r >> s)
                seen_n.add((grp << s) + (r & ((1 << s) - 1)))
                tid += 1
            cost += len(seen_m) * bm + len(seen_n) * bn
        if best < 0 or cost < best:
            best, best_s = cost, s
        s += 1
    return best_s


Path = namedtuple("Path", "inst epi KT tiles_m tiles_n walk shift n_main_mod8 pp_ngroup n_tiles grid extra")


def uses_pp(M, K):
    return K >= 128 and cdiv(M, 256) >= 44


def select(epi, M, N, K, hint=0, gate_rows=1, fuse=0, qk_norm=False, cus=256):
    """dispatch<EPI>(): the instantiation.  fuse: 0, 1 (AdaLN consumer: ln_stats) or 2 (producer: stats_out)."""
    blocks = lambda bm, bn: cdiv(M, bm) * cdiv(N, bn)    # noqa: E731
    assert hint in (0, 1, 2, 3, 9) and epi in EPIS
    if fuse:
        assert not (epi == "qkv" and qk_norm)
        if epi == "gate":
            assert fuse == 2
            if gate_rows == 1 and blocks(64, 64) <= cus:
                return PROD_RS6 if K % 128 == 0 else PROD_RS4
            if gate_rows == 1 and blocks(128, 64) <= cus:
                return PROD_BIG6 if K % 128 == 0 else PROD_BIG4
            return PROD_C4 if K >= 2048 and blocks(64, 64) <= cus else PROD_C3
        assert fuse == 1
        if epi == "qkv":
            if N % 192 == 0 and blocks(64, 192) <= cus:
                return CONS_QKV
            if N % 192 == 0 and blocks(128, 192) <= cus:
                return CONS_QKV_BIG
        else:
            if N % 128 == 0 and blocks(64, 128) <= cus and K % 128 == 0:
                return CONS_WIDE
            if N % 128 == 0 and blocks(128, 128) <= cus:
                return CONS_WIDE_BIG
        return CONS_C3
    sel = hint
    if sel == 9 or (sel == 0 and uses_pp(M, K)):
        assert K >= 128
        return PP
    if epi == "qkv" and qk_norm:
        sel = 1
    if sel == 0:
        sel = 1 if blocks(128, 128) >= 320 else 2 if blocks(128, 64) >= 512 else 3
    if sel == 1:
        return T128
    if sel == 2:
        return T128X64
    if epi == "gate" and gate_rows == 1 and blocks(64, 64) <= cus:
        return GATE_RS
    return T64_4 if K >= 2048 and blocks(64, 64) <= cus else T64_3


def path(epi, M, N, K, hint=0, gate_rows=1, fuse=0, qk_norm=False, cus=256):
    """dispatch<EPI>() + launch<>() / launch_pp_t<>(): instantiation, K tiles, tile grid and tile walk.
    walk: ring kernels "m_major" (M > N) or "grouped" with ``shift`` from pick_group_shift (0 when a side has more than 256
    tiles); ping-pong "m_major", "grouped" (M > N and more than 4 n-tiles: pp_ngroup = 4) or "n_major"."""
    inst = select(epi, M, N, K, hint, gate_rows, fuse, qk_norm, cus)
    tm, tn = cdiv(M, inst.BM), cdiv(N, inst.BN)
    n_tiles = tm * tn
    if inst.kernel == "pp":
        ngroup = 4 if tn > 4 else 0
        walk = ("grouped" if ngroup else "m_major") if M > N else "n_major"
        n_cu = cus // 8 * 8 or 8
        grid = cdiv(n_tiles, 8) * 8 if n_tiles < n_cu else n_cu
        return Path(inst, epi, K // 64, tm, tn, walk, 0, n_tiles % 8, ngroup, n_tiles, grid, n_tiles % grid)
    if M > N:
        walk, shift = "m_major", 0
    else:
        walk, shift = "grouped", pick_group_shift(tm, tn, inst.BM, inst.BN) if tm <= 256 and tn <= 256 else 0
    return Path(inst, epi, K // 64, tm, tn, walk, shift, n_tiles % 8, 0, n_tiles, n_tiles, 0)


def ring_states(inst, KT):
    """The states of the LDS ring the K loop passes through, as a set of names.  Ring kernels: NPRO = NSTAGE - DSTEP tiles are
    issued ahead of the first hand-over; DSTEP == 2 also has the parity of KT / 2 (which register set holds the last tile);
    ping-pong: the parity of KT (which half of the ring the last K-tile sits in) and KT == 2 (nothing staged in the loop)."""
    if inst.kernel == "pp":
        return {"KT odd" if KT & 1 else "KT even"} | ({"KT == 2"} if KT == 2 else set())
    npro = inst.NSTAGE - inst.DSTEP
    st = {"KT < NPRO" if KT < npro else "KT == NPRO" if KT == npro else "KT > NSTAGE" if KT > inst.NSTAGE else "KT in (NPRO, NSTAGE]"}
    if inst.DSTEP == 2:
        st.add("KT/2 odd" if (KT // 2) & 1 else "KT/2 even")
    return st


def possible_ring_states(inst, fuse_consumer_k=False):
    """Every ring state of the instantiation that some K the host accepts reaches, and the ones no K reaches, with reasons."""
    want = {"KT odd", "KT even", "KT == 2"} if inst.kernel == "pp" else \
        {"KT < NPRO", "KT == NPRO", "KT > NSTAGE"} | ({"KT/2 odd", "KT/2 even"} if inst.DSTEP == 2 else set())
    never = {}
    npro = inst.NSTAGE - inst.DSTEP
    if inst.kernel == "ring" and npro == 1:
        never["KT < NPRO"] = "NSTAGE 2: one tile ahead, and K >= 64"
    if inst in (T64_4, PROD_C4):
        for s in ("KT < NPRO", "KT == NPRO"):
            never[s] = "selected only for K >= 2048: KT >= 32"
    if inst.FUSE == 1:
        # parts = K / 64 is a multiple of 4 up to 16: KT in {4, 8, 12, 16}
        for s in [x for x in want if not any(x in ring_states(inst, kt) for kt in (4, 8, 12, 16))]:
            never[s] = "a fused consumer has K / 64 = parts in {4, 8, 12, 16}"
    return want - set(never), never


def wave_rows(inst):
    return 128 if inst.kernel == "pp" else inst.BM // inst.WGM


def edge_flags(inst, epi, M, N, rps=0, lens=None):
    """partial last row / column tile, M == 1, a sequence boundary inside a wave tile, masked rows inside a tile."""
    f = set()
    if M % inst.BM:
        f.add("partial M tile")
    if N % inst.BN:
        f.add("partial N tile")
    if M == 1:
        f.add("M == 1")
    if epi in ("gate", "qkv") and rps:
        if any((s * rps) % wave_rows(inst) for s in range(1, cdiv(M, rps))):
            f.add("sequence boundary in a wave tile")
        if epi == "gate" and lens is not None and any(int(n) < min(rps, M - s * rps) for s, n in enumerate(lens)):
            f.add("masked rows in a tile")
    return f


def possible_edge_flags(inst, epis):
    want = {"partial M tile", "partial N tile", "M == 1"}
    never = {}
    if "gate" in epis or "qkv" in epis:
        want.add("sequence boundary in a wave tile")
    if "gate" in epis:
        want.add("masked rows in a tile")
    if inst.FUSE == 2:
        never["partial N tile"] = "the producer needs N % 64 == 0 and has 64-column tiles"
    if inst in (CONS_QKV, CONS_QKV_BIG):
        never["partial N tile"] = "selected only for N % 192 == 0"
    if inst in (CONS_WIDE, CONS_WIDE_BIG):
        never["partial N tile"] = "selected only for N % 128 == 0"
    if inst in (PROD_BIG6, PROD_BIG4):
        never["M == 1"] = "selected only past 256 tiles of 64 x 64"
    if inst == CONS_QKV_BIG:
        never["M == 1"] = "selected only past 256 tiles of 64 x 192"
    if inst == CONS_WIDE_BIG:
        never["M == 1"] = "with one row 64 x 128 tiles are as many as 128 x 128 ones, and every fused consumer has K % 128 == 0"
    return want - set(never), never


# ================================================================== cases

_CASE = dict(hint=0, gate_rows=1, fuse=0, qk_norm=False, rps=0, masked=False, bias=True, evalp=False, rope_heads=0, out="bf16")
Case = namedtuple("Case", ("epi", "M", "N", "K") + tuple(_CASE), defaults=tuple(_CASE.values()))


def cid(c):
    extra = [f"{k}={getattr(c, k)}" for k, v in _CASE.items() if getattr(c, k) != v]
    return f"{c.epi}:{c.M}x{c.N}x{c.K}" + ("," + ",".join(extra) if extra else "")


def case_lens(c):
    """seq_len of a masked case: every sequence loses a few rows, sequence 1 (if any) all but one, the last one none."""
    if not c.masked:
        return None
    S = cdiv(c.M, c.rps)
    lens = [max(1, c.rps - 3 * (s + 1)) for s in range(S)]
    if S > 2:
        lens[1] = 1
    if S > 1:
        lens[-1] = c.rps
    return lens


def case_path(c):
    return path(c.epi, c.M, c.N, c.K, c.hint, c.gate_rows, c.fuse, c.qk_norm)


def case_cells(c):
    p = case_path(c)
    walk = {p.walk if p.inst.kernel == "pp" or p.walk == "m_major" else f"grouped shift {p.shift}"}
    if p.n_main_mod8:
        walk.add("n_main % 8 != 0")
    if p.inst.kernel == "pp":
        if p.pp_ngroup and p.walk == "grouped" and p.tiles_n % 4:
            walk.add("pp_ngroup 4 with a narrower last group")
        if p.n_tiles > p.grid:
            walk.add("more tiles than workgroups")
        if p.extra:
            walk.add("extra > 0")
    return p, ring_states(p.inst, p.KT), edge_flags(p.inst, c.epi, c.M, c.N, c.rps, case_lens(c)), walk


def _bias_cases(shapes, hint, epis=_BIAS_EPIS):
    return tuple(Case(e, M, N, K, hint=hint, out="f32" if e == "f32" else "bf16") for e in epis for (M, N, K) in shapes)


# 64 x 64, 3 stages (hint 3): KT 1 (< NPRO), 2 (= NPRO), 3, 4, 5, 7 (> NSTAGE); M, N around the tile; both walks
S64 = ((1, 64, 64), (15, 4, 128), (16, 60, 192), (17, 68, 256), (63, 100, 320), (64, 128, 448), (65, 196, 64), (127, 260, 128),
       (129, 192, 384), (130, 64, 256), (257, 128, 64), (64, 1024, 64), (128, 2048, 64))
S64_4 = ((1, 64, 2048), (65, 196, 2048), (257, 128, 2048), (128, 512, 2048))              # 4 stages: K >= 2048, one round
S128 = ((1, 128, 64), (17, 68, 128), (127, 260, 192), (129, 128, 256), (130, 100, 320), (257, 196, 64), (128, 1024, 64),
        (256, 2048, 64), (65, 4, 448))
S128X64 = ((1, 64, 64), (17, 68, 128), (127, 260, 192), (129, 64, 256), (130, 100, 320), (257, 196, 448), (128, 1024, 64),
           (256, 2048, 64), (65, 4, 128))
SPP = ((1, 256, 128), (17, 68, 192), (257, 260, 128), (130, 100, 256), (300, 1300, 128), (1300, 300, 192), (2112, 1300, 128),
       (2112, 1536, 128), (4352, 4096, 128), (10753, 4, 128))
BIAS_CASES = _bias_cases(S64, 3) + _bias_cases(S64_4, 3) + _bias_cases(S128, 1) + _bias_cases(S128X64, 2) + \
    _bias_cases(SPP[:8], 9) + (Case("bf16", 4352, 4096, 128, hint=9), Case("f32", 4352, 4096, 128, hint=9, out="f32"),
                               Case("gelu", 4352, 4096, 128, hint=9), Case("bf16", 10753, 4, 128), Case("bf16", 2112, 1024, 64), Case("bf16", 1024, 2048, 64, hint=3),
                               Case("f32", 130, 256, 64, hint=3, out="f32"), Case("bf16", 130, 256, 2048, hint=3),
                               Case("bf16", 300, 512, 64, hint=1),
                               Case("f32", 1088, 1024, 64, out="f32"), Case("bf16", 65, 196, 128, hint=3, bias=False),
                               Case("f32", 257, 260, 128, hint=9, bias=False, out="f32"))


def _gate(M, N, K, rps, **kw):
    return Case("gate", M, N, K, rps=rps, out="f32", **kw)


GATE_CASES = (
    # role split 64 x 64, 4 stages (gate_rows 1, one round): KT 1, 2 (< NPRO), 3 (= NPRO), 5, 7 (> NSTAGE)
    _gate(1, 64, 64, 1), _gate(15, 4, 128, 5, masked=True), _gate(65, 68, 192, 13, masked=True, evalp=True),
    _gate(127, 260, 320, 127), _gate(130, 64, 448, 65, masked=True), _gate(257, 196, 64, 129, bias=False),
    _gate(64, 1024, 128, 16, masked=True), _gate(128, 2048, 64, 64), _gate(1, 128, 2048, 1), _gate(130, 256, 128, 65),
    # classic 64 x 64 (two gate rows, or past one round): 3 stages and, K >= 2048, 4
    _gate(1, 64, 64, 1, gate_rows=2, hint=3), _gate(17, 68, 128, 5, gate_rows=2, masked=True, evalp=True),
    _gate(65, 100, 192, 13, gate_rows=2, masked=True), _gate(130, 64, 320, 65, gate_rows=2),
    _gate(129, 260, 256, 43, gate_rows=2, masked=True, bias=False), _gate(64, 1024, 64, 16, gate_rows=2),
    _gate(128, 2048, 64, 32, gate_rows=2, masked=True), _gate(1088, 1024, 64, 136, masked=True),
    _gate(65, 196, 2048, 13, gate_rows=2, masked=True), _gate(257, 128, 2048, 129, gate_rows=2),
    _gate(128, 512, 2048, 64, gate_rows=2), _gate(2, 64, 2048, 1, gate_rows=2),
    # 128 x 128 (hint 1: the generic epilogue, TM x TN = 8) and 128 x 64 (hint 2: the prefetched one)
    _gate(1, 128, 64, 1, hint=1), _gate(17, 68, 128, 5, hint=1, gate_rows=2, masked=True, evalp=True),
    _gate(129, 128, 256, 43, hint=1, masked=True), _gate(257, 196, 64, 129, hint=1), _gate(127, 260, 192, 127, hint=1),
    _gate(128, 1024, 64, 32, hint=1, masked=True), _gate(256, 2048, 64, 64, hint=1),
    _gate(1, 64, 64, 1, hint=2), _gate(17, 68, 128, 5, hint=2, gate_rows=2, masked=True, evalp=True),
    _gate(129, 64, 256, 43, hint=2, masked=True), _gate(257, 196, 448, 129, hint=2), _gate(127, 260, 192, 127, hint=2),
    _gate(128, 1024, 64, 32, hint=2, masked=True), _gate(256, 2048, 64, 64, hint=2),
    # ping-pong: lean wave tiles (128 rows live, one gate row), general ones, both in one launch
    _gate(1, 256, 128, 1, hint=9), _gate(17, 68, 192, 5, hint=9, gate_rows=2, masked=True, evalp=True),
    _gate(600, 260, 128, 300, hint=9, masked=True), _gate(786, 512, 256, 131, hint=9, gate_rows=2),
    _gate(300, 1300, 128, 150, hint=9, masked=True), _gate(2112, 1300, 128, 528, hint=9, masked=True),
    _gate(2112, 1536, 192, 1056, hint=9), _gate(4352, 4096, 128, 1088, hint=9, masked=True),
)


def _qkv(M, heads, K, rps, **kw):
    return Case("qkv", M, 3 * heads * 64, K, rps=rps, **kw)


QKV_CASES = (
    _qkv(1, 1, 64, 1, hint=3), _qkv(17, 1, 128, 5, hint=3), _qkv(130, 1, 256, 65, hint=3), _qkv(65, 2, 320, 13, hint=3),
    _qkv(257, 1, 64, 129, hint=3), _qkv(64, 4, 64, 64, hint=3), _qkv(128, 16, 64, 32, hint=3),
    _qkv(65, 1, 2048, 13, hint=3), _qkv(257, 1, 2048, 129, hint=3), _qkv(1, 1, 2048, 1, hint=3), _qkv(128, 4, 2048, 32, hint=3),
    _qkv(1, 1, 64, 1, hint=1), _qkv(17, 1, 128, 5, hint=1), _qkv(257, 1, 192, 129, hint=1), _qkv(129, 2, 256, 43, hint=1),
    _qkv(128, 4, 64, 32, hint=1), _qkv(256, 16, 64, 64, hint=1),
    _qkv(1, 1, 64, 1, hint=2), _qkv(17, 1, 128, 5, hint=2), _qkv(257, 1, 192, 129, hint=2), _qkv(129, 2, 448, 43, hint=2),
    _qkv(128, 4, 64, 32, hint=2), _qkv(256, 16, 64, 64, hint=2),
    _qkv(1, 1, 128, 1, hint=9), _qkv(17, 1, 192, 5, hint=9), _qkv(393, 2, 128, 131, hint=9), _qkv(600, 5, 256, 300, hint=9),
    _qkv(300, 6, 128, 150, hint=9), _qkv(2112, 6, 128, 528, hint=9), _qkv(2112, 8, 192, 1056, hint=9),
)
# RoPE and qk_norm (which forces the 128-wide tile, and the ping-pong kernel under hint 9): toleranced
QKV_ROPE_CASES = (
    _qkv(65, 2, 128, 13, hint=3, rope_heads=1), _qkv(129, 2, 192, 43, hint=2, rope_heads=2),
    _qkv(129, 2, 256, 43, hint=1, rope_heads=2), _qkv(393, 2, 128, 131, hint=9, rope_heads=1),
    _qkv(65, 2, 128, 13, hint=3, rope_heads=1, qk_norm=True), _qkv(129, 2, 256, 43, rope_heads=2, qk_norm=True),
    _qkv(393, 2, 128, 131, hint=9, rope_heads=2, qk_norm=True),
)


def _prod(M, N, K, rps, **kw):
    return Case("gate", M, N, K, rps=rps, fuse=2, out="f32", **kw)


PRODUCER_CASES = (
    # role split, ring of six, two tiles per hand-over (K % 128 == 0): KT 2 (< NPRO), 4 (= NPRO), 6, 8, 10 (> NSTAGE)
    _prod(1, 64, 128, 1), _prod(65, 128, 256, 13, masked=True, evalp=True), _prod(130, 64, 384, 65, masked=True),
    _prod(257, 192, 512, 129), _prod(130, 256, 128, 65), _prod(64, 1024, 128, 16, masked=True), _prod(128, 2048, 640, 64), _prod(17, 256, 128, 5),
    # role split, 4 stages (K % 128 != 0): KT 1 (< NPRO), 3 (= NPRO), 5, 7
    _prod(1, 64, 64, 1), _prod(65, 128, 192, 13, masked=True, evalp=True), _prod(130, 64, 320, 65, masked=True),
    _prod(257, 192, 448, 129), _prod(130, 256, 64, 65), _prod(64, 1024, 64, 16, masked=True), _prod(128, 2048, 64, 64), _prod(17, 256, 192, 5),
    # 128 x 64 role split: past 256 tiles of 64 x 64, at most 256 of 128 x 64
    _prod(1088, 1024, 128, 136, masked=True), _prod(1089, 1024, 256, 363, masked=True, evalp=True), _prod(1088, 1088, 512, 1088),
    _prod(520, 2112, 128, 65), _prod(1088, 1024, 640, 272), _prod(770, 1536, 128, 385),
    _prod(1088, 1024, 64, 136, masked=True), _prod(1089, 1024, 192, 363, masked=True, evalp=True), _prod(1088, 1088, 320, 1088),
    _prod(520, 2112, 64, 65), _prod(1088, 1024, 448, 272), _prod(770, 1536, 64, 385),
    # classic producers: two gate rows (3 stages; 4 for K >= 2048 in one round), or past the 128-row round
    _prod(1, 64, 64, 1, gate_rows=2), _prod(2, 64, 64, 1, gate_rows=2), _prod(65, 128, 128, 13, gate_rows=2, masked=True, evalp=True),
    _prod(130, 64, 256, 65, gate_rows=2, masked=True), _prod(257, 192, 320, 129, gate_rows=2),
    _prod(64, 1024, 64, 16, gate_rows=2), _prod(128, 2048, 64, 32, gate_rows=2), _prod(130, 256, 128, 65, gate_rows=2), _prod(2112, 1024, 128, 528, masked=True),
    _prod(65, 128, 2048, 13, gate_rows=2, masked=True), _prod(257, 192, 2048, 129, gate_rows=2),
    _prod(128, 512, 2048, 64, gate_rows=2), _prod(1, 64, 2048, 1, gate_rows=2), _prod(130, 256, 2048, 65, gate_rows=2),
)


def _cons(epi, M, N, K, rps=0, **kw):
    return Case(epi, M, N, K, rps=rps or M, fuse=1, bias=False, out="f32" if epi == "f32" else "bf16", **kw)


CONSUMER_CASES = (
    # 64 x 192 (QKV, N % 192 == 0, one round): KT 4 (= NSTAGE), 8, 12
    _cons("qkv", 1, 192, 256, 1), _cons("qkv", 65, 192, 512, 13), _cons("qkv", 257, 192, 768, 129), _cons("qkv", 64, 768, 256, 16),
    _cons("qkv", 128, 3072, 256, 64),
    # 128 x 192: past 256 tiles of 64 x 192
    _cons("qkv", 1089, 3072, 256, 363), _cons("qkv", 2048, 768, 512, 1024), _cons("qkv", 1088, 3072, 768, 136),
    _cons("qkv", 1100, 1536, 256, 275), _cons("qkv", 520, 6144, 256, 130), _cons("qkv", 4100, 768, 256, 1025),
    # classic 64 x 64 for QKV: past the 128-row round, or ... (N is always a multiple of 192)
    _cons("qkv", 2112, 3072, 256, 528),
    # 64 x 128, ring of six: KT 4 (= NPRO), 8, 12 (KT / 2 is always even)
    _cons("bf16", 1, 128, 256), _cons("gelu", 65, 128, 512), _cons("f32", 257, 128, 768), _cons("bf16", 64, 1024, 256),
    _cons("gelu", 128, 2048, 256), _cons("f32", 130, 256, 512), _cons("f32", 1, 128, 256), _cons("gelu", 17, 256, 256),
    _cons("bf16", 257, 128, 768), _cons("bf16", 520, 1024, 256),
    # 128 x 128: past 256 tiles of 64 x 128
    _cons("bf16", 1089, 2048, 256), _cons("gelu", 1088, 2048, 512), _cons("f32", 2048, 1024, 256), _cons("bf16", 1100, 4096, 256),
    _cons("f32", 1089, 2048, 768), _cons("gelu", 2048, 128, 256), _cons("bf16", 520, 4096, 256), _cons("f32", 4100, 512, 256),
    # classic 64 x 64: N % 128 != 0, or past the 128-row round
    _cons("bf16", 1, 64, 256), _cons("gelu", 65, 68, 512), _cons("f32", 257, 196, 768), _cons("bf16", 64, 1088, 256),
    _cons("f32", 17, 4, 256), _cons("gelu", 2112, 2048, 256), _cons("bf16", 130, 320, 1024), _cons("f32", 128, 2112, 256),
    _cons("gelu", 1, 64, 256), _cons("f32", 1, 192, 512),
)

EXACT_CASES = BIAS_CASES + GATE_CASES + QKV_CASES + PRODUCER_CASES
ALL_CASES = EXACT_CASES + QKV_ROPE_CASES + CONSUMER_CASES


# ================================================================== exact inputs and expectations

def _ri(lo, hi, shape, seed):
    return torch.randint(lo, hi + 1, shape, generator=g(seed))


@functools.lru_cache(maxsize=4)
def int_operands(M, N, K):
    """a [M, K], w [N, K] int64 in [-3, 3] with the planted tie rows, bias [N] in [-8, 8] with bias[0] = bias[1] = 0."""
    s = 9000 + 131 * M + 17 * N + K
    a, w, bias = _ri(-3, 3, (M, K), s), _ri(-3, 3, (N, K), s + 1), _ri(-8, 8, (N,), s + 2)
    a[0] = 3
    a[0, 0] = 1
    w[0] = 0
    w[0, 0] = 1
    w[0, 1:29] = 3
    w[0, 29] = 2                      # 1 + 3 (28 * 3 + 2) = 259
    w[1] = -w[0]
    bias[:2] = 0
    return a, w, bias


@functools.lru_cache(maxsize=4)
def acc_i64(M, N, K):
    """a @ w.T in int64.  Large problems go through the fp64 matmul: every partial sum is an integer below 2^53, so it is
    the same number (tests/test_gemm_bf16_cpu.py compares the two where int64 is affordable)."""
    a, w, _ = int_operands(M, N, K)
    if M * N * K <= 1 << 24:
        return a @ w.T
    return (a.double() @ w.double().T).to(I64)


def pre_activation(c):
    """acc + bias, int64."""
    _, _, bias = int_operands(c.M, c.N, c.K)
    z = acc_i64(c.M, c.N, c.K)
    return z + bias if c.bias else z


def gelu_scale(c):
    """2^-s with |acc + bias| 2^-s <= 6: W and bias are multiplied by it, which keeps the accumulation exact."""
    top = float(pre_activation(c).abs().max())
    return 2.0 ** -max(0, math.ceil(math.log2(max(top, 1.0) / 6.0)))


def gate_operands(c):
    """resid [M, N] integers in [-64, 64], the gate table [evals 3][gate_rows][N] in [-2, 2] (never 0 on live rows' first
    column, so an update is visible), the evaluation index (2 with eval_ptr, else 0), seq_len or None, and ``live`` [M]."""
    s = 9500 + 131 * c.M + 17 * c.N + c.K
    resid = _ri(-64, 64, (c.M, c.N), s).float()
    table = _ri(-2, 2, (3, c.gate_rows, c.N), s + 1).float()
    table[:, :, 0] = 1.0
    lens = case_lens(c)
    m = torch.arange(c.M)
    live = torch.ones(c.M, dtype=torch.bool) if lens is None else (m % c.rps) < torch.tensor(lens)[m // c.rps]
    return resid, table, (2 if c.evalp else 0), lens, live


def gate_expect(c):
    """resid + gate[seq % gate_rows] * (acc + bias) on live rows, resid elsewhere; exact: |.| <= 64 + 2 (9 K + 8) < 2^24."""
    resid, table, e, _, live = gate_operands(c)
    seq = torch.arange(c.M) // c.rps
    upd = resid.double() + table[e][seq % c.gate_rows].double() * pre_activation(c).double()
    return torch.where(live[:, None], upd, resid.double())


def producer_operands(c):
    """row_mean [M] integers in [-4, 4], next_scale table [3][gate_rows][N] integers in [-2, 2]."""
    s = 9700 + 131 * c.M + 17 * c.N + c.K
    return _ri(-4, 4, (c.M,), s).float(), _ri(-2, 2, (3, c.gate_rows, c.N), s + 1).float()


def producer_expect(c, dtype=F64):
    """x_new (= gate_expect; the OLD x on masked rows), xs = bf16((x_new - rm) (1 + ns)) (exact integers before the rounding),
    stats [M][N / 64][2] = (mean of the tile - rm, M2 of the tile).  The mean is a sum of integers over 64: exact in fp32."""
    x_new = gate_expect(c)
    rm, ns = producer_operands(c)
    _, _, e, _, _ = gate_operands(c)
    seq = torch.arange(c.M) // c.rps
    xs = (x_new - rm.double()[:, None]) * (1.0 + ns[e][seq % c.gate_rows].double())
    tiles = x_new.to(dtype).view(c.M, c.N // 64, 64)
    mean = tiles.sum(2) / 64
    m2 = ((tiles - mean[..., None]) ** 2).sum(2)
    return x_new, xs, mean - rm.to(dtype)[:, None], m2


def consumer_operands(c):
    """stats [M, parts, 2] (tile means around 0.1, M2 around 64), row_mean [M], c, d [N] floats; parts = K / 64."""
    s = 9800 + 131 * c.M + 17 * c.N + c.K
    parts = c.K // 64
    stats = torch.empty(c.M, parts, 2)
    stats[..., 0] = torch.randn(c.M, parts, generator=g(s)) * 0.1
    stats[..., 1] = (torch.rand(c.M, parts, generator=g(s + 1)) + 0.5) * 64
    return stats, torch.randn(c.M, generator=g(s + 2)), torch.randn(c.N, generator=g(s + 3)), torch.randn(c.N, generator=g(s + 4))


def consumer_expect(c, dtype=F64, eps=1e-6, w_scale=1.0):
    """The kernel's contract: rstd (acc - mean c[n]) + d[n], mean = avg of the parts' means, M2 = sum M2_p + (K / parts) sum
    (mean_p - mean)^2 (Chan), rstd = (M2 / K + eps)^-1/2  -> (pre-epilogue value [M, N], mean [M])."""
    stats, _, cc, dd = consumer_operands(c)
    st = stats.to(dtype)
    parts = st.shape[1]
    mean = st[..., 0].sum(1) / parts
    m2 = (st[..., 1] + (c.K / parts) * (st[..., 0] - mean[:, None]) ** 2).sum(1)
    rstd = (m2 / c.K + eps) ** -0.5
    acc = acc_i64(c.M, c.N, c.K).to(dtype) * w_scale
    return rstd[:, None] * (acc - mean[:, None] * cc.to(dtype)) + dd.to(dtype), mean


# ================================================================== fragment-major layouts (gemm_bf16_epilogue.h)

def qk_offset(pos, d):
    """q / k: ((tile * 4 + (d >> 4)) * 32 + pr) * 16 + ((d >> 3) & 1) * 8 + (d & 7), tile = pos >> 5, pr = pos & 31."""
    tile, pr = pos >> 5, pos & 31
    return ((tile * 4 + (d >> 4)) * 32 + pr) * 16 + ((d >> 3) & 1) * 8 + (d & 7)


def v_offset(pos, d):
    """v^T: ((((tile * 2 + s16) * 2 + (d >> 5)) * 32 + (d & 31)) * 2 + hk) * 8 + jj with pr = pos & 31, s16 = pr >> 4,
    k16 = pr & 15, jj = ((k16 >> 3) << 2) | (k16 & 3), hk = (k16 >> 2) & 1."""
    tile, pr = pos >> 5, pos & 31
    s16, k16 = pr >> 4, pr & 15
    jj, hk = ((k16 >> 3) << 2) | (k16 & 3), (k16 >> 2) & 1
    return ((((tile * 2 + s16) * 2 + (d >> 5)) * 32 + (d & 31)) * 2 + hk) * 8 + jj


def frag_tables(n_pad):
    pos, d = torch.arange(n_pad)[:, None], torch.arange(64)[None, :]
    return qk_offset(pos, d), v_offset(pos, d)


def qkv_scatter(c, vals, n_pad, fill=SENTINEL):
    """vals [M, 3 * heads * 64] (any float dtype) -> three [S, heads, n_pad * 64] bf16 images: the fragment-major q, k and
    v^T buffers with ``fill`` at every pad position."""
    heads, S = c.N // 192, cdiv(c.M, c.rps)
    qi, vi = frag_tables(n_pad)
    m = torch.arange(c.M)
    seq, pos = m // c.rps, m % c.rps
    out = []
    for which, idx in ((0, qi), (1, qi), (2, vi)):
        buf = torch.full((S, heads, n_pad * 64), fill, dtype=BF)
        v = vals[:, which * heads * 64:(which + 1) * heads * 64].reshape(c.M, heads, 64).to(BF)
        for h in range(heads):
            buf[seq[:, None], h, idx[pos]] = v[:, h]
        out.append(buf)
    return out


def qkv_gather(c, bufs, n_pad):
    """The inverse on device results: three [S, heads, n_pad * 64] buffers -> [M, 3 * heads * 64] float."""
    heads = c.N // 192
    qi, vi = frag_tables(n_pad)
    m = torch.arange(c.M)
    seq, pos = m // c.rps, m % c.rps
    cols = []
    for buf, idx in zip(bufs, (qi, qi, vi)):
        cols.append(torch.stack([buf[seq[:, None], h, idx[pos]] for h in range(heads)], 1).reshape(c.M, heads * 64))
    return torch.cat(cols, 1).float()


def rope_table(rps):
    """cos_sin [rps][32][2] f32 as f5e_rope_table writes it (angles pos / 10000^(2 i / 64)), computed in fp64."""
    inv = 1.0 / (10000 ** (torch.arange(0, 64, 2).double() / 64))
    ang = torch.outer(torch.arange(rps).double(), inv)
    return torch.stack([ang.cos(), ang.sin()], -1).float()


def qkv_rope_expect(c, cs, qn_w, kn_w, dtype=F64):
    """(acc + bias) -> optional RMSNorm over each q / k head (eps 1e-6, weights qn_w / kn_w) -> RoPE on the first rope_heads
    heads of q and k -> q times QSCALE; v untouched.  [M, 3 * heads * 64] before the bf16 rounding, in ``dtype``."""
    heads = c.N // 192
    v = pre_activation(c).to(dtype).view(c.M, 3, heads, 64).clone()
    pos = torch.arange(c.M) % c.rps
    if c.qk_norm:
        for which, wt in ((0, qn_w), (1, kn_w)):
            t = v[:, which]
            v[:, which] = t * ((t * t).sum(-1, keepdim=True) / 64 + 1e-6) ** -0.5 * wt.to(dtype)
    t = cs.to(dtype)[pos]                                # [M, 32, 2]
    co, si = t[:, None, :, 0], t[:, None, :, 1]
    for which in (0, 1):
        x = v[:, which, :c.rope_heads]
        x0, x1 = x[..., 0::2].clone(), x[..., 1::2].clone()
        x[..., 0::2] = x0 * co - x1 * si
        x[..., 1::2] = x1 * co + x0 * si
    v[:, 0] = v[:, 0] * torch.tensor(QSCALE, dtype=dtype)
    return v.reshape(c.M, c.N)
