"""The host logic behind the prefetch-hosting launches of f5e_dit_forward, restated in tests/dit_chain_ref.py and pinned here
without a GPU: the grid tail of ``launch()`` (csrc/gemm_bf16.hip), the kernel pick of ``f5e_flash_attn_pf`` (csrc/attention.hip),
the scheme-0 assignment of csrc/runtime.hip, the byte ranges the prefetch workgroups walk (f5e_common.h), and the coverage of the
case list that tests/test_dit_chain_gpu.py runs: every hosting state and attention kernel of ``REQUIRED`` must be reached by
some case on 256 CUs, and every case must reach the states it names."""
import pytest
import torch

import dit_chain_ref as C
import gemm_bf16_ref as R

KIB, MIB = 1024, 1024 * 1024


def states(S, N, L=1, cus=256):
    return {(x.op, x.block): x for x in C.chain_hosting(S, N, 1024, 16, 2048, L, 100, cus)}


def test_lds_and_granule_of_the_hosting_instantiations():
    """``lds`` and ``gran`` of launch() for the fused kernels: only the four-stage 64 x 64 producer fits twice into a CU's LDS,
    so it alone of the role-split kernels keeps 32 KiB granules whatever the idle count."""
    lds = {n: C.lds_bytes(R.NAMES[n]) for n in R.NAMES if R.NAMES[n].kernel == "ring"}
    assert lds["PROD_RS6"] == 97 * KIB and lds["PROD_RS4"] == 65 * KIB and lds["PROD_BIG6"] == 146 * KIB
    assert lds["CONS_QKV"] == 129 * KIB and lds["CONS_QKV_BIG"] == 122 * KIB and lds["CONS_WIDE"] == 145 * KIB
    assert lds["CONS_WIDE_BIG"] == 130 * KIB and lds["PROD_C3"] == 49 * KIB and lds["CONS_C3"] == 49 * KIB
    assert all(v <= 160 * KIB for v in lds.values())
    packs = {n for n, v in lds.items() if R.NAMES[n].NLOAD and 2 * v > 160 * KIB}
    assert packs == {"PROD_RS6", "PROD_BIG6", "PROD_BIG4", "CONS_QKV", "CONS_QKV_BIG", "CONS_WIDE", "CONS_WIDE_BIG"}
    assert C.dma_granule(R.PROD_RS6) == 8 * KIB and C.dma_granule(R.CONS_QKV) == 16 * KIB and C.dma_granule(R.PROD_BIG6) == 12 * KIB


def test_grid_tail_rules():
    g = C.gemm_hosting
    # role split, one workgroup per CU: granules while they fit on the idle CUs, packed past that, nothing on a full chip
    assert g(R.PROD_RS6, 128, 4 * MIB) == C.Host("granules", 128, 0)
    assert g(R.PROD_RS6, 128, 4 * MIB + 1) == C.Host("packed", 104, 40 * KIB)          # 129 granules over 128 CUs, 8 KiB steps
    assert g(R.PROD_RS6, 128, 6 * MIB) == C.Host("packed", 128, 48 * KIB)
    assert g(R.PROD_RS6, 255, 6 * MIB) == C.Host("packed", 1, 6 * MIB)
    assert g(R.PROD_RS6, 256, 6 * MIB) == C.NONE and g(R.PROD_RS6, 300, 6 * MIB, cus=304) == C.Host("packed", 4, 1536 * KIB)
    assert g(R.CONS_QKV, 240, 2 * MIB) == C.Host("packed", 16, 128 * KIB)
    assert g(R.PROD_BIG6, 144, 4 * MIB) == C.Host("packed", 86, 48 * KIB)              # ceil(4 MiB / 112) -> 12 KiB steps
    # two of its workgroups fit a CU: no packing, no idle rule
    assert g(R.PROD_RS4, 256, 4 * MIB) == C.Host("granules", 128, 0)
    # classic kernels: four waves host up to 768 main workgroups, eight-wave tiles never
    assert g(R.PROD_C3, 768, 4 * MIB) == C.Host("granules", 128, 0) and g(R.PROD_C3, 769, 4 * MIB) == C.NONE
    assert g(R.CONS_C3, 1584, 2 * MIB) == C.NONE and g(R.T128, 64, 4 * MIB) == C.NONE and g(R.T64_3, 64, 100) == C.Host("granules", 1, 0)
    assert g(R.PROD_RS6, 16, 0) == C.NONE


@pytest.mark.parametrize("inst,n_main,nbytes", [(R.PROD_RS6, 128, 6 * MIB), (R.PROD_RS6, 240, 204800), (R.PROD_RS6, 253, 204800),
                                                (R.CONS_QKV, 240, 2 * MIB), (R.PROD_BIG6, 144, 4 * MIB), (R.PROD_C3, 528, 204800),
                                                (R.PROD_RS6, 128, 204800), (R.CONS_WIDE, 255, 4 * MIB + 48)])
def test_prefetch_workgroups_cover_the_range_and_stay_inside(inst, n_main, nbytes):
    """The 16-byte loads of the grid tail (f5e_prefetch_run<256> / f5e_prefetch_run_packed) touch every whole 16-byte piece of
    [0, nbytes) exactly once and nothing at or past nbytes - 15: the ``off + 16 <= b0`` bound with a partial last granule."""
    host = C.gemm_hosting(inst, n_main, nbytes)
    assert host.kind != "none"
    nt = 256 if host.kind == "granules" else 64 * (inst.WGM * inst.WGN + inst.NLOAD)
    assert host.kind == "granules" or (host.per_wg % (nt * 16) == 0 and host.n <= 256 - n_main)
    off = C.prefetch_offsets(host, nt, nbytes)
    assert torch.equal(off, torch.arange(nbytes // 16) * 16)


def test_attention_pick():
    a = C.attn_pick
    assert a(2, 16, 33)[:3] == ("<1>", 64, True) and a(2, 16, 33).ktiles == 1
    assert a(2, 16, 130)[:3] == ("<2>", 128, True) and a(1, 4, 96).kernel == "<2>" and a(1, 16, 192).kernel == "<2>"
    assert a(1, 16, 469)[:3] == ("b1", 256, True) and a(2, 16, 512).kernel == "b1" and a(2, 16, 512).grid == 512
    assert a(1, 16, 530).kernel == "<4>" and a(1, 16, 513).kernel == "<4>"
    assert a(2, 16, 530)[:3] == ("<1>", 64, True) and a(2, 16, 530).grid == 544          # past two workgroups per CU: unsplit
    assert a(2, 16, 530, cus=304).kernel == "<4>"
    assert a(8, 16, 1875).kernel == "<1>" and a(9, 16, 1875)[:3] == ("lds", 256, False)   # 8192 query tiles: LDS-shared, no tail
    assert a(1, 2, 130, splits=-1).hosts is False and a(1, 2, 33, splits=4).kernel == "b1" and a(3, 2, 513, splits=2).kernel == "<2>"


def test_scheme_0_and_the_hand_derived_shapes():
    """The table of tests/test_dit_chain_gpu.py's docstring, D = 1024, H = 16, FF = 2048, 256 CUs."""
    s = states(1, 469, L=2)
    assert [(x.op, x.weight, x.nbytes) for x in C.chain_hosting(1, 469, 1024, 16, 2048, 2)] == \
        [("qkv", "w_out", 2 * MIB), ("attn", "w_ff1", 4 * MIB), ("out", "w_ff2", 4 * MIB), ("ff1", None, 0), ("ff2", "w_qkv", 6 * MIB),
         ("qkv", "w_out", 2 * MIB), ("attn", "w_ff1", 4 * MIB), ("out", "w_ff2", 4 * MIB), ("ff1", None, 0), ("ff2", "w_proj", 204800)]
    assert all(s[k].n_main == 128 for k in (("qkv", 0), ("out", 0), ("ff1", 0), ("ff2", 0)))
    assert (s["qkv", 0].inst, s["out", 0].inst, s["ff1", 0].inst) == (R.CONS_QKV, R.PROD_RS6, R.CONS_WIDE)
    assert s["qkv", 0].host == C.Host("granules", 64, 0) and s["out", 0].host == C.Host("granules", 128, 0)
    assert s["ff1", 0].host == C.NONE and s["ff2", 0].host == C.Host("packed", 128, 49152) and s["ff2", 1].host == C.Host("granules", 7, 0)
    assert s["attn", 0].inst.kernel == "b1" and s["attn", 0].host == C.Host("granules", 128, 0)
    s = states(2, 469, L=2)
    assert s["qkv", 0].n_main == 240 and {s[k].host.kind for k in (("qkv", 0), ("out", 0), ("ff2", 0))} == {"packed"}
    assert s["ff2", 1].host == C.Host("granules", 7, 0) and s["attn", 0].inst.kernel == "b1"
    s = states(2, 512)
    assert s["qkv", 0].n_main == 256 and {s[k].host for k in (("qkv", 0), ("out", 0), ("ff2", 0))} == {C.NONE}
    assert s["attn", 0].inst.kernel == "b1" and s["attn", 0].host.n == 128
    s = states(2, 530, L=2)
    assert (s["qkv", 0].inst, s["out", 0].inst, s["ff1", 0].inst, s["ff2", 0].inst) == (R.CONS_QKV_BIG, R.PROD_BIG6, R.CONS_WIDE_BIG, R.PROD_BIG6)
    assert s["qkv", 0].n_main == 144 and s["qkv", 0].host.kind == "granules" and s["out", 0].host.kind == s["ff2", 0].host.kind == "packed"
    assert s["attn", 0].inst[:2] == ("<1>", 64)
    assert states(1, 530)["attn", 0].inst.kernel == "<4>" and states(2, 130)["attn", 0].inst.kernel == "<2>"
    assert states(2, 33)["attn", 0].inst[:2] == ("<1>", 64) and states(2, 33)["attn", 0].inst.ktiles == 1
    s = states(3, 704)
    assert (s["qkv", 0].inst, s["out", 0].inst, s["ff2", 0].inst) == (R.CONS_C3, R.PROD_C3, R.PROD_C3)
    assert s["qkv", 0].n_main == 1584 and s["qkv", 0].host == C.NONE and s["out", 0].n_main == 528 and s["out", 0].host.kind == "granules"


def test_case_list_reaches_every_required_state():
    reached = set().union(*(C.case_tags(c) for c in C.CASES))
    missing = [t for t in C.REQUIRED if t not in reached]
    assert not missing, f"no case of dit_chain_ref.CASES reaches: {missing}"
    unknown = reached - set(C.REQUIRED)
    assert not unknown, f"states without a name in REQUIRED: {sorted(unknown)}"


@pytest.mark.parametrize("c", C.CASES, ids=C.cid)
def test_case_reaches_the_states_it_names_and_stays_small(c):
    missing = set(c.expect) - C.case_tags(c)
    assert not missing, f"{C.cid(c)} does not reach {sorted(missing)}; it reaches {sorted(C.case_tags(c))}"
    assert set(c.expect) <= set(C.REQUIRED)
    D, H, FF = C.dims(c)
    assert c.L <= 3 and c.S * c.N <= 2112 and c.S % c.B == 0 and c.S * c.N <= C.LN_FUSE_MAX_ROWS
    assert (c.fused and not c.per_item and "qn" not in c.arch) or not c.fused
    if c.lens:
        assert len(c.lens) == c.S and max(c.lens) == c.N and min(c.lens) <= c.N - 64      # one sequence a whole key tile short


def test_case_list_covers_the_further_cases():
    cs = C.CASES
    assert {c.L for c in cs if c.fused and c.arch == "base"} == {1, 3}
    assert {c.N for c in cs if c.fused and c.arch == "tiny"} == {33, 96}
    assert any(c.lens for c in cs if c.fused) and any(c.lens for c in cs if not c.fused)
    assert any(c.per_item and c.B > 1 for c in cs) and any(c.arch == "tiny_qn_skip" for c in cs)
    assert len({C.cid(c) for c in cs}) == len(cs)
