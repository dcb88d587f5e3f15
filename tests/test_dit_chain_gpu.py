"""f5e_dit_forward (csrc/runtime.hip:184-332) pinned to its op-by-op assembly, Infinity-Cache prefetch hosting included.

``tests/dit_chain_ref.py::assemble`` re-issues one evaluation launch for launch through the public entry points of
f5e_tts_amd.ops, which launch WITHOUT prefetch workgroups (its docstring lists the mirrored sequence with runtime.hip line
numbers).  Three arenas with the layout of f5e_workspace_bytes, each with spare bytes on both sides, sentinel-filled except the
zeroed q / k / vt range, take the same evaluation: ``ops.dit_forward`` with ``mall_prefetch = 1`` (the production launches:
``grid = n_main + pf_wgs``), with ``mall_prefetch = 0``, and the assembly.  After the evaluation, and again after a second one
with another ``eval_ptr`` value, the three buffers must be equal BYTE FOR BYTE: every workspace buffer, ``pred`` included, the
alignment gaps and the spare bytes.  No buffer is held to less than that, so there is no tolerance in this file except
``close`` of tests/test_ops_gpu.py in the flash_attn edge cases.  Bitwise equality holds because ``dispatch<EPI>()`` and
``f5e_flash_attn_pf`` pick instantiation and tile order from M, N, K, ln and n_main only, never from the prefetch hint, and the
kernels are deterministic (tests/test_e2e_gpu.py::test_graph_equals_eager_bitwise relies on the same).

Containment: the spare bytes and the gaps between buffers keep the sentinel, the q / k / vt pad positions stay zero, and byte
copies of y, in_const, mod, cd, the rope table, seq_len, eval_ptr and every weight tensor of the engine taken before the runs
equal the tensors after them (the prefetch workgroups only load: a store through a stale pointer would show here).

Cases (tests/dit_chain_ref.py::CASES; D = 1024, H = 16, FF = 2048 unless "tiny": D = 256, H = 4, FF = 512) and the hosting states
they reach on 256 CUs, asserted against the device's real CU count through the same model before anything runs:
  S 1 N 469 L 3   128 main workgroups, idle 128: QKV (w_out) and OUT (w_ff2) granules, FF2 (6 MiB w_qkv) packed 128 x 49152 B,
                  the last FF2 hosts w_proj (200 KB: a partial 7th granule); batch-1 attention kernel hosting w_ff1
  S 2 N 469 L 1   240 main, idle 16: every GEMM packed (w_proj: 7 granules); batch-1 attention; sequence 1 a key tile short
  S 2 N 512 L 1   256 main = the chip: the GEMMs host nothing; batch-1 attention (512 query tiles) still hosts
  S 2 N 530 L 3   128-row role-split tiles (144 main): QKV granules, OUT / FF2 packed; 544 query tiles: unsplit <1> hosting
  S 1 N 530 L 1   general <4> (9 key tiles, 272 query tiles)
  S 2 N 130 L 1   <2> (3 key tiles); sequence 1 a key tile short
  S 2 N 33  L 3   <1> with one key tile; 32 main workgroups: every GEMM granules, middle blocks included
  S 3 N 704 L 1   classic FUSE kernels: QKV 1584 main (> 768: hosts nothing), OUT / FF2 528 main (hosts 32 KiB granules)
  tiny N 33 / 96  the cheapest fused chains (<1>, <2>)
  plain           separate LayerNorms with per-item times (mod_rows = B), qk_norm = rms_norm and the long skip connection

The sampler-level test runs CFM.sample with the engine's prefetch switch off and on, eagerly and from graphs.

flash_attn edges (the chain is their only caller): kv_len[s] = 0 gives all-zero rows and kv_len[s] > rows_per_seq is clamped,
for the <1>, <2>, <4>, batch-1 and LDS-shared kernels, into an output view with ldo = H * 64 + 8 whose surroundings must keep the
sentinel.  These cases found a bug: the merge of the split kernels (attn_fwd_kernel<2 / 4>, attn_fwd_b1_kernel) computed
exp2(m - m_new) with every wave's m = -inf when a sequence has no key, i.e. exp2(NaN), and stored NaN rows; the merge now clamps
m_new to -FLT_MAX, which leaves every other case bit-identical."""
import functools
import threading

import pytest
import torch

import dit_chain_ref as R
import fp32_ops_ref as F
from oracle import f5e_oracle as O
from test_e2e_gpu import SMALL, build
from test_fp32_ops_gpu import Placed
from test_ops_gpu import QSCALE, close, g, pack_qkv
from tools import synth as SY

pytestmark = pytest.mark.gpu

BF, I32 = torch.bfloat16, torch.int32


@pytest.fixture(scope="module")
def ops():
    import f5e_tts_amd.ops as ops_mod
    ops_mod.require_device()
    return ops_mod


@functools.lru_cache(maxsize=None)
def model_for(arch, L):
    sd, dit, cfm = build(O.DiTConfig(**dict(SMALL, depth=L, **R.ARCH[arch])))
    return dit, cfm


def first_difference(ch, plan, a, b):
    """Names the first buffer (WS_NAMES order = launch order of its writer) in which two arena buffers differ."""
    ne = a != b
    for name, lo, hi in ch.used(plan):
        n = int(ne[lo:hi].sum())
        if n:
            return f"{name}: {n} of {hi - lo} bytes differ, first at byte {int(ne[lo:hi].nonzero()[0])}"
    return f"outside every buffer: {int(ne.sum())} bytes differ, first at byte {int(ne.nonzero()[0])} of the spared arena"


@pytest.mark.parametrize("c", R.CASES, ids=R.cid)
def test_forward_equals_assembly_and_prefetch_off_bitwise(ops, c):
    from f5e_tts_amd import _C
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    missing = set(c.expect) - R.case_tags(c, cus)
    assert not missing, f"on {cus} CUs this case no longer reaches {sorted(missing)}"
    eng = model_for(c.arch, c.L)[0].engine()
    assert eng.L == c.L and (eng.can_fuse_ln or not c.fused)
    ch = R.Chain(c, eng, _C.WS_NAMES)
    inputs = ch.inputs()
    before = [t.clone() for t in inputs]
    runs = []
    for name in ("forward, hosting on", "forward, hosting off", "assembly"):
        buf, plan = ch.new_arena()
        if c.fused:
            plan.c.mall_prefetch = 1 if name.endswith("on") else 0
        else:
            assert plan.c.mall_prefetch == 0
        runs.append((name, buf, plan))
    fresh = runs[0][1].clone()
    assert all(torch.equal(fresh, buf) for _, buf, _ in runs)
    preds = []
    for e in (2, 1):
        ch.eval_ptr.fill_(e)
        for name, buf, plan in runs:
            if name == "assembly":
                R.assemble(ops, ch, ch.views(buf, plan))
            else:
                ops.dit_forward(plan.c)
        torch.cuda.synchronize()
        assert ch.eval_ptr.tolist() == [e], "eval_ptr changed"
        ref_name, ref, plan = runs[0]
        for name, buf, _ in runs[1:]:
            assert torch.equal(ref, buf), f"evaluation {e}: '{ref_name}' vs '{name}': {first_difference(ch, plan, ref, buf)}"
        pred = ch.views(ref, plan)["pred"]
        assert torch.isfinite(pred).all() and not (pred == R.SENTINEL).any()
        preds.append(pred.clone())
    assert not torch.equal(preds[0], preds[1]), "eval_ptr did not select another evaluation's tables"
    # containment: spare bytes and alignment gaps, q / k / vt pads, inputs
    name, buf, plan = runs[0]            # the three buffers are equal: one check covers them all
    used = ch.used(plan)
    edges = [0] + [x for _, lo, hi in used for x in (lo, hi)] + [buf.numel()]
    assert edges == sorted(edges) and edges[1] == R.SPARE
    for lo, hi in zip(edges[0::2], edges[1::2]):
        assert torch.equal(buf[lo:hi], fresh[lo:hi]), f"bytes [{lo}, {hi}) outside every buffer changed"
    v = ch.views(buf, plan)
    N, n_pad = c.N, plan.c.n_pad
    if n_pad > N:
        qi, vi = ops.qk_frag_index(n_pad)[N:].reshape(-1).cuda(), ops.v_frag_index(n_pad)[N:].reshape(-1).cuda()
        for nm, idx in (("q", qi), ("k", qi), ("vt", vi)):
            pads = v[nm].reshape(c.S, eng.cfg.heads, -1)[:, :, idx]
            assert not pads.view(torch.int16).any(), f"{nm}: a pad position was written"
    for t, b in zip(inputs, before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), "an input or weight tensor changed"


def test_sampler_prefetch_on_equals_off(monkeypatch):
    """CFM.sample with the engine's Infinity-Cache prefetch off, then on: eager launches, the one-step graph and the whole-loop
    graph must all return the same output and trajectory.  The cached loop states (which hold the plans) are dropped in
    between; a spy on make_plan confirms that the switch reached the plans."""
    sd, dit, cfm = build(O.DiTConfig(**SMALL))
    eng = dit.engine()
    assert eng.can_fuse_ln and eng.fuse_ln
    wav = SY.synthetic_ref_wave(40).cuda()
    text = SY.synthetic_text_ids(90, vocab=300)
    kw = dict(duration=90, steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
    seen, make_plan = [], eng.make_plan

    def spy(*a, **k):
        p = make_plan(*a, **k)
        seen.append(int(p.c.mall_prefetch))
        return p

    monkeypatch.setattr(eng, "make_plan", spy)
    res = {}
    for graph in (False, True):
        cfm.use_graph = graph
        for on in (False, True):
            eng.mall_prefetch = on
            eng._loops = threading.local()            # drop the cached plans and graphs
            del seen[:]
            for form in range(3 if graph else 1):     # with graphs: eager launches, the one-step graph, the whole-loop graph
                o, t = cfm.sample(wav, text, **kw)
                res[(graph, on, form)] = (o.clone(), t.clone())
            assert seen and set(seen) == {int(on)}, (graph, on, seen)
    ref = res[(False, False, 0)]
    assert torch.isfinite(ref[0]).all()
    for key, (o, t) in res.items():
        assert torch.equal(o, ref[0]) and torch.equal(t, ref[1]), f"(graph, prefetch, call) = {key} differs from eager, prefetch off"


# ------------------------------------------------------------------ flash_attn edges

@functools.lru_cache(maxsize=None)
def attn_edge_inputs(N):
    """S = 3, H = 2 with the seeds of tests/test_ops_gpu.py::test_flash_attn; kv_len = (0, N + 7, N - 5): no key at all, more
    keys than rows (clamped to N) and an ordinary masked sequence -> (q, k, v bf16 [S, H, N, 64], lens, reference [S N, H 64])."""
    S, H = 3, 2
    q = (torch.randn(S, H, N, 64, generator=g(12)) * QSCALE).to(BF)
    k = torch.randn(S, H, N, 64, generator=g(13)).to(BF)
    v = torch.randn(S, H, N, 64, generator=g(14)).to(BF)
    lens = torch.tensor([0, N + 7, N - 5], dtype=I32)
    s = (q.float() @ k.float().transpose(-1, -2)) * 0.6931471805599453           # 2^(q' k) = e^(q k / 8)
    km = torch.arange(N)[None, :] < lens.clamp(max=N)[:, None]
    p = torch.softmax(s.masked_fill(~km[:, None, None, :], float("-inf"))[1:], -1)
    ref = torch.cat([torch.zeros(1, H, N, 64), p @ v.float()[1:]]).transpose(1, 2).reshape(S * N, H * 64)
    return q, k, v, lens, ref


@pytest.mark.parametrize("N", [33, 469, 513])
@pytest.mark.parametrize("waves", [1, 2, 4, -1])
def test_flash_attn_no_key_and_too_many_keys_contained(ops, N, waves):
    """waves 1 / 2: attn_fwd_kernel<1 / 2>; 4: the batch-1 kernel (N <= 512) or the general <4>; -1: LDS-shared.  The output is a
    view 8 elements into a sentinel-filled buffer with ldo = H * 64 + 8 and two spare rows."""
    S, H = 3, 2
    q, k, v, lens, ref = attn_edge_inputs(N)
    n_pad = (N + 63) // 64 * 64
    qd, kd, vtd = pack_qkv(ops, q, k, v, n_pad)
    ld = H * 64 + 8
    out = Placed(torch.full((S * N, H * 64), R.SENTINEL, dtype=BF), 8, ld)
    whole_rows = out.dflat[8:8 + S * N * ld].view(S * N, ld)        # the same memory as out.v, as the contiguous tensor ops takes
    assert whole_rows.data_ptr() == out.v.data_ptr() and whole_rows.stride(0) == out.v.stride(0) == ld
    ops.flash_attn(qd, kd, vtd, whole_rows, N, kv_len=lens.cuda(), waves=waves)
    torch.cuda.synchronize()
    flat = out.dflat.cpu()
    got = F.view(flat, out.spec).clone()
    F.view(flat, out.spec).fill_(R.SENTINEL)          # what is left is everything outside [0, S N) x [0, H 64)
    assert bool((flat == R.SENTINEL).all()), f"flash_attn wrote {int((flat != R.SENTINEL).sum())} elements outside its output"
    assert not (got[:N] != 0).any(), f"kv_len = 0: {int((got[:N] != 0).sum())} output elements are not zero (NaN counts)"
    close(got, ref, 2 ** -6, 6e-3, f"attention, kv_len {lens.tolist()}")
