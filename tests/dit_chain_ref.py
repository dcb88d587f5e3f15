"""f5e_dit_forward (csrc/runtime.hip) restated for its tests: which launch of an evaluation hosts which Infinity-Cache prefetch
(the grid tail of ``launch()`` in csrc/gemm_bf16.hip and the kernel pick of ``f5e_flash_attn_pf`` in csrc/attention.hip, in plain
Python on top of the dispatch of tests/gemm_bf16_ref.py), the case list of tests/test_dit_chain_gpu.py with the states every
case names, and the op-by-op assembly of one evaluation through f5e_tts_amd.ops.  tests/test_dit_chain_cpu.py pins the model
and asserts that the case list reaches every hosting state; tests/test_dit_chain_gpu.py runs the cases.  Nothing at module
level imports f5e_tts_amd: the device helpers take ``ops`` and the engine as arguments.

The launch sequence that ``assemble`` mirrors (runtime.hip line numbers):
  196-197  gemm_f32: input projection, in_const as addend, h0 and its bf16 copy
  199-200  convpos twice; the second adds the residual h0 into x
  202-206  long skip: device copy of x into skip_res
  fused AdaLN (207-303):  222-223 adaln_pre;  per block 282-283 gemm_bf16_qkv_rope(consumer), 284-285 flash_attn (auto),
           286-289 gemm_bf16_gate_residual(producer, seq_len, next_scale = scale_mlp), 290-292 gemm_bf16_bias(GELU, consumer),
           294-297 gemm_bf16_gate_residual(producer, next_scale = block l + 1's scale_msa or the final AdaLN's scale);
           299-301 gemm_bf16_bias consumer with f32 output
  separate LayerNorm (304-331):  per block 307 layernorm, 309 gemm_bf16_qkv_rope(bias, qk_norm weights), 311 flash_attn,
           312 gemm_bf16_gate_residual(seq_len), 314 layernorm, 316 gemm_bf16_bias(GELU), 317 gemm_bf16_gate_residual;
           320-325 long skip: two gemm_f32;  328 layernorm;  330 gemm_bf16_bias with f32 output

Who hosts what is scheme 0 of runtime.hip (the only one the shipped library has): QKV -> w_out, attention -> w_ff1, OUT -> w_ff2,
FF1 nothing, FF2 -> the next block's w_qkv or, after the last block, w_proj.  Every ``F5ePrefetch`` of scheme 0 has ONE range
(ptr[1] is null everywhere); the two-range branch of ``f5e_prefetch_run`` is reached by schemes 1-4 only, which exist behind a
switch of the diagnostics build, so no case here reaches it."""
from collections import namedtuple

import torch

import gemm_bf16_ref as R

BF, F32, I32, U8 = torch.bfloat16, torch.float32, torch.int32, torch.uint8
cdiv = R.cdiv
PF_BYTES_PER_WG = 32 * 1024          # F5E_PF_BYTES_PER_WG of f5e_common.h
PF_MAX_MAIN = 3 * 256                # launch(): prefetch workgroups ride along up to this many main workgroups
LN_FUSE_MAX_ROWS = 2800              # engine.DiTEngine.LN_FUSE_MAX_ROWS
SPARE = 1024                         # spare bytes in front of and behind every test arena
SENTINEL = R.SENTINEL


# ================================================================== the grid tail of launch(), restated

Host = namedtuple("Host", "kind n per_wg")      # kind: "none", "granules" (n workgroups of 32 KiB) or "packed" (n of per_wg bytes)
NONE = Host("none", 0, 0)


def lds_bytes(inst):
    """``lds`` of launch(): NSTAGE (BM + BN) BK 2 bytes of ring + BM * 16 of statistics scratch for a fused kernel."""
    return inst.NSTAGE * (inst.BM + inst.BN) * 64 * 2 + (inst.BM * 16 if inst.FUSE else 0)


def prefetch_wgs(nbytes):
    """f5e_prefetch_wgs for one range."""
    return cdiv(nbytes, PF_BYTES_PER_WG)


def dma_granule(inst):
    """One LDS-DMA of every thread of the workgroup: 64 (WGM WGN + NLOAD) 16 bytes."""
    return 64 * (inst.WGM * inst.WGN + inst.NLOAD) * 16


def gemm_hosting(inst, n_main, nbytes, cus=256):
    """launch<>() of gemm_bf16.hip from ``pf_wgs`` to ``grid``: what an instantiation with n_main main workgroups appends for
    nbytes of hosted weights on a chip of ``cus`` CUs."""
    assert inst.kernel == "ring"          # the ping-pong kernel takes no prefetch (and the fused chain never selects it)
    pf = prefetch_wgs(nbytes) if (inst.WGM * inst.WGN == 4 or inst.NLOAD > 0) and n_main <= PF_MAX_MAIN else 0
    per = 0
    if inst.NLOAD > 0 and 2 * lds_bytes(inst) > 160 * 1024 and pf > 0:        # one workgroup per CU by LDS: pack onto the idle CUs
        idle = cus - n_main
        if idle <= 0:
            pf = 0
        elif pf > idle:
            gran, total = dma_granule(inst), pf * PF_BYTES_PER_WG
            per = cdiv(cdiv(total, idle), gran) * gran
            pf = cdiv(total, per)
    if pf == 0:
        return NONE                                                            # grid == n_main -> a.pf = {}
    return Host("packed" if per else "granules", pf, per)


def prefetch_offsets(host, nt, nbytes):
    """Byte offsets of the 16-byte loads that the prefetch workgroups of ``host`` issue over a range of nbytes, sorted:
    f5e_prefetch_run<NT> (granules; NT threads, the GEMM's first 256) and f5e_prefetch_run_packed (nt = all threads)."""
    if host.kind == "none":
        return torch.empty(0, dtype=torch.int64)
    wg, tid = torch.arange(host.n)[:, None, None], torch.arange(nt)[None, :, None]
    if host.kind == "granules":
        it = torch.arange(PF_BYTES_PER_WG // (nt * 16))[None, None, :]
        off = wg * PF_BYTES_PER_WG + tid * 16 + it * nt * 16
    else:
        it = torch.arange(cdiv(host.per_wg, nt * 16))[None, None, :]
        off = wg * host.per_wg + tid * 16 + it * nt * 16
        off = off[off < (wg + 1) * host.per_wg]
    off = off.reshape(-1)
    return off[off + 16 <= nbytes].sort().values


# ================================================================== f5e_flash_attn_pf, restated

Attn = namedtuple("Attn", "kernel threads hosts grid ktiles")     # kernel: "<1>", "<2>", "b1", "<4>" or "lds"


def attn_pick(S, H, N, splits=0, cus=256):
    """Which kernel f5e_flash_attn_pf launches and whether it appends prefetch workgroups when given a hint."""
    grid, ktiles = cdiv(N, 32) * H * S, cdiv(N, 64)
    if splits == -1 or (splits == 0 and grid >= 8192):
        return Attn("lds", 256, False, grid, ktiles)
    if splits <= 0:
        splits = 1 if grid > 2 * cus else 4
        while splits > 1 and splits > ktiles:
            splits >>= 1
    assert splits in (1, 2, 4)
    kernel = {1: "<1>", 2: "<2>", 4: "b1" if ktiles <= 8 else "<4>"}[splits]
    return Attn(kernel, 64 * splits, True, grid, ktiles)


# ================================================================== one evaluation: who hosts what (scheme 0)

Launch = namedtuple("Launch", "op block inst n_main weight nbytes host")


def chain_hosting(S, N, D, H, FF, L, mel=100, cus=256):
    """The hosting launches of one fused-AdaLN evaluation with mall_prefetch on, in launch order (FF1 included: it hosts
    nothing).  ``inst`` is the GEMM instantiation or the Attn pick."""
    M, inner = S * N, H * 64
    b_out, b_ff, b_qkv, b_proj = D * inner * 2, FF * D * 2, 3 * inner * D * 2, mel * D * 2
    out = []

    def gemm(op, l, epi, n, k, fuse, weight, nbytes):
        p = R.path(epi, M, n, k, 0, 1, fuse, False, cus)
        host = gemm_hosting(p.inst, p.n_tiles, nbytes, cus) if nbytes else NONE
        out.append(Launch(op, l, p.inst, p.n_tiles, weight, nbytes, host))

    for l in range(L):
        gemm("qkv", l, "qkv", 3 * inner, D, 1, "w_out", b_out)
        a = attn_pick(S, H, N, 0, cus)
        out.append(Launch("attn", l, a, a.grid, "w_ff1", b_ff, Host("granules", prefetch_wgs(b_ff), 0) if a.hosts else NONE))
        gemm("out", l, "gate", D, inner, 2, "w_ff2", b_ff)
        gemm("ff1", l, "gelu", FF, D, 1, None, 0)
        last = l + 1 == L
        gemm("ff2", l, "gate", D, FF, 2, "w_proj" if last else "w_qkv", b_proj if last else b_qkv)
    return out


def chain_tags(launches):
    """The hosting states of an evaluation as the names tests/test_dit_chain_cpu.py asks for."""
    tags = set()
    for x in launches:
        if x.op == "attn":
            a = x.inst
            if a.hosts:
                tags.add(f"attn {a.kernel} hosts" + (" (unsplit: grid > 2 per CU)" if a.kernel == "<1>" and a.ktiles > 1 else ""))
            continue
        if not x.nbytes:
            continue
        i = x.inst
        if i.NLOAD > 0:
            tags.add(f"role split {i.BM}-row {x.host.kind}")
        else:
            tags.add("classic FUSE hosts (n_main <= 768)" if x.host.kind != "none" else "classic FUSE hosts nothing (n_main > 768)")
        if x.weight == "w_proj" and x.host.kind != "none" and x.nbytes % PF_BYTES_PER_WG:
            tags.add("w_proj partial last granule")
    return tags


REQUIRED = (
    "attn <1> hosts", "attn <2> hosts", "attn b1 hosts", "attn <4> hosts", "attn <1> hosts (unsplit: grid > 2 per CU)",
    "role split 64-row granules", "role split 64-row packed", "role split 64-row none",
    "role split 128-row granules", "role split 128-row packed",
    "classic FUSE hosts (n_main <= 768)", "classic FUSE hosts nothing (n_main > 768)", "w_proj partial last granule",
)


# ================================================================== cases

# arch: "base" D 1024 H 16 FF 2048, "tiny" D 256 H 4 FF 512, "tiny_qn_skip" the same with qk_norm = rms_norm and the long skip
ARCH = dict(base=dict(dim=1024, heads=16), tiny=dict(dim=256, heads=4),
            tiny_qn_skip=dict(dim=256, heads=4, qk_norm="rms_norm", long_skip_connection=True))
_CASE = dict(B=1, lens=None, fused=True, per_item=False, expect=())
Case = namedtuple("Case", ("arch", "L", "S", "N") + tuple(_CASE), defaults=tuple(_CASE.values()))


def cid(c):
    s = f"{c.arch}-L{c.L}-S{c.S}B{c.B}-N{c.N}-" + ("fused" if c.fused else "plain")
    return s + ("-masked" if c.lens else "") + ("-per_item" if c.per_item else "")


def dims(c):
    a = ARCH[c.arch]
    return a["dim"], a["heads"], 2 * a["dim"]


def case_tags(c, cus=256):
    D, H, FF = dims(c)
    return chain_tags(chain_hosting(c.S, c.N, D, H, FF, c.L, 100, cus)) if c.fused else set()


CASES = (
    # the shapes of the table in the module docstring of tests/test_dit_chain_gpu.py; depth 1 and 3 alternate
    Case("base", 3, 1, 469, expect=("role split 64-row granules", "role split 64-row packed", "attn b1 hosts",
                                    "w_proj partial last granule")),
    Case("base", 1, 2, 469, lens=(469, 405), expect=("role split 64-row packed", "attn b1 hosts", "w_proj partial last granule")),
    Case("base", 1, 2, 512, B=2, lens=(448, 512), expect=("role split 64-row none", "attn b1 hosts")),
    Case("base", 3, 2, 530, lens=(530, 466), expect=("role split 128-row granules", "role split 128-row packed",
                                                     "attn <1> hosts (unsplit: grid > 2 per CU)")),
    Case("base", 1, 1, 530, expect=("attn <4> hosts", "role split 64-row granules")),
    Case("base", 1, 2, 130, B=2, lens=(130, 66), expect=("attn <2> hosts", "role split 64-row granules")),
    Case("base", 3, 2, 33, expect=("attn <1> hosts", "role split 64-row granules", "w_proj partial last granule")),
    Case("base", 1, 3, 704, lens=(704, 640, 704), expect=("classic FUSE hosts (n_main <= 768)",
                                                          "classic FUSE hosts nothing (n_main > 768)",
                                                          "attn <1> hosts (unsplit: grid > 2 per CU)")),
    # the cheapest shapes
    Case("tiny", 2, 2, 33, expect=("attn <1> hosts", "role split 64-row granules")),
    Case("tiny", 2, 1, 96, expect=("attn <2> hosts", "role split 64-row granules")),
    # separate LayerNorms: per-item times (mod_rows = B), qk_norm and the long skip connection
    Case("base", 1, 2, 130, B=2, lens=(130, 66), fused=False, per_item=True),
    Case("tiny", 2, 2, 96, B=2, fused=False, per_item=True),
    Case("tiny_qn_skip", 2, 2, 96, B=2, lens=(96, 32), fused=False, per_item=True),
    Case("tiny_qn_skip", 2, 1, 33, fused=False),
)


# ================================================================== device side: inputs, arenas, the assembly

def ws_shapes(c_plan):
    """name -> (dtype, shape) of every workspace buffer of f5e_workspace_bytes."""
    p = c_plan
    M, D, inner = p.S * p.N, p.D, p.H * 64
    qk = (p.S, p.H, p.n_pad, 64)
    return dict(h0=(F32, (M, D)), h0_bf16=(BF, (M, D)), c1=(BF, (M, D)), x=(F32, (M, D)), hn=(BF, (M, D)), q=(BF, qk), k=(BF, qk),
                vt=(BF, (p.S, p.H, 64, p.n_pad)), ao=(BF, (M, inner)), ff=(BF, (M, p.FF)), pred=(F32, (M, p.mel)),
                ln_stats=(F32, (M, D // 64, 2)), skip_res=(F32, (M, D)), skip_tmp=(F32, (M, D)), ln_rowmean=(F32, (M,)))


class Chain:
    """One case on the device: the engine's real tables for three evaluation times, seeded y and in_const, eval_ptr."""

    def __init__(self, c, eng, names):
        self.c, self.eng, self.names = c, eng, names
        S, B, N, D = c.S, c.B, c.N, eng.cfg.dim
        gen = torch.Generator().manual_seed(4000 + 7 * S + N)
        self.y = torch.randn(B * N, eng.cfg.mel_dim, generator=gen).cuda()
        self.in_const = (0.5 * torch.randn(S * N, D, generator=gen)).cuda()
        t = torch.tensor([0.11, 0.47, 0.83])
        if c.per_item:
            t = t[:, None] + 0.05 * torch.arange(B)[None, :]
        self.mod = eng.time_tables(t.cuda())                                  # [3, mod_rows, row_stride]
        self.cd = eng.cd_tables(self.mod) if c.fused else None                # [3, 1, cd_stride]
        self.rope = eng.rope_table(N)
        self.seq_len = torch.tensor(c.lens, dtype=I32).cuda() if c.lens else None
        self.eval_ptr = torch.zeros(1, dtype=I32).cuda()
        torch.cuda.synchronize()

    def inputs(self):
        """Every tensor an evaluation only reads, except eval_ptr (which the test itself sets between evaluations)."""
        eng = self.eng
        ts = [self.y, self.in_const, self.mod, self.rope, eng.in_w, eng.proj_w, eng.proj_b]
        ts += [t for t in (self.cd, self.seq_len, eng.skip_w) if t is not None]
        ts += [t for pair in eng.cp for t in pair] + [t for keep in eng.blocks_keep for t in keep]
        return ts

    def new_arena(self):
        """(buffer, plan): the arena of eng.workspace_layout with SPARE bytes on both sides, sentinel-filled, q / k / vt zeroed."""
        c, eng = self.c, self.eng
        layout = eng.workspace_layout(eng.plan_shape(c.S, c.B, c.N, self.mod.shape[1], c.fused))
        total = int(layout.total)
        buf = torch.empty(total + 2 * SPARE, dtype=U8, device="cuda")
        buf.view(F32).fill_(SENTINEL)
        arena = buf[SPARE:SPARE + total]
        plan = eng.make_plan(c.S, c.B, c.N, self.y, self.in_const, self.mod, self.eval_ptr, self.rope, self.seq_len, cd=self.cd,
                             arena=arena)
        assert bool(plan.c.fuse_ln) == c.fused and arena.data_ptr() == buf.data_ptr() + SPARE
        eng.zero_pads(plan.layout, arena)
        return buf, plan

    def used(self, plan):
        """[(name, begin, end)] byte ranges inside the buffer (SPARE included) of the buffers the plan uses."""
        w = plan.layout
        return [(n, SPARE + int(w.offset[i]), SPARE + int(w.offset[i] + w.bytes[i])) for i, n in enumerate(self.names) if w.bytes[i]]

    def views(self, buf, plan):
        sh = ws_shapes(plan.c)
        return {n: buf[a:b].view(sh[n][0]).view(sh[n][1]) for n, a, b in self.used(plan)}


def assemble(ops, ch, v):
    """One evaluation through the public entry points, into the buffers ``v`` of a twin arena (see the module docstring)."""
    c, eng = ch.c, ch.eng
    S, B, N = c.S, c.B, c.N
    D, H, L, FF, mel, inner = eng.cfg.dim, eng.cfg.heads, eng.L, eng.FF, eng.cfg.mel_dim, eng.inner
    M, rs, mod_rows = S * N, eng.row_stride, ch.mod.shape[1]
    ev, es = ch.eval_ptr, mod_rows * rs
    mflat = ch.mod.view(-1)
    modv = lambda off: mflat.as_strided((mod_rows, D), (rs, 1), off)                  # noqa: E731  evaluation 0's rows
    ops.gemm_f32(ch.y, eng.in_w, None, out=v["h0"], out_bf16=v["h0_bf16"], M=M, addend=ch.in_const, K=mel)
    ops.convpos(v["h0_bf16"], eng.cp[0][0], eng.cp[0][1], S, N, out_bf16=v["c1"])
    ops.convpos(v["c1"], eng.cp[1][0], eng.cp[1][1], S, N, out_f32=v["x"], resid=v["h0"])
    x, hn, q, k, vt, ao, ff = (v[n] for n in ("x", "hn", "q", "k", "vt", "ao", "ff"))
    if eng.skip_w is not None:
        v["skip_res"].copy_(x)
    if c.fused:
        stats, rowmean, cds = v["ln_stats"], v["ln_rowmean"], ch.cd.shape[2]
        cflat, ls = ch.cd.view(-1), 6 * inner + 2 * FF
        cdv = lambda off, n: cflat.as_strided((1, n), (cds, 1), off)                  # noqa: E731
        cons = lambda off, n: ops.ln_consumer(stats, cdv(off, n), cdv(off + n, n), N, rowmean, ev, cds)    # noqa: E731
        prod = lambda off: ops.ln_producer(hn, modv(off), stats, rowmean)             # noqa: E731
        ops.adaln_pre(x, hn, modv(D), stats, rowmean, N, ev, es)
        for l in range(L):
            w_qkv, _, w_out, b_out, w_ff1, _, w_ff2, b_ff2 = eng.blocks_keep[l][:8]
            mb = l * 6 * D
            ops.gemm_bf16_qkv_rope(hn, w_qkv, None, q, k, vt, H, eng.rope_heads, ch.rope, N, ln=cons(l * ls, 3 * inner))
            ops.flash_attn(q, k, vt, ao, N, kv_len=ch.seq_len, waves=0)
            ops.gemm_bf16_gate_residual(ao, w_out, b_out, x, modv(mb + 2 * D), N, ch.seq_len, ev, es, ln=prod(mb + 4 * D))
            ops.gemm_bf16_bias(hn, w_ff1, None, ff, act=ops.ACT_GELU_TANH, ln=cons(l * ls + 6 * inner, FF))
            nxt = mb + 6 * D + D if l + 1 < L else L * 6 * D
            ops.gemm_bf16_gate_residual(ff, w_ff2, b_ff2, x, modv(mb + 5 * D), N, None, ev, es, ln=prod(nxt))
        ops.gemm_bf16_bias(hn, eng.proj_w, None, v["pred"], ln=cons(L * ls, mel))
        return
    norm = lambda scale, shift: ops.layernorm(x, hn, scale=modv(scale), shift=modv(shift), rows_per_seq=N, eval_ptr=ev,    # noqa: E731
                                              eval_stride=es)
    for l in range(L):
        keep = eng.blocks_keep[l]
        w_qkv, b_qkv, w_out, b_out, w_ff1, b_ff1, w_ff2, b_ff2 = keep[:8]
        qn, kn = (keep[8], keep[9]) if len(keep) > 8 else (None, None)
        mb = l * 6 * D
        norm(mb + D, mb)
        ops.gemm_bf16_qkv_rope(hn, w_qkv, b_qkv, q, k, vt, H, eng.rope_heads, ch.rope, N, q_norm_w=qn, k_norm_w=kn)
        ops.flash_attn(q, k, vt, ao, N, kv_len=ch.seq_len, waves=0)
        ops.gemm_bf16_gate_residual(ao, w_out, b_out, x, modv(mb + 2 * D), N, ch.seq_len, ev, es)
        norm(mb + 4 * D, mb + 3 * D)
        ops.gemm_bf16_bias(hn, w_ff1, b_ff1, ff, act=ops.ACT_GELU_TANH)
        ops.gemm_bf16_gate_residual(ff, w_ff2, b_ff2, x, modv(mb + 5 * D), N, None, ev, es)
    if eng.skip_w is not None:
        ops.gemm_f32(x, eng.skip_w, None, out=v["skip_tmp"], K=D)
        ops.gemm_f32(v["skip_res"], eng.skip_w[:, D:], None, out=x, addend=v["skip_tmp"], K=D)
    norm(L * 6 * D, L * 6 * D + D)
    ops.gemm_bf16_bias(hn, eng.proj_w, eng.proj_b, v["pred"])
