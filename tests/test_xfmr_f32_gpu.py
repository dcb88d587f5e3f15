"""``xfmr_f32.layer`` pins the launch order of its six users: each user's sequence is written out here as plain ``ops.*`` calls
(what the models issued before they shared the layer), and ``layer`` on a copy of the same buffers must leave every written
buffer bit-equal -- x / the layer stack, xn, qkv, ao, q, ff, the key / value caches, the memory's k | v and the alignment slice.

Smallest shapes that reach every branch: D = 64, H = 4 (head dim 16), FF = 128; encoders B = 2, T = 37, kv_len = [37, 21];
steps R = 6 (B = 2 x 3 rows), Umax = 8, p = 0 .. 3 with a non-identity ancestry table from p = 2, Tk = 50, mem_len = [50, 33]."""
import pytest
import torch

pytestmark = pytest.mark.gpu

D, H, FF, B, T, R, UMAX, TK = 64, 4, 128, 2, 37, 6, 8, 50
SCALE = (D // H) ** -0.5
EPS = 1e-5


def weights(seed, cross=False, extra=False):
    from f5e_tts_amd.xfmr_f32 import LayerWeights
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, k=0.1: (k * torch.randn(*s, generator=g)).cuda()   # noqa: E731
    ln = lambda: (1 + r(D), r(D))   # noqa: E731
    x = dict(ln_x=ln(), xq=(r(D, D), r(D)), xkv=(r(2 * D, D), r(2 * D)), xout=(r(D, D), r(D))) if cross else \
        dict(ln_x=None, xq=None, xkv=None, xout=None)
    return LayerWeights(ln1=ln(), qkv=(r(3 * D, D), r(3 * D)), out=(r(D, D), r(D)), ln_ff=ln(), ff=(r(FF, D), r(FF), r(D, FF), r(D)),
                        extra=(r(8, D // H, k=0.3), r(8), 1 + r(H)) if extra else None, **x)


def buffers(M, seed, **more):
    """The scratch filled with noise (a launch that is skipped or misdirected shows) plus the case's own tensors."""
    g = torch.Generator().manual_seed(seed)
    b = {n: torch.randn(M, w, generator=g).cuda() for n, w in (("x", D), ("xn", D), ("qkv", 3 * D), ("ao", D), ("q", D), ("ff", FF))}
    b.update(more)
    return b


def same(a, b):
    assert a.keys() == b.keys()
    for n in a:
        assert torch.equal(a[n], b[n]), n


def clone(b):
    return {n: t.clone() for n, t in b.items()}


def bufs_of(b):
    return b["xn"], b["qkv"], b["ao"], b["q"], b["ff"]


def qkv3(qkv):
    return qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]


def i32(v):
    return torch.tensor(v, dtype=torch.int32).cuda()


# ---- the encoders --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["ACT_GELU_ERF", "ACT_RELU"])
def test_post_norm_encoder_layer_wav2vec2(act):
    from f5e_tts_amd import ops
    from f5e_tts_amd.xfmr_f32 import layer
    act, frames = getattr(ops, act), i32([37, 21])
    Ws, a = [weights(1), weights(2)], buffers(B * T, 3)
    b = clone(a)
    x, qkv, ao, ff = a["x"], a["qkv"], a["ao"], a["ff"]
    for W in Ws:
        ops.gemm_f32(x, W.qkv[0], W.qkv[1], out=qkv)
        ops.mha_f32(*qkv3(qkv), H, SCALE, B=B, kv_len=frames, out=ao)
        ops.gemm_f32(ao, W.out[0], W.out[1], out=x, addend=x)
        ops.layernorm(x, x, W.ln1[0], W.ln1[1], eps=EPS)
        ops.gemm_f32(x, W.ff[0], W.ff[1], out=ff, act=act)
        ops.gemm_f32(ff, W.ff[2], W.ff[3], out=x, addend=x)
        ops.layernorm(x, x, W.ln_ff[0], W.ln_ff[1], eps=EPS)

    def self_attn(_W, _x, qkv, ao):
        ops.mha_f32(*qkv3(qkv), H, SCALE, B=B, kv_len=frames, out=ao)
    for W in Ws:
        layer(b["x"], b["x"], W, bufs_of(b), pre_norm=False, act=act, eps=EPS, self_attn=self_attn)
    same(a, b)


def test_pre_norm_layer_stack_wavlm():
    """A 3-deep stack: layer l reads out[l] and writes out[l + 1], twice; the gate reads the normed input and ``W.extra``."""
    from f5e_tts_amd import ops
    from f5e_tts_amd.xfmr_f32 import layer
    g = torch.Generator().manual_seed(4)
    frames, table = i32([37, 21]), torch.randn(H, 2 * T - 1, generator=g).cuda()
    Ws, M = [weights(5, extra=True), weights(6, extra=True)], B * T
    a = buffers(M, 7, out=torch.randn(3, M, D, generator=g).cuda(), gate=torch.randn(B, H, T, generator=g).cuda())
    b = clone(a)
    xn, qkv, ao, ff, gate = a["xn"], a["qkv"], a["ao"], a["ff"], a["gate"]
    for l, W in enumerate(Ws):
        x, y = a["out"][l], a["out"][l + 1]
        ops.layernorm(x, xn, W.ln1[0], W.ln1[1], eps=EPS)
        ops.gemm_f32(xn, W.qkv[0], W.qkv[1], out=qkv)
        ops.wavlm_gate(xn, W.extra[0], W.extra[1], W.extra[2], gate)
        ops.relbias_attn(*qkv3(qkv), gate, table, H, SCALE, kv_len=frames, out=ao)
        ops.gemm_f32(ao, W.out[0], W.out[1], out=y, addend=x)
        ops.layernorm(y, xn, W.ln_ff[0], W.ln_ff[1], eps=EPS)
        ops.gemm_f32(xn, W.ff[0], W.ff[1], out=ff, act=ops.ACT_GELU_ERF)
        ops.gemm_f32(ff, W.ff[2], W.ff[3], out=y, addend=y)

    def self_attn(W, xn, qkv, ao):
        ops.wavlm_gate(xn, *W.extra, b["gate"])
        ops.relbias_attn(*qkv3(qkv), b["gate"], table, H, SCALE, kv_len=frames, out=ao)
    for l, W in enumerate(Ws):
        layer(b["out"][l], b["out"][l + 1], W, bufs_of(b), pre_norm=True, act=ops.ACT_GELU_ERF, eps=EPS, self_attn=self_attn)
    same(a, b)


def test_pre_norm_encoder_layer_whisper():
    from f5e_tts_amd import ops
    from f5e_tts_amd.xfmr_f32 import layer
    Ws, a = [weights(8), weights(9)], buffers(B * T, 10)
    b = clone(a)
    x, xn, qkv, ao, ff = a["x"], a["xn"], a["qkv"], a["ao"], a["ff"]
    for W in Ws:
        ops.layernorm(x, xn, *W.ln1, eps=1e-5)
        ops.gemm_f32(xn, W.qkv[0], W.qkv[1], out=qkv)
        ops.mha_f32(*qkv3(qkv), H, SCALE, B=B, out=ao)
        ops.gemm_f32(ao, W.out[0], W.out[1], out=x, addend=x)
        ops.layernorm(x, xn, *W.ln_ff, eps=1e-5)
        ops.gemm_f32(xn, W.ff[0], W.ff[1], out=ff, act=ops.ACT_GELU_ERF)
        ops.gemm_f32(ff, W.ff[2], W.ff[3], out=x, addend=x)

    def self_attn(_W, _xn, qkv, ao):
        ops.mha_f32(*qkv3(qkv), H, SCALE, B=B, out=ao)
    for W in Ws:
        layer(b["x"], b["x"], W, bufs_of(b), pre_norm=True, act=ops.ACT_GELU_ERF, eps=1e-5, self_attn=self_attn)
    same(a, b)


# ---- the decoders --------------------------------------------------------------------------------------------------------------
def test_teacher_forced_decoder_layer_wenet():
    """``decode``: causal self-attention over B * n_hyp items of U1 rows, the memory's k | v projected per layer."""
    from f5e_tts_amd import ops
    from f5e_tts_amd.xfmr_f32 import layer
    g = torch.Generator().manual_seed(11)
    n_hyp, U1 = 3, 5
    NB = B * n_hyp
    ys_len, mem_len, mem = i32([5, 1, 3, 4, 2, 5]), i32([50, 33]), torch.randn(B * TK, D, generator=g).cuda()
    Ws = [weights(12, cross=True), weights(13, cross=True)]
    a = buffers(NB * U1, 14, kv=torch.randn(B * TK, 2 * D, generator=g).cuda())
    b = clone(a)
    x, hn, qkv, ctx, q, mid, kv = (a[n] for n in ("x", "xn", "qkv", "ao", "q", "ff", "kv"))
    for L in Ws:
        ops.layernorm(x, hn, gamma=L.ln1[0], beta=L.ln1[1], eps=1e-5)
        ops.gemm_f32(hn, *L.qkv, out=qkv)
        ops.mha_f32(*qkv3(qkv), H, SCALE, B=NB, kv_len=ys_len, causal=True, out=ctx)
        ops.gemm_f32(ctx, *L.out, out=x, addend=x)
        ops.layernorm(x, hn, gamma=L.ln_x[0], beta=L.ln_x[1], eps=1e-5)
        ops.gemm_f32(hn, *L.xq, out=q)
        ops.gemm_f32(mem, *L.xkv, out=kv)
        ops.mha_f32(q, kv[:, :D], kv[:, D:], H, SCALE, B=B, kv_len=mem_len, causal=False, out=ctx)
        ops.gemm_f32(ctx, *L.xout, out=x, addend=x)
        ops.layernorm(x, hn, gamma=L.ln_ff[0], beta=L.ln_ff[1], eps=1e-5)
        ops.gemm_f32(hn, L.ff[0], L.ff[1], out=mid, act=ops.ACT_RELU)
        ops.gemm_f32(mid, L.ff[2], L.ff[3], out=x, addend=x)

    def self_attn(_L, _hn, qkv, ctx):
        ops.mha_f32(*qkv3(qkv), H, SCALE, B=NB, kv_len=ys_len, causal=True, out=ctx)

    def src_attn(L, q, ctx):
        ops.gemm_f32(mem, *L.xkv, out=b["kv"])
        ops.mha_f32(q, b["kv"][:, :D], b["kv"][:, D:], H, SCALE, B=B, kv_len=mem_len, causal=False, out=ctx)
    for L in Ws:
        layer(b["x"], b["x"], L, bufs_of(b), pre_norm=True, act=ops.ACT_RELU, eps=1e-5, self_attn=self_attn, cross_attn=src_attn)
    same(a, b)


def ancestry():
    """i32 [R, Umax]: identity, then from p = 2 rows swap inside their utterance (rows 0-2 and 3-5)."""
    anc = torch.arange(R, dtype=torch.int32)[:, None].repeat(1, UMAX)
    anc[:, 0] = torch.tensor([1, 0, 0, 4, 5, 3])
    anc[:, 1] = torch.tensor([2, 2, 0, 3, 3, 4])
    return anc.cuda()


def step_case(seed):
    g = torch.Generator().manual_seed(seed)
    Ws = [weights(seed + 1, cross=True), weights(seed + 2, cross=True)]
    rnd = lambda *s: torch.randn(*s, generator=g).cuda()   # noqa: E731
    xs = rnd(4, R, D)                                                  # the embedded token of steps p = 0 .. 3
    return Ws, xs, rnd(2, R, UMAX, D), rnd(2, R, UMAX, D), [rnd(B * TK, 2 * D) for _ in Ws]


@pytest.mark.parametrize("every", [False, True])
def test_cached_step_wenet(every):
    """``decode_step``: the ancestry table on layer 0 alone (the default) or on every layer (``reorder_cache``)."""
    from f5e_tts_amd import ops
    from f5e_tts_amd.xfmr_f32 import layer
    Ws, xs, kc, vc, kvs = step_case(20)
    mem_len, anc = i32([50, 33]), ancestry()
    a = buffers(R, 21, kc=kc, vc=vc)
    b = clone(a)
    x, hn, qkv, ctx, q, mid = (a[n] for n in ("x", "xn", "qkv", "ao", "q", "ff"))
    at = dict(i=0, p=0, anc=None)

    def self_attn(_L, _hn, qkv, ctx):
        i = at["i"]
        ops.attn_decode_f32(qkv, b["kc"][i], b["vc"][i], at["p"], H, SCALE, anc=at["anc"] if (i == 0 or every) else None, out=ctx)

    def src_attn(_L, q, ctx):
        kv = kvs[at["i"]]
        ops.mha_f32(q, kv[:, :D], kv[:, D:], H, SCALE, B=B, kv_len=mem_len, causal=False, out=ctx)
    bufs = bufs_of(b)
    for p in range(4):
        use = anc if p >= 2 else torch.arange(R, dtype=torch.int32)[:, None].repeat(1, UMAX).cuda()
        x.copy_(xs[p])
        for i, L in enumerate(Ws):
            ops.layernorm(x, hn, gamma=L.ln1[0], beta=L.ln1[1], eps=1e-5)
            ops.gemm_f32(hn, *L.qkv, out=qkv)
            ops.attn_decode_f32(qkv, a["kc"][i], a["vc"][i], p, H, SCALE, anc=use if (i == 0 or every) else None, out=ctx)
            ops.gemm_f32(ctx, *L.out, out=x, addend=x)
            ops.layernorm(x, hn, gamma=L.ln_x[0], beta=L.ln_x[1], eps=1e-5)
            ops.gemm_f32(hn, *L.xq, out=q)
            ops.mha_f32(q, kvs[i][:, :D], kvs[i][:, D:], H, SCALE, B=B, kv_len=mem_len, causal=False, out=ctx)
            ops.gemm_f32(ctx, *L.xout, out=x, addend=x)
            ops.layernorm(x, hn, gamma=L.ln_ff[0], beta=L.ln_ff[1], eps=1e-5)
            ops.gemm_f32(hn, L.ff[0], L.ff[1], out=mid, act=ops.ACT_RELU)
            ops.gemm_f32(mid, L.ff[2], L.ff[3], out=x, addend=x)
        b["x"].copy_(xs[p])
        at["p"], at["anc"] = p, use
        for i, L in enumerate(Ws):
            at["i"] = i
            layer(b["x"], b["x"], L, bufs, pre_norm=True, act=ops.ACT_RELU, eps=1e-5, self_attn=self_attn, cross_attn=src_attn)
        same(a, b)


@pytest.mark.parametrize("beam", [False, True])
def test_cached_step_whisper(beam):
    """``_dec_step``: a row's own cache (greedy) or the ancestry table on every layer (beam); layer 1 owns one run of two
    alignment heads, written to slots 1 .. 2 of three at token position p - 1 from p = 1 on."""
    from f5e_tts_amd import ops
    from f5e_tts_amd.xfmr_f32 import layer
    Ws, xs, kc, vc, kvs = step_case(30)
    kv = [(m.view(B, TK, 2 * D)[..., :D], m.view(B, TK, 2 * D)[..., D:]) for m in kvs]
    caches = lambda t: [(t["kc"][i], t["vc"][i]) for i in range(2)]   # noqa: E731
    heads_of, m_len, anc = {1: [(1, i32([3, 1]))]}, i32([50, 33]), ancestry()
    a = buffers(R, 31, kc=kc, vc=vc, probs=torch.zeros(R, 3, 3, 52).cuda())
    b = clone(a)
    x, xn, qkv, ao, q, ff = (a[n] for n in ("x", "xn", "qkv", "ao", "q", "ff"))
    at = dict(i=0, p=0, anc=None, align=None)

    def self_attn(_W, _xn, qkv, ao):
        kc, vc = caches(b)[at["i"]]
        ops.attn_decode_f32(qkv, kc, vc, at["p"], H, SCALE, anc=at["anc"], out=ao)

    def cross_attn(_W, q, ao):
        (K, Vv), align = kv[at["i"]], at["align"]
        ops.cross_attn_decode_f32(q, K, Vv, H, SCALE, rows_per_utt=R // K.shape[0], out=ao)
        if align is not None:
            for s0, heads in heads_of.get(at["i"], ()):
                ops.cross_attn_probs_f32(q, K, heads, H, SCALE, align[0][:, s0:s0 + heads.shape[0], align[1]],
                                         rows_per_utt=R // K.shape[0], m_len=align[2])
    bufs = bufs_of(b)
    for p in range(4):
        use = None if not beam else anc if p >= 2 else torch.arange(R, dtype=torch.int32)[:, None].repeat(1, UMAX).cuda()
        align = (a["probs"], p - 1, m_len) if p >= 1 else None
        x.copy_(xs[p])
        for li, (lp, (kc_, vc_), (K, Vv)) in enumerate(zip(Ws, caches(a), kv)):
            ops.layernorm(x, xn, *lp.ln1, eps=1e-5)
            ops.gemm_f32(xn, lp.qkv[0], lp.qkv[1], out=qkv)
            ops.attn_decode_f32(qkv, kc_, vc_, p, H, SCALE, anc=use, out=ao)
            ops.gemm_f32(ao, lp.out[0], lp.out[1], out=x, addend=x)
            ops.layernorm(x, xn, *lp.ln_x, eps=1e-5)
            ops.gemm_f32(xn, lp.xq[0], lp.xq[1], out=q)
            ops.cross_attn_decode_f32(q, K, Vv, H, SCALE, rows_per_utt=R // K.shape[0], out=ao)
            if align is not None:
                for s0, heads in heads_of.get(li, ()):
                    ops.cross_attn_probs_f32(q, K, heads, H, SCALE, align[0][:, s0:s0 + heads.shape[0], align[1]],
                                             rows_per_utt=R // K.shape[0], m_len=align[2])
            ops.gemm_f32(ao, lp.xout[0], lp.xout[1], out=x, addend=x)
            ops.layernorm(x, xn, *lp.ln_ff, eps=1e-5)
            ops.gemm_f32(xn, lp.ff[0], lp.ff[1], out=ff, act=ops.ACT_GELU_ERF)
            ops.gemm_f32(ff, lp.ff[2], lp.ff[3], out=x, addend=x)
        b["x"].copy_(xs[p])
        at["p"], at["anc"], at["align"] = p, use, (b["probs"], p - 1, m_len) if p >= 1 else None
        for i, W in enumerate(Ws):
            at["i"] = i
            layer(b["x"], b["x"], W, bufs, pre_norm=True, act=ops.ACT_GELU_ERF, eps=1e-5, self_attn=self_attn, cross_attn=cross_attn)
        same(a, b)
    assert a["probs"][:, 1:].abs().sum() > 0 and not a["probs"][:, 0].any()              # the run landed in its own slots
