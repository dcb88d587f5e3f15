"""The tiny Qwen2 of tests/golden/qwen2.npz on the GPU (infer/qwen2.py) against the ``transformers`` fixture: prefill logits at the
project's 2e-4 relative-L2 gate for fp32 models, the 16 greedy tokens of both rows (every top-2 gap of the fixture is >= 1e-2),
each row against its B = 1 run, the captured step against the eager run (greedy and sampled, bit for bit), the second turn of a
``ChatSession`` against the fixture's second-turn logits, and "f32" against "bf16" weights on the bf16-valued fixture.

Measured on an MI355X: see DESIGN.md 4s."""
import numpy as np
import pytest
import torch

import qwen2_ref as Q

pytestmark = pytest.mark.gpu

GATE = 2e-4
_m = {}


def fixture():
    if "fx" not in _m:
        _m["fx"] = Q.load_fixture()
    return _m["fx"]


def model(weights="bf16"):
    from f5e_tts_amd.infer.qwen2 import Qwen2, Qwen2Config
    if weights not in _m:
        fx, sd, cfg = fixture()
        m = Qwen2(Qwen2Config.from_dict(dict(cfg["hf"], model_type="qwen2")), weights=weights)
        _m[weights] = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return _m[weights]


def rows():
    fx = fixture()[0]
    return [fx["ids"][0].tolist(), fx["ids"][1, 4:].tolist()]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


GREEDY = dict(do_sample=False, repetition_penalty=1.05, eos_token_id=[])


def test_prefill_logits_and_greedy_tokens_match_transformers():
    fx = fixture()[0]
    st = {}
    toks, n = model().generate(rows(), 16, pad_token_id=int(fx["pad"]), stats=st, **GREEDY)
    e = rel(st["prefill_logits"].cpu().numpy(), fx["logits"])
    print(f"qwen2 prefill logits vs transformers: rel L2 {e:.3e} (gate {GATE:.0e})")
    assert e <= GATE
    assert np.array_equal(toks.cpu().numpy(), fx["tokens"]) and n == [16, 16]


def test_each_row_equals_its_own_run_and_weight_types_agree():
    fx = fixture()[0]
    both, _ = model().generate(rows(), 16, **GREEDY)
    for r, row in enumerate(rows()):
        one, _ = model().generate([row], 16, **GREEDY)
        assert torch.equal(one[0], both[r])
    st16, st32 = {}, {}
    a, _ = model("bf16").generate(rows(), 16, stats=st16, **GREEDY)
    b, _ = model("f32").generate(rows(), 16, stats=st32, **GREEDY)
    assert torch.equal(a, b) and torch.equal(st16["prefill_logits"], st32["prefill_logits"])
    assert model("bf16").device_bytes() < model("f32").device_bytes()


@pytest.mark.parametrize("kw", (GREEDY, dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.95, repetition_penalty=1.05, seed=1234,
                                             eos_token_id=[])))
def test_step_graph_gives_the_eager_tokens(kw):
    st = {}
    eager, n1 = model().generate(rows(), 24, **kw)
    graph, n2 = model().generate(rows(), 24, step_graph=True, stats=st, **kw)
    assert torch.equal(eager, graph) and n1 == n2
    assert st["captures"] == 1 and st["replays"] == 23
    if kw.get("do_sample"):                                      # another seed draws other tokens: the draw is live
        other, _ = model().generate(rows(), 24, **dict(kw, seed=99))
        assert not torch.equal(other, eager)


def test_eos_closes_a_row_and_pads_behind_it():
    fx = fixture()[0]
    eos = int(fx["tokens"][0, 5])
    first = fx["tokens"][0].tolist().index(eos)
    toks, n = model().generate(rows()[:1], 16, do_sample=False, repetition_penalty=1.05, eos_token_id=[eos, 383], pad_token_id=7)
    assert n == [first + 1] and toks[0, :first + 1].tolist() == fx["tokens"][0, :first + 1].tolist()
    assert (toks[0, first + 1:] == 7).all()


def test_chat_session_second_turn_matches_transformers():
    from f5e_tts_amd.infer.qwen2 import ChatSession
    fx = fixture()[0]
    for graph in (False, True):
        s = ChatSession(model(), positions=64)
        out = s.turn_ids(rows()[0], 16, step_graph=graph, **GREEDY)
        assert out == fx["tokens"][0].tolist()
        s.turn_ids(fx["turn2_ids"].tolist(), 4, step_graph=graph, **GREEDY)
        e = rel(s.last_logits[0].cpu().numpy(), fx["turn2_logits"])
        print(f"qwen2 second-turn logits vs transformers (step_graph={graph}): rel L2 {e:.3e} (gate {GATE:.0e})")
        assert e <= GATE
        assert s.prefilled == [9, 7]                              # the turn's 6 ids behind the one token that was never fed
        s.clear()
        assert s.turn_ids(rows()[0], 16, **GREEDY) == fx["tokens"][0].tolist()


def test_generate_refusals():
    from f5e_tts_amd._C import F5EError
    with pytest.raises(F5EError, match="4096-position cap"):
        model().generate([[1, 2, 3]], 4094, **GREEDY)
    with pytest.raises(F5EError, match="top_k"):
        model().generate([[1, 2, 3]], 4, do_sample=True, top_k=65)
    with pytest.raises(F5EError, match="step_graph"):
        model().generate([[1, 2, 3]], 4, step_graph=1)


# ---- full-size shapes: one layer + lm_head of Qwen2.5-3B, one decode step at p = 300 -------------------------------------------------

def test_full_size_layer_and_lm_head_decode_step_against_float64():
    """D 2048 / I 11008 / 16-2-128 / V 151936, seeded bf16 weights (tools/synth.py), R = 1.  Every launch of the step is held
    against float64 on ITS OWN device input under its kernel's bound, 10 sqrt(K) 2^-24 relative L2 (K = D for the norms and the
    GEMMs over D, H dk for o_proj, I for down_proj, dk for the attention, 1 for SwiGLU); the pick must be the arg max of the
    penalised device logits exactly; and ``Qwen2._step`` on the same state gives the chain's bits."""
    import math
    from types import SimpleNamespace

    from f5e_tts_amd import ops
    from f5e_tts_amd.infer.qwen2 import Qwen2, Qwen2Config
    from tools import synth as SY
    F64 = torch.float64
    fields = SY.qwen2_config_fields(num_hidden_layers=1)
    m = Qwen2(Qwen2Config.from_dict(fields), "bf16").load_state_dict(SY.init_qwen2_state(fields, 77, "cuda"))
    cfg, L = m.cfg, m.layers[0]
    H, Hkv, dk, D, I, V = 16, 2, 128, 2048, 11008, 151936
    p, P = 300, 512
    g = torch.Generator(device="cuda").manual_seed(5)

    def fresh():
        S = m.new_state(1, P)
        gg = torch.Generator(device="cuda").manual_seed(5)
        S.kc[0][:, :p].normal_(generator=gg)
        S.vc[0][:, :p].normal_(generator=gg)
        S.tokens.random_(0, V, generator=gg)
        S.last.copy_(S.tokens[:, p])
        S.rec.copy_(ops.whisper_step_record(p, 1, 0))
        return S
    del g
    S = fresh()
    kc0, vc0 = S.kc[0].clone(), S.vc[0].clone()
    sm = SimpleNamespace(do_sample=False, temperature=1.0, top_k=1, top_p=1.0, penalty=1.05)
    bound = lambda K: 10.0 * math.sqrt(K) * 2.0 ** -24                       # noqa: E731
    rel = lambda a, b: float((a.to(F64) - b).norm() / b.norm())              # noqa: E731
    report = []

    def hold(name, got, want, K):
        e = rel(got, want)
        report.append(f"{name} {e:.2e}/{bound(K):.2e}")
        assert e <= bound(K), (name, e, bound(K))

    def rms(x, w):
        x = x.to(F64)
        return x / torch.sqrt((x * x).mean(-1, keepdim=True) + cfg.rms_norm_eps) * w.to(F64)
    buf = lambda *s: torch.empty(*s, device="cuda")                           # noqa: E731
    x, xn, qkv, ao, gu, ff, logits = buf(1, D), buf(1, D), buf(1, (H + 2 * Hkv) * dk), buf(1, H * dk), buf(1, 2 * I), buf(1, I), buf(1, V)
    gemm = lambda a, w, b=None, **kw: m._gemm_step(S, a, w, b, **kw)         # noqa: E731
    ops.llm_embed(S.last, m.embed, x)
    assert torch.equal(x[0], m.embed[int(S.last[0])].float())
    ops.rmsnorm_f32(x, L.ln1, cfg.rms_norm_eps, out=xn)
    hold("rmsnorm", xn, rms(x, L.ln1), D)
    gemm(xn, L.wqkv, L.bqkv, out=qkv)
    hold("qkv", qkv, xn.to(F64) @ L.wqkv.to(F64).T + L.bqkv.to(F64), D)
    ops.gqa_rope_decode_dev_f32(qkv, S.kc[0], S.vc[0], m.cos, m.sin, S.rec, H, Hkv, dk ** -0.5, begin=S.begin, out=ao)
    cos, sin = m.cos[p].to(F64), m.sin[p].to(F64)

    def rot(t):                                                               # [heads, dk] at position p
        a, b = t[:, :dk // 2], t[:, dk // 2:]
        return torch.cat([a * cos - b * sin, b * cos + a * sin], 1)
    q64 = rot(qkv[0, :H * dk].to(F64).view(H, dk))
    k_new = rot(qkv[0, H * dk:(H + Hkv) * dk].to(F64).view(Hkv, dk))
    K = torch.cat([kc0[0, :p].to(F64).view(p, Hkv, dk), k_new[None]], 0)
    Vv = torch.cat([vc0[0, :p].to(F64).view(p, Hkv, dk), qkv[0, (H + Hkv) * dk:].to(F64).view(1, Hkv, dk)], 0)
    want = torch.stack([torch.softmax(K[:, h // 8] @ q64[h] * dk ** -0.5, 0) @ Vv[:, h // 8] for h in range(H)]).view(1, H * dk)
    hold("attention", ao, want, dk)
    hold("filed key", S.kc[0][0, p].view(Hkv, dk), k_new, 1)
    assert torch.equal(S.vc[0][0, p], qkv[0, (H + Hkv) * dk:]) and torch.equal(S.kc[0][:, :p], kc0[:, :p])
    x0 = x.clone()
    gemm(ao, L.wo, None, out=x, addend=x)
    hold("o_proj", x, x0.to(F64) + ao.to(F64) @ L.wo.to(F64).T, H * dk)
    ops.rmsnorm_f32(x, L.ln2, cfg.rms_norm_eps, out=xn)
    hold("rmsnorm 2", xn, rms(x, L.ln2), D)
    gemm(xn, L.wgu, None, out=gu)
    hold("gate|up", gu, xn.to(F64) @ L.wgu.to(F64).T, D)
    ops.swiglu_f32(gu, out=ff)
    g64 = gu.to(F64)
    hold("swiglu", ff, g64[:, :I] / (1.0 + torch.exp(-g64[:, :I])) * g64[:, I:], 1)
    x1 = x.clone()
    gemm(ff, L.wdown, None, out=x, addend=x)
    hold("down_proj", x, x1.to(F64) + ff.to(F64) @ L.wdown.to(F64).T, I)
    ops.rmsnorm_f32(x, m.norm, cfg.rms_norm_eps, out=xn)
    hold("final norm", xn, rms(x, m.norm), D)
    gemm(xn, m.lm_head, None, out=logits)
    hold("lm_head", logits, xn.to(F64) @ m.lm_head.to(F64).T, D)
    m._pick(S, logits, sm, [], 0)
    seen = torch.unique(S.tokens[0, :p + 1].long())
    y = logits[0].clone()
    y[seen] = torch.where(y[seen] < 0, y[seen] * torch.tensor(1.05, device="cuda"), y[seen] / torch.tensor(1.05, device="cuda"))
    assert int(S.tokens[0, p + 1]) == int(torch.nonzero(y == y.max())[0]) and int(S.rec[0]) == p + 1
    print("full-size step, rel L2 / bound: " + ", ".join(report))
    S2 = fresh()                                                              # the model's own step: the chain's bits
    m._step(S2, sm, [], 0)
    from f5e_tts_amd.xfmr_f32 import view
    assert torch.equal(view(S2.ws, S2.plan, "logits"), logits) and torch.equal(S2.tokens, S.tokens)
    assert torch.equal(S2.kc[0], S.kc[0]) and torch.equal(S2.vc[0], S.vc[0])
