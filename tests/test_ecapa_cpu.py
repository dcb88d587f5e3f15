"""ECAPA-TDNN speaker encoder and SIM scoring, host side: tests/ecapa_ref.py (the CPU restatement of the forward) against
every tensor the reference's own ``ECAPA_TDNN.forward`` produced (tests/golden/ecapa.npz, made by
tests/golden/make_ecapa_golden.py) and, ragged, against its own B = 1 runs; the module's state-dict mirror; ``train()`` and
the global-context length floor; the ``eval_sim`` driver on a stub encoder; the six new C-ABI entries are declared, bound,
exported and refuse bad arguments without a GPU.  No kernel is launched here.

Tolerance: the restatement and the reference are both fp32 on the CPU and differ only in summation order; the reference's own
fp32-versus-fp64 distance (stored in the fixture) is 2-3e-7 relative L2, 2-3e-6 at T = 2 where the instance norm divides by a
two-frame spread.  1e-5 is the bound the generator asserted before it wrote the fixture."""
import ctypes as C
import json
import os
import re
import threading

import numpy as np
import pytest
import torch

import ecapa_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "ecapa.npz"))
FEAT_DIM, L, CHANNELS, EMB, SEED = 16, 4, 64, 24, 4100
TS = [int(t) for t in GOLD["ts"]]
ENTRIES = [("f5e_layer_mix_inorm", 10), ("f5e_res2_dconv", 16), ("f5e_time_stats", 10), ("f5e_se_scale", 11),
           ("f5e_bias_tanh", 9), ("f5e_attn_stats_pool", 10)]


def cfg_of(tag):
    return ER.make_cfg(FEAT_DIM, CHANNELS, EMB, tag == "g", L)


@pytest.fixture(scope="module")
def weights():
    return {tag: ER.synth_state_dict(cfg_of(tag), SEED) for tag in ("p", "g")}


def test_synth_state_dict_is_as_specified(weights):
    sd = weights["g"]
    n = sum(v.numel() for v in sd.values() if v.is_floating_point())
    assert 0.9e6 < n < 1.3e6          # 1536 is fixed: about a million values even at channels = 64
    again = ER.synth_state_dict(cfg_of("g"), SEED)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    assert not torch.equal(sd["linear.weight"], ER.synth_state_dict(cfg_of("g"), SEED + 1)["linear.weight"])
    for k, v in sd.items():
        if k.endswith("running_var"):
            assert 0.5 <= float(v.min()) and float(v.max()) <= 1.5
        if k.endswith("running_mean"):
            assert float(v.abs().max()) > 0.1
    # the hash itself: first values of stream 0 at seed 1 (splitmix64, top 53 bits), fixed for every machine
    assert (ER.hash_uniform(1, 0, 3) * (1 << 53)).astype(np.uint64).tolist() == \
        [3886858653415212, 6717404888216029, 6747740474277763]


@pytest.mark.parametrize("tag", ["p", "g"])
def test_ref_matches_reference_fixture(weights, tag):
    for T in TS:
        got = ER.forward(weights[tag], cfg_of(tag), torch.from_numpy(GOLD[f"hs_{T}"])[:, None])
        for k in ("out1", "out2", "out3", "out4", "pooled", "emb"):
            e = ER.rel_l2(got[k][0], GOLD[f"{tag}_{k}_{T}"])
            print(f"{tag} T={T} {k}: {e:.2e} (reference fp32 vs fp64 on emb: {float(GOLD[f'{tag}_err64_{T}']):.2e})")
            assert e < 1e-5, (tag, T, k, e)
    embs = {T: ER.forward(weights[tag], cfg_of(tag), torch.from_numpy(GOLD[f"hs_{T}"])[:, None])["emb"][0] for T in (150, 37)}
    cos = float(torch.nn.functional.cosine_similarity(embs[150], embs[37], dim=0))
    assert abs(cos - float(GOLD[f"{tag}_cos"])) < 1e-5


def ragged_batch(lengths, garbage=1e4, seed=0):
    T = max(lengths)
    hs = ER.hash_tensor(SEED + 77 + seed, 5, (L, len(lengths), T, FEAT_DIM), -garbage, garbage)
    for b, n in enumerate(lengths):
        hs[:, b, :n] = torch.from_numpy(GOLD[f"hs_{n}"])
    return hs


@pytest.mark.parametrize("tag", ["p", "g"])
def test_ref_ragged_rows_equal_their_batch_of_one(weights, tag):
    lengths = [150, 37, 9]
    got = ER.forward(weights[tag], cfg_of(tag), ragged_batch(lengths), torch.tensor(lengths))
    for b, n in enumerate(lengths):
        one = ER.forward(weights[tag], cfg_of(tag), torch.from_numpy(GOLD[f"hs_{n}"])[:, None])
        for k in ("out1", "out2", "out3", "out4"):
            assert ER.rel_l2(got[k][b, :n], one[k][0]) < 1e-5 and float(got[k][b, n:].abs().max() if n < 150 else 0) == 0
        assert ER.rel_l2(got["pooled"][b], one["pooled"][0]) < 1e-5 and ER.rel_l2(got["emb"][b], one["emb"][0]) < 1e-5


# ---- the module: a state-dict mirror that needs no GPU to be built and loaded ----

def build(tag, **kw):
    from f5e_tts_amd.eval.ecapa_tdnn import ECAPA_TDNN
    return ECAPA_TDNN(FEAT_DIM, channels=CHANNELS, emb_dim=EMB, global_context_att=tag == "g", feat_num=L, **kw)


@pytest.mark.parametrize("tag", ["p", "g"])
def test_state_dict_names_and_shapes(tag):
    want = list(zip([str(s) for s in GOLD[f"{tag}_names"]],
                    [tuple(int(d) for d in str(s).split()) for s in GOLD[f"{tag}_shapes"]]))
    got = [(k, tuple(v.shape)) for k, v in build(tag).state_dict().items()]
    assert got == want
    assert want == ER.head_shapes(cfg_of(tag))


def test_small_is_the_reference_configuration():
    from f5e_tts_amd.eval.ecapa_tdnn import ECAPA_TDNN_SMALL
    m = ECAPA_TDNN_SMALL(1024)
    assert (m.channels, m.emb_dim, m.feat_num, m.global_context_att) == (512, 256, 25, False)
    assert m.state_dict()["layer2.Res2Conv1dReluBn.convs.0.weight"].shape == (64, 64, 3)
    assert m.workspace_bytes(2, 500) > 0


def test_load_reference_checkpoint_ignores_the_upstream(weights):
    m = build("p")
    ckpt = {"model": dict(weights["p"])}
    ckpt["model"]["feature_extract.model.encoder.layers.0.self_attn.k_proj.weight"] = torch.zeros(4, 4)
    ckpt["model"]["feature_extract.model.mask_emb"] = torch.zeros(4)
    missing, unexpected = m.load_state_dict(ckpt["model"], strict=False)
    assert not missing and sorted(unexpected) == sorted(k for k in ckpt["model"] if k.startswith("feature_extract."))
    assert torch.equal(m.state_dict()["layer3.Res2Conv1dReluBn.bns.4.running_var"],
                       weights["p"]["layer3.Res2Conv1dReluBn.bns.4.running_var"])
    assert torch.equal(m.feature_weight, weights["p"]["feature_weight"])


def test_eval_only_and_argument_errors():
    from f5e_tts_amd._C import F5EError
    m = build("g")
    assert not m.training and m.eval() is m
    with pytest.raises(F5EError, match="training is out of scope"):
        m.train()
    with pytest.raises(F5EError, match="at least 2 frames"):
        m(torch.zeros(L, 1, 1, FEAT_DIM))
    with pytest.raises(F5EError, match=r"\[2, 5\]"):
        m(torch.zeros(L, 2, 5, FEAT_DIM), [5, 1])
    p = build("p")
    with pytest.raises(F5EError, match="no CPU path"):
        p(torch.zeros(L, 2, 5, FEAT_DIM), [5, 1])                 # length 1 is fine without the global context
    with pytest.raises(F5EError, match="feat_num"):
        p([torch.zeros(1, 5, FEAT_DIM)] * (L + 1))
    with pytest.raises(F5EError, match="hidden_states must be"):
        p(torch.zeros(L + 1, 1, 5, FEAT_DIM))
    with pytest.raises(F5EError, match="float32"):
        p(torch.zeros(L, 1, 5, FEAT_DIM, dtype=torch.float64))
    with pytest.raises(F5EError, match="WavLM upstream is not built"):
        p.embed_wavs([torch.zeros(16000)])


# ---- the driver ----

class StubEncoder:
    """Embedding = the mean over the valid frames of layer 0: cosine of two rows is then known in closed form."""

    def __init__(self):
        self.calls = []

    def __call__(self, hs, lengths):
        self.calls.append((tuple(hs.shape), list(lengths)))
        return torch.stack([hs[0, b, :n].mean(0) for b, n in enumerate(lengths)])


def make_eval_dir(tmp_path):
    gen, feats = tmp_path / "gen", tmp_path / "feats"
    gen.mkdir(), feats.mkdir(), (tmp_path / "prompts").mkdir()
    rng = np.random.default_rng(5)
    lines, want = [], {}
    for i, (tg, tp) in enumerate([(7, 4), (3, 9), (5, 5)]):
        utt = f"utt{i}"
        (gen / f"{utt}.wav").write_bytes(b"")
        a, b = rng.standard_normal((2, tg, 8)).astype(np.float32), rng.standard_normal((2, tp, 8)).astype(np.float32)
        np.save(feats / f"{utt}.npy", a), np.save(feats / f"prompt{i}.npy", b)
        lines.append(f"{utt}|some prompt text|prompts/prompt{i}.wav|the truth {i}")
        ea, eb = a[0].mean(0), b[0].mean(0)
        want[utt] = float(ea @ eb / (np.linalg.norm(ea) * np.linalg.norm(eb)))
    lines.append("missing|x|prompts/prompt0.wav|no generated wav: skipped")
    (tmp_path / "meta.lst").write_text("\n".join(lines) + "\n")
    return str(tmp_path / "meta.lst"), str(gen), str(feats), want


def test_run_sim_and_main_on_a_stub_encoder(tmp_path, capsys):
    from f5e_tts_amd.eval import eval_sim
    metalst, gen, feats, want = make_eval_dir(tmp_path)
    test_set = eval_sim.get_test_set(metalst, gen)
    assert [os.path.basename(g) for g, _, _ in test_set] == ["utt0.wav", "utt1.wav", "utt2.wav"]
    assert test_set[1][1] == os.path.join(os.path.dirname(metalst), "prompts/prompt1.wav") and test_set[2][2] == "the truth 2"
    enc = StubEncoder()
    res = eval_sim.run_sim(test_set, None, feats, "cpu", model=enc)
    assert [r["wav"] for r in res] == list(want) and all(abs(r["sim"] - want[r["wav"]]) < 1e-5 for r in res)
    assert enc.calls == [((2, 2, 7, 8), [7, 4]), ((2, 2, 9, 8), [3, 9]), ((2, 2, 5, 8), [5, 5])]    # one ragged B = 2 call each
    sim = eval_sim.main(["--metalst", metalst, "--gen_wav_dir", gen, "--feat_dir", feats, "--device", "cpu"], model=StubEncoder())
    assert abs(sim - np.mean(list(want.values()))) < 1e-5 and f"SIM: {sim:.5f}" in capsys.readouterr().out
    saved = json.load(open(os.path.join(gen, "_sim_results.json")))
    assert [r["wav"] for r in saved] == list(want) and all(abs(r["sim"] - want[r["wav"]]) < 1e-5 for r in saved)
    os.remove(os.path.join(feats, "prompt1.npy"))
    with pytest.raises(FileNotFoundError, match="prompt1.npy"):
        eval_sim.run_sim(test_set, None, feats, "cpu", model=StubEncoder())


# ---- the C ABI ----

def test_abi_entries_declared_bound_and_exported():
    from f5e_tts_amd import _C
    text = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _C.lib()
    for name, arity in ENTRIES:
        m = re.search(r"F5E_API int " + name + r"\((.*?)\);", text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == arity == len(_C.SIGNATURES[name])
        assert hasattr(lib, name) and f"`{name}`" in doc
    assert "ecapa.hip" in open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "Makefile")).read()


def on_thread(fn):
    """f5e_last_error is thread-local and nothing clears it: the calls that are MEANT to fail run on a thread of their own."""
    box = []
    t = threading.Thread(target=lambda: box.append(fn()))
    t.start(), t.join()
    assert box and box[0] is True


def test_argument_errors_without_a_device():
    from f5e_tts_amd import _C
    lib = _C.lib()
    p = C.c_void_p(4096)       # never dereferenced: every call below is refused before a launch

    def body():
        err = lambda: lib.f5e_last_error()  # noqa: E731
        assert lib.f5e_layer_mix_inorm(None, None, p, p, p, p, 4, 1, 8, 16) == -1 and b"null" in err()
        assert lib.f5e_layer_mix_inorm(None, p, p, p, p, p, 4, 1, 8, 18) == -1 and b"multiple of 4" in err()
        assert lib.f5e_layer_mix_inorm(None, p, p, p, p, p, 257, 1, 8, 16) == -1 and b"256" in err()
        res2 = lambda x=p, y=C.c_void_p(8192), Cc=64, d=2, first=0, count=7, ld=64: lib.f5e_res2_dconv(  # noqa: E731
            None, x, ld, y, ld, p, p, p, p, None, 1, 8, Cc, d, first, count)
        assert res2(x=None) == -1 and b"null" in err()
        assert res2(Cc=60, ld=64) == -1 and b"multiple of 8" in err()
        assert res2(first=3, count=5) == -1 and b"steps" in err()
        assert res2(d=0) == -1 and b"dilation" in err()
        assert res2(y=p) == -1 and b"in-place" in err()
        assert res2(Cc=1024, ld=1024) == -1 and b"LDS" in err()
        assert lib.f5e_time_stats(None, p, 64, None, None, None, 64, 1, 8, 64) == -1 and b"null" in err()
        assert lib.f5e_time_stats(None, p, 62, None, p, None, 64, 1, 8, 62) == -1 and b"multiples of 4" in err()
        assert lib.f5e_se_scale(None, p, 64, p, None, 64, p, 64, 1, 8, 64) == -1 and b"null" in err()
        assert lib.f5e_se_scale(None, p, 32, p, p, 64, p, 64, 1, 8, 64) == -1 and b"ld" in err()
        assert lib.f5e_bias_tanh(None, p, 128, None, 128, 1, 2, 8, 128) == -1 and b"null" in err()
        assert lib.f5e_bias_tanh(None, p, 128, p, 128, 3, 2, 8, 128) == -1 and b"add_rows" in err()
        assert lib.f5e_attn_stats_pool(None, p, 64, p, 64, None, None, 1, 8, 64) == -1 and b"null" in err()
        assert lib.f5e_attn_stats_pool(None, C.c_void_p(4100), 64, p, 64, None, p, 1, 8, 64) == -1 and b"aligned" in err()
        return True

    on_thread(body)
