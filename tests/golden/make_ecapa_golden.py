"""Generates tests/golden/ecapa.npz from the reference's own ``ECAPA_TDNN`` (eval/ecapa_tdnn.py), imported where it lies.
The class fetches its WavLM upstream through ``torch.hub.load``; that call is replaced by a stub upstream (an nn.Module with
one parameter whose ``.model.encoder.layers`` has a length other than 24) that returns ``{"hidden_states": [...]}`` from a
tensor this script sets, so the reference's own ``forward`` runs end to end on hidden states of our choosing.  It pins
tests/ecapa_ref.py, csrc/ecapa.hip and f5e_tts_amd/eval/ecapa_tdnn.py.

Usage (where the reference checkout is; it never travels to the GPU machine):
    python tests/golden/make_ecapa_golden.py <reference root>

Configuration: feat_dim 16, 4 layers, channels 64, emb_dim 24, global_context_att False ("p") and True ("g"); weights =
``ecapa_ref.synth_state_dict(cfg, seed 4100)`` (never stored); B = 1 at T in {2, 5, 9, 37, 150}.  Stored: hs_<T> [L, T, 16]
(shared by both variants); per variant v and T: <v>_out1_<T> .. <v>_out4_<T> [T, 64], <v>_pooled_<T> [3072], <v>_emb_<T> [24],
<v>_err64_<T> (relative L2 of the reference's fp32 embedding against its own fp64 run); <v>_cos = cosine of the T = 150 and
T = 37 embeddings; <v>_names / <v>_shapes: the head's state-dict entries.  ``ecapa_ref.forward`` must match the reference to
1e-5 (relative L2, every tensor) before anything is written."""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ecapa_ref as ER  # noqa: E402

FEAT_DIM, L, CHANNELS, EMB = 16, 4, 64, 24
TS = (2, 5, 9, 37, 150)
SEED = 4100


class _Layers(nn.Module):
    def __init__(self):
        super().__init__()
        self.layers = nn.ModuleList([nn.Identity() for _ in range(3)])      # not 24: the fp32_attention patch is skipped


class _Model(nn.Module):
    def __init__(self):
        super().__init__()
        self.encoder = _Layers()


class StubUpstream(nn.Module):
    def __init__(self):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(1))
        self.model = _Model()
        self.hs = torch.zeros(L, 1, 1, FEAT_DIM)

    def forward(self, wavs):
        return {"hidden_states": [h.to(self.scale.dtype) for h in self.hs]}


def load_reference(ref_root: str):
    path = os.path.join(ref_root, "src", "f5_tts", "eval", "ecapa_tdnn.py")
    spec = importlib.util.spec_from_file_location("reference_ecapa", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref_root: str):
    torch.hub.load = lambda *a, **kw: StubUpstream()
    ref = load_reference(ref_root)
    out = {"ts": np.asarray(TS, np.int32)}
    hs = {T: ER.synth_hidden_states(SEED + T, L, 1, T, FEAT_DIM) for T in TS}
    for T in TS:
        out[f"hs_{T}"] = hs[T][:, 0].numpy()
    for tag, gc in (("p", False), ("g", True)):
        cfg = ER.make_cfg(FEAT_DIM, CHANNELS, EMB, gc, L)
        sd = ER.synth_state_dict(cfg, SEED)
        model = ref.ECAPA_TDNN(feat_dim=FEAT_DIM, channels=CHANNELS, emb_dim=EMB, global_context_att=gc).eval()
        assert model.feat_num == L
        missing, unexpected = model.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.startswith("feature_extract.") for k in missing), (missing, unexpected)
        head = [(k, tuple(v.shape)) for k, v in model.state_dict().items() if not k.startswith("feature_extract.")]
        assert head == ER.head_shapes(cfg)
        out[f"{tag}_names"] = np.asarray([k for k, _ in head])
        out[f"{tag}_shapes"] = np.asarray([" ".join(str(d) for d in s) for _, s in head])
        model64 = ref.ECAPA_TDNN(feat_dim=FEAT_DIM, channels=CHANNELS, emb_dim=EMB, global_context_att=gc).eval()
        model64.load_state_dict(sd, strict=False)
        model64 = model64.double()
        taps = {}
        for name in ("layer1", "layer2", "layer3", "layer4", "pooling"):
            getattr(model, name).register_forward_hook(lambda m, i, o, name=name: taps.__setitem__(name, o.detach()))
        embs = {}
        for T in TS:
            model.feature_extract.hs = hs[T]
            model64.feature_extract.hs = hs[T].double()
            with torch.no_grad():
                emb = model([torch.zeros(16)])
                emb64 = model64([torch.zeros(16, dtype=torch.float64)])
            assert emb.shape == (1, EMB) and torch.isfinite(emb).all()
            got = {"out1": taps["layer1"], "out2": taps["layer2"], "out3": taps["layer3"], "out4": taps["layer4"]}
            got = {k: v[0].T for k, v in got.items()}
            got.update(pooled=taps["pooling"][0], emb=emb[0])
            mine = ER.forward(sd, cfg, hs[T])
            for k, v in got.items():
                e = ER.rel_l2(mine[k][0], v)
                assert e < 1e-5, (tag, T, k, e)
                out[f"{tag}_{k}_{T}"] = v.numpy().astype(np.float32)
            out[f"{tag}_err64_{T}"] = np.asarray(ER.rel_l2(emb, emb64), np.float64)
            embs[T] = emb[0]
            print(f"{tag} T={T}: |emb| {float(emb.norm()):.4f}  fp32 vs fp64 {float(out[f'{tag}_err64_{T}']):.2e}  "
                  f"ecapa_ref vs reference (emb) {ER.rel_l2(mine['emb'][0], emb[0]):.2e}")
        out[f"{tag}_cos"] = np.asarray(float(torch.nn.functional.cosine_similarity(embs[150], embs[37], dim=0)), np.float32)
        print(f"{tag}: cosine(T=150, T=37) = {float(out[f'{tag}_cos']):.6f}")
    path = os.path.join(HERE, "ecapa.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main(sys.argv[1])
