"""The host side of Whisper's 16-bit weight modes (eval/whisper.py, xfmr_f32.py, the command lines, the ABI's new names): what a
checkpoint's tensors become on loading, without a GPU."""
import json
import os
import re
import struct

import pytest
import torch

import test_whisper_cpu as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, BF = torch.float32, torch.float16, torch.bfloat16
ST_NAME = {F32: "F32", F16: "F16", BF: "BF16"}
NEW = (("f5e_gemm_f32_w16_skinny_workspace", 3), ("f5e_gemm_f32_w16_skinny", 17), ("f5e_gemm_f32_w16", 22),
       ("f5e_whisper_embed_w16", 13), ("f5e_whisper_embed_w16_dev", 12))


def W():
    from f5e_tts_amd.eval import whisper
    return whisper


def raw(t):
    """The little-endian bytes of a tensor as a checkpoint stores them."""
    t = t.contiguous()
    return (t.view(torch.int16) if t.dtype == BF else t).numpy().tobytes()


def write_safetensors(path, tensors):
    header, blobs, off = {}, [], 0
    for name, t in tensors.items():
        b = raw(t)
        header[name] = dict(dtype=ST_NAME[t.dtype], shape=list(t.shape), data_offsets=[off, off + len(b)])
        blobs.append(b)
        off += len(b)
    h = json.dumps(header).encode("utf-8")
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(h)) + h + b"".join(blobs))


def test_read_safetensors_in_the_stored_dtype(tmp_path):
    a = torch.tensor([[1.0, -2.5, 2.0 ** -24], [65504.0, 0.0, -0.0]], dtype=F16)
    b = torch.tensor([1.0, -3.0e38, 1e-40, 0.0], dtype=BF)                       # 1e-40: a bf16 subnormal
    c = torch.tensor([[0.1], [1e-45]], dtype=F32)
    p = str(tmp_path / "three.safetensors")
    write_safetensors(p, dict(a=a, b=b, c=c))
    wide = W().read_safetensors(p)                                               # the default: everything float32, exact
    assert all(v.dtype == F32 for v in wide.values())
    assert torch.equal(wide["a"], a.float()) and torch.equal(wide["b"], b.float()) and torch.equal(wide["c"], c)
    got = W().read_safetensors(p, stored=True)
    for name, want in dict(a=a, b=b, c=c).items():
        assert got[name].dtype == want.dtype and got[name].shape == want.shape
        assert raw(got[name]) == raw(want), name                                 # bit for bit (-0.0 and the subnormals too)


def tiny_dir(path, dtype):
    """A checkpoint directory of the tiny model with every tensor stored in ``dtype``."""
    fx = WC.gold()
    os.makedirs(path, exist_ok=True)
    for name, obj in (("config.json", fx["config"]), ("generation_config.json", fx["generation_config"])):
        with open(os.path.join(path, name), "w") as f:
            json.dump(obj, f)
    sd = {k: torch.from_numpy(v.copy()).to(dtype) for k, v in fx["sd"].items()}
    write_safetensors(os.path.join(path, "model.safetensors"), sd)
    return sd


@pytest.mark.parametrize("dtype, mode", ((F16, "fp16"), (BF, "bf16"), (F32, "f32")))
def test_from_pretrained_dir_auto_resolves_the_stored_dtype(tmp_path, dtype, mode):
    Wh = W()
    sd = tiny_dir(str(tmp_path / mode), dtype)
    m = Wh.Whisper.from_pretrained_dir(str(tmp_path / mode), weights="auto")
    assert m.weights == mode and m.wdtype == Wh.WEIGHT_MODES[mode]
    for k, v in m.state_dict().items():
        want = sd[k] if Wh.is_matrix(k) else sd[k].float()                       # a matching type is a pure copy
        assert v.dtype == want.dtype and torch.equal(v, want), k
    # the default widens, as it always did
    d = Wh.Whisper.from_pretrained_dir(str(tmp_path / mode))
    assert d.weights == "f32" and all(v.dtype == F32 and torch.equal(v, sd[k].float()) for k, v in d.state_dict().items())
    with pytest.raises(Wh._C.F5EError, match="weights"):
        Wh.Whisper.from_pretrained_dir(str(tmp_path / mode), weights="int8")
    with pytest.raises(Wh._C.F5EError, match="weights"):
        Wh.Whisper(WC.tiny_cfg(), weights="auto")                                # "auto" needs a checkpoint to look at


def test_load_state_dict_rounds_to_nearest_even_and_refuses_overflow():
    Wh = W()
    sd = {k: torch.from_numpy(v.copy()) for k, v in WC.gold()["sd"].items()}
    k = "model.encoder.layers.0.fc1.weight"
    # fp16 has 10 fraction bits: 1 + 2^-11 lies halfway between 1 (even) and 1 + 2^-10 (odd), 1 + 3 2^-11 halfway between
    # 1 + 2^-10 (odd) and 1 + 2^-9 (even); one fp32 ulp beyond a halfway point goes up
    e = 2.0 ** -11
    cases16 = [(1 + e, 1.0), (1 + 3 * e, 1 + 2 * 2.0 ** -10), (1 + e + 2.0 ** -23, 1 + 2.0 ** -10), (-(1 + e), -1.0),
               (65519.0, 65504.0), (2.0 ** -25, 0.0), (3 * 2.0 ** -25, 2.0 ** -23)]
    # bf16 has 7 fraction bits
    e = 2.0 ** -8
    cases_bf = [(1 + e, 1.0), (1 + 3 * e, 1 + 2 * 2.0 ** -7), (1 + e + 2.0 ** -23, 1 + 2.0 ** -7), (-(1 + 3 * e), -(1 + 2.0 ** -6))]
    for mode, cases in (("fp16", cases16), ("bf16", cases_bf)):
        m = Wh.Whisper(WC.tiny_cfg(), weights=mode)
        mine = dict(sd)
        mine[k] = sd[k].clone()
        for i, (x, _) in enumerate(cases):
            mine[k].view(-1)[i] = x
        m.load_state_dict(mine)
        got = m.state_dict()
        assert got[k].dtype == Wh.WEIGHT_MODES[mode]
        for i, (x, want) in enumerate(cases):
            assert float(got[k].view(-1)[i]) == want, (mode, x, float(got[k].view(-1)[i]), want)
        # biases, LayerNorms and both position tables stay fp32, bit for bit
        for name, v in got.items():
            assert v.dtype == (Wh.WEIGHT_MODES[mode] if Wh.is_matrix(name) else F32), name
            if not Wh.is_matrix(name):
                assert torch.equal(v, sd[name]), name
        # any floating dtype is accepted: a float64 dict gives the same bits as its float32 rounding would
        m2 = Wh.Whisper(WC.tiny_cfg(), weights=mode)
        m2.load_state_dict({n: v.double() for n, v in mine.items()})
        assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    # 65520 is the first value that rounds to fp16's infinity; the refusal names the parameter and leaves bf16 / f32 alone
    bad = dict(sd)
    bad[k] = sd[k].clone()
    bad[k][1, 2] = -65520.0
    with pytest.raises(Wh._C.F5EError, match=r"model\.encoder\.layers\.0\.fc1\.weight holds 65520"):
        Wh.Whisper(WC.tiny_cfg(), weights="fp16").load_state_dict(bad)
    Wh.Whisper(WC.tiny_cfg(), weights="bf16").load_state_dict(bad)
    Wh.Whisper(WC.tiny_cfg()).load_state_dict(bad)
    bad[k][1, 2] = float("inf")                                                   # an infinity in the checkpoint is kept, not refused
    Wh.Whisper(WC.tiny_cfg(), weights="fp16").load_state_dict(bad)
    with pytest.raises(Wh._C.F5EError, match="floating"):
        Wh.Whisper(WC.tiny_cfg(), weights="fp16").load_state_dict({n: v.to(torch.int32) for n, v in sd.items()})
    with pytest.raises(Wh._C.F5EError, match="weights"):
        Wh.Whisper(WC.tiny_cfg(), weights="fp8")


def test_matrices_are_the_linears_the_convs_and_the_token_embedding():
    names = [n for n, _ in W().Whisper(WC.tiny_cfg()).named_parameters()]
    mats = {n for n in names if W().is_matrix(n)}
    assert mats == {n for n in names if n.endswith(".weight") and "layer_norm" not in n and "embed_positions" not in n}
    assert "model.decoder.embed_tokens.weight" in mats and "model.encoder.conv1.weight" in mats
    assert not any(n.endswith(".bias") for n in mats)


def test_cli_flags_parse_and_default_to_f32():
    from f5e_tts_amd.eval import eval_wer
    from f5e_tts_amd.infer import infer_cli, speech_edit
    base = {eval_wer: ["--gen_wav_dir", "d", "--metalst", "m", "--lang", "en"], infer_cli: [], speech_edit: []}
    for mod, argv in base.items():
        p = mod.build_parser()
        required = [a.option_strings[0] for a in p._actions if a.required and a.option_strings]
        argv = argv + [x for o in required if o not in argv for x in (o, "x")]
        assert p.parse_args(argv).whisper_weights == "f32", mod.__name__
        for v in ("f32", "fp16", "bf16", "auto"):
            assert p.parse_args(argv + ["--whisper_weights", v]).whisper_weights == v
        with pytest.raises(SystemExit):
            p.parse_args(argv + ["--whisper_weights", "fp8"])


def test_recognizer_hands_the_mode_to_the_model_and_its_assistant(tmp_path, monkeypatch):
    Wh = W()
    tiny_dir(str(tmp_path / "m"), F16)
    seen = []
    real = Wh.Whisper.from_pretrained_dir.__func__

    def spy(cls, path, weights="f32"):
        seen.append(weights)
        return real(cls, path, weights)
    monkeypatch.setattr(Wh.Whisper, "from_pretrained_dir", classmethod(spy))
    monkeypatch.setattr(Wh.Whisper, "prompt_ids", lambda self, *a, **k: [])
    r = Wh.WhisperRecognizer(str(tmp_path / "m"), device="cpu", weights="auto")
    assert seen == ["auto"] and r.model.weights == "fp16"
    Wh.WhisperRecognizer(str(tmp_path / "m"), device="cpu")
    assert seen == ["auto", "f32"]
    # the assistant takes the model's mode unless it is given its own
    del seen[:]
    r = Wh.WhisperRecognizer(str(tmp_path / "m"), device="cpu", weights="fp16", assistant_dir=str(tmp_path / "m"))
    assert seen == ["fp16", "fp16"] and r.assistant.weights == "fp16"
    del seen[:]
    r = Wh.WhisperRecognizer(str(tmp_path / "m"), device="cpu", weights="fp16", assistant_dir=str(tmp_path / "m"),
                             assistant_weights="f32")
    assert seen == ["fp16", "f32"] and r.model.weights == "fp16" and r.assistant.weights == "f32"


def test_xfmr_fold_and_stack_with_a_weight_type():
    from f5e_tts_amd import xfmr_f32 as X
    g = torch.Generator().manual_seed(0)
    lin = lambda n, k, bias=True: (torch.randn(n, k, generator=g), torch.randn(n, generator=g) if bias else None)   # noqa: E731
    q, k, v, out, fc1, fc2 = lin(8, 8), lin(8, 8, False), lin(8, 8), lin(8, 8), lin(16, 8), lin(8, 16)
    ln = (torch.randn(8, generator=g), torch.randn(8, generator=g))
    dev = torch.device("cpu")
    for wd in (F16, BF):
        w, b = X.fold(dev, out, wd)
        assert w.dtype == wd and b.dtype == F32 and torch.equal(w, out[0].to(wd)) and torch.equal(b, out[1])
        sw, sb = X.stack(dev, q, k, v, wdtype=wd)
        assert sw.dtype == wd and sw.shape == (24, 8) and sb.dtype == F32 and sb.shape == (24,)          # ONE stacked tensor
        assert torch.equal(sw, torch.cat([q[0], k[0], v[0]]).to(wd)) and torch.equal(sb[8:16], torch.zeros(8))
        L = X.fold_layer(dev, ln, q, k, v, out, ln, fc1, fc2, ln_x=ln, xq=q, xk=k, xv=v, xout=out, wdtype=wd)
        assert all(p[0].dtype == wd and p[1].dtype == F32 for p in (L.qkv, L.out, L.xq, L.xkv, L.xout))
        assert [t.dtype for t in L.ff] == [wd, F32, wd, F32]
        assert all(p[0].dtype == F32 and p[1].dtype == F32 for p in (L.ln1, L.ln_x, L.ln_ff))            # LayerNorm pairs stay fp32
    # without it nothing changes
    L = X.fold_layer(dev, ln, q, k, v, out, ln, fc1, fc2)
    assert L.qkv[0].dtype == F32 and torch.equal(L.qkv[0], torch.cat([q[0], k[0], v[0]]))


def test_abi_header_exports_and_ctypes_agree_on_the_new_names():
    from f5e_tts_amd import _C, ops
    header = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    emap = open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "exports.map")).read()
    assert "f5e_*" in emap
    for name, nargs in NEW:
        m = re.search(r"F5E_API int %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in f5e_abi.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs == len(_C.SIGNATURES[name]), name
        assert hasattr(_C.lib(), name), f"{name} is not exported"
        assert hasattr(ops, name[len("f5e_"):]), f"ops.{name[4:]} is missing"
    enum = re.search(r"enum \{ F5E_W_FP16 = (\d+), F5E_W_BF16 = (\d+) \};", header)
    assert enum and (int(enum.group(1)), int(enum.group(2))) == (_C.W_FP16, _C.W_BF16)
    assert ops.W16_TYPES == {F16: _C.W_FP16, BF: _C.W_BF16}
    mk = open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "Makefile")).read()
    assert "gemm_f32_w16.hip" in mk and all(h in mk for h in ("w_load.h", "gemm_f32_tile.h", "gemm_f32_skinny_body.h"))
    # the refusals that need no device
    import ctypes as C
    lib = _C.lib()
    n = C.c_ulonglong(7)
    assert lib.f5e_gemm_f32_w16_skinny_workspace(0, 16, C.byref(n)) != 0 and b"gemm_f32_w16_skinny_workspace" in lib.f5e_last_error()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.f5e_gemm_f32_w16_skinny(None, p, 16, p, 16, 3, None, 0, None, 0, p, 16, None, 0, 1, 4, 16) != 0
    assert b"wtype" in lib.f5e_last_error()
    assert lib.f5e_gemm_f32_w16_skinny(None, p, 16, p, 16, _C.W_FP16, None, 0, None, 0, p, 16, None, 0, 17, 4, 16) != 0
    assert b"1 <= M <= 16" in lib.f5e_last_error()
    assert lib.f5e_gemm_f32_w16(None, p, 16, 1, 0, p, 18, _C.W_BF16, None, 0, None, None, 0, 0, None, p, 16, None, 0, 1, 4, 16) != 0
    assert b"multiples of 4" in lib.f5e_last_error()
    assert lib.f5e_whisper_embed_w16(None, p, None, p, 9, p, p, 1, 1, 4, 0, 4, 4) != 0 and b"wtype" in lib.f5e_last_error()
    assert lib.f5e_whisper_embed_w16_dev(None, p, None, p, 9, p, p, 1, 4, p, 4, 4) != 0 and b"wtype" in lib.f5e_last_error()
