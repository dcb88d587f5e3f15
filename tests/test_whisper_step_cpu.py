"""The captured Whisper decode step, the parts that need no GPU (``generate_from_kv(step_graph=, step_gemm=)``, the
device-position entry points of csrc/whisper_step.hip): the refusals by name before any launch, the wrappers' refusal of CPU
tensors, the C ABI's three declarations of the new entries, the unchanged arities of the old ones, and the wirings on stubs."""
import os
import re

import pytest
import torch

from test_whisper_cpu import tiny_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, I32 = torch.float32, torch.int32
NEW = (("f5e_attn_decode_dev_f32", 16), ("f5e_whisper_embed_dev", 11), ("f5e_greedy_pick_dev", 17),
       ("f5e_whisper_ts_pick_dev", 20), ("f5e_whisper_sample_pick_dev", 22))
OLD = (("f5e_attn_decode_f32", 17), ("f5e_attn_decode_from_f32", 18), ("f5e_text_gather", 11), ("f5e_whisper_embed", 12),
       ("f5e_greedy_pick", 17), ("f5e_whisper_ts_pick", 20), ("f5e_whisper_sample_pick", 24), ("f5e_whisper_ts_rule", 17),
       ("f5e_gemm_f32_skinny", 16))

_model = {}


def model():
    if not _model:
        _model["m"] = tiny_model()
    return _model["m"]


# ---- refusals by name, before any launch (the model and every tensor live on the CPU: a launch would fail differently) --------

@pytest.mark.parametrize("kw,match", (
    (dict(step_graph=True, beam_size=3), "step_graph with beam_size = 3"),
    (dict(step_graph=True, return_beams=True), "step_graph with beam_size"),
    (dict(step_graph=True, assistant=("draft", None)), "step_graph with assistant"),
    (dict(step_graph=True, return_token_timestamps=True), "step_graph with return_token_timestamps"),
    (dict(step_gemm="skinny"), "step_gemm = 'skinny' needs step_graph"),
    (dict(step_graph=True, step_gemm="bf16"), "step_gemm = 'bf16' must be 'f32' or 'skinny'"),
    (dict(step_gemm="tf32"), "step_gemm = 'tf32' must be 'f32' or 'skinny'"),
    (dict(step_graph=1), "step_graph = 1 must be a bool"),
))
def test_generate_from_kv_refusals_by_name(kw, match):
    from f5e_tts_amd._C import F5EError
    with pytest.raises(F5EError, match=match):
        model().generate_from_kv(None, [141, 142, 146, 159], **kw)


@pytest.mark.parametrize("kw,match", (
    (dict(step_graph=True, beam_size=2), "step_graph with beam_size = 2"),
    (dict(step_graph=True, assistant=object()), "step_graph with assistant"),
    (dict(step_graph=True, return_token_timestamps=True), "step_graph with return_token_timestamps"),
    (dict(step_gemm="skinny"), "needs step_graph"),
    (dict(step_graph=True, step_gemm="fast"), "must be 'f32' or 'skinny'"),
))
def test_generate_refusals_by_name(kw, match):
    from f5e_tts_amd._C import F5EError
    with pytest.raises(F5EError, match=match):
        model().generate(torch.zeros(1, 16000), None, "en", **kw)


@pytest.mark.parametrize("kw,match", (
    (dict(step_graph=True, beam_size=2), "step_graph with beam_size = 2"),
    (dict(step_graph=True, assistant=object()), "step_graph with assistant"),
    (dict(step_gemm="skinny"), "needs step_graph"),
    (dict(step_graph=True, step_gemm=None), "must be 'f32' or 'skinny'"),
))
def test_transcribe_long_refusals_by_name(kw, match):
    from f5e_tts_amd._C import F5EError
    with pytest.raises(F5EError, match=match):
        model().transcribe_long(torch.zeros(1, 16000), None, "en", **kw)


def test_the_name_graph_stays_refused_and_the_keywords_are_keyword_only():
    import inspect
    from f5e_tts_amd._C import F5EError
    from f5e_tts_amd.eval.whisper import Whisper, WhisperRecognizer
    with pytest.raises(F5EError, match="graph = True is out of scope"):
        model().transcribe_long(torch.zeros(1, 16000), None, "en", graph=True)
    for fn in (Whisper.generate_from_kv, Whisper.generate, Whisper.transcribe_long):
        ps = [p for p in inspect.signature(fn).parameters.values() if p.kind != p.VAR_KEYWORD]
        assert [p.name for p in ps[-2:]] == ["step_graph", "step_gemm"], fn.__name__
        assert all(p.kind == p.KEYWORD_ONLY for p in ps[-2:]) and ps[-2].default is False and ps[-1].default == "f32"
    ps = inspect.signature(WhisperRecognizer.__init__).parameters
    assert ps["step_graph"].default is False and ps["step_gemm"].default == "f32"


def test_skinny_above_sixteen_rows_is_refused_by_name():
    """The row count is known once the state is asked for: refused before any launch or allocation."""
    from f5e_tts_amd import ops
    from f5e_tts_amd._C import F5EError
    with pytest.raises(F5EError, match="step_gemm = 'skinny' is built for at most 16 rows \\(got 17\\)"):
        model()._step_state(ops.SKINNY_MAX_M + 1, "greedy", False, "skinny", 150, torch.device("cpu"))


# ---- the wrappers have no CPU path ---------------------------------------------------------------------------------------------

def test_the_new_wrappers_refuse_cpu_tensors():
    from f5e_tts_amd import ops
    from f5e_tts_amd._C import F5EError
    R, P, D, V = 2, 8, 64, 160
    z = lambda *s: torch.zeros(*s, dtype=I32)       # noqa: E731
    f = lambda *s: torch.zeros(*s, dtype=F32)       # noqa: E731
    rec = ops.whisper_step_record(3, 2)
    assert rec.dtype == I32 and rec.tolist() == [3, 2, 0, 0, 0, 0, 0, 0] and ops.STEP_REC_WORDS == 8
    with pytest.raises(F5EError, match="there is no CPU path"):
        ops.attn_decode_dev_f32(f(R, 3 * D), f(R, P, D), f(R, P, D), rec, 4, 0.25)
    with pytest.raises(F5EError, match="there is no CPU path"):
        ops.whisper_embed_dev(z(R), f(V, D), f(P, D), f(R, D), rec)
    with pytest.raises(F5EError, match="there is no CPU path"):
        ops.greedy_pick_dev(f(R, V), z(R, P), z(R), z(R), z(1), rec, 140)
    with pytest.raises(F5EError, match="there is no CPU path"):
        ops.whisper_ts_pick_dev(f(R, V), z(R, P), z(R), z(R), z(1), f(R), rec, 100, 110)
    with pytest.raises(F5EError, match="there is no CPU path"):
        ops.whisper_sample_pick_dev(f(R, V), z(R, P), z(R), z(R), z(1), f(R), rec, 100, 110, z(R), z(R))


def test_the_step_record_packs_seed_and_temperature():
    import struct
    from f5e_tts_amd import ops
    from f5e_tts_amd._C import F5EError
    rec = ops.whisper_step_record(7, 4, seed=(0xDEADBEEF << 32) | 0x80000001, temperature=0.4).tolist()
    assert rec[:2] == [7, 4] and rec[5:] == [0, 0, 0]
    assert rec[2] & 0xffffffff == 0x80000001 and rec[3] & 0xffffffff == 0xDEADBEEF
    assert struct.unpack("<f", struct.pack("<i", rec[4]))[0] == struct.unpack("<f", struct.pack("<f", 0.4))[0]
    with pytest.raises(F5EError, match="seed"):
        ops.whisper_step_record(0, 1, seed=1 << 64)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------

def _declared(header, name):
    m = re.search(r"F5E_API int %s\(([^;]*)\);" % name, header)
    assert m, name
    return len(m.group(1).split(","))


def test_abi_declares_and_binds_the_new_entries():
    from f5e_tts_amd import _C, ops
    header = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    emap = open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "exports.map")).read()
    source = open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "whisper_step.hip")).read()
    assert "f5e_*" in emap                                            # the version script exports the whole f5e_ prefix
    for name, nargs in NEW:
        assert _declared(header, name) == nargs == len(_C.SIGNATURES[name]), name
        m = re.search(r'extern "C" int %s\(([^)]*)\)' % name, source)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(ops, name[len("f5e_"):]), name
    assert "#define F5E_ABI_VERSION 2 " in header and _C.ABI_VERSION == 2       # functions were only added
    assert "whisper_step.hip" in open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "Makefile")).read()


def test_the_old_entries_keep_their_arities():
    from f5e_tts_amd import _C
    header = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    for name, nargs in OLD:
        assert _declared(header, name) == nargs == len(_C.SIGNATURES[name]), name


def test_no_kernel_of_the_step_waits_for_another_workgroup():
    """The stream is the only ordering: the source has no grid barrier, no cooperative launch and no spin on memory."""
    source = open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "whisper_step.hip")).read()
    code = "\n".join(line.split("//")[0] for line in source.split("\n"))
    for word in ("cooperative", "grid.sync", "while (", "atomicCAS", "__threadfence", "volatile"):
        assert word not in code, word


# ---- the wirings ---------------------------------------------------------------------------------------------------------------

def test_eval_wer_and_infer_cli_have_the_flags():
    from f5e_tts_amd.eval import eval_wer
    from f5e_tts_amd.infer import infer_cli
    args = infer_cli.build_parser().parse_args(["--whisper_dir", "W", "--whisper_step_graph"])
    assert args.whisper_step_graph is True
    assert infer_cli.build_parser().parse_args([]).whisper_step_graph is False      # opt-in: nothing changes without the flag
    p = eval_wer.build_parser()
    a = p.parse_args(["--metalst", "m", "--gen_wav_dir", "g", "--lang", "en", "--whisper_step_graph", "--whisper_step_gemm", "skinny"])
    assert a.whisper_step_graph is True and a.whisper_step_gemm == "skinny"
    b = p.parse_args(["--metalst", "m", "--gen_wav_dir", "g", "--lang", "en"])
    assert b.whisper_step_graph is False and b.whisper_step_gemm == "f32"


def test_recognizer_refuses_the_combinations_before_it_loads(tmp_path):
    from f5e_tts_amd._C import F5EError
    from f5e_tts_amd.eval.whisper import WhisperRecognizer
    with pytest.raises(F5EError, match="step_graph with beam_size = 5"):
        WhisperRecognizer(str(tmp_path / "none"), "cpu", "en", beam_size=5, step_graph=True)
    with pytest.raises(F5EError, match="step_graph with assistant"):
        WhisperRecognizer(str(tmp_path / "none"), "cpu", "en", assistant_dir=str(tmp_path), step_graph=True)
    with pytest.raises(F5EError, match="needs step_graph"):
        WhisperRecognizer(str(tmp_path / "none"), "cpu", "en", step_gemm="skinny")
