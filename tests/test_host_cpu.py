"""CPU-side tests: the C-ABI library loads and exports what include/f5e_abi.h declares; the module mirrors keep the
reference's state_dict layout; caller mirrors (chunking, duration/RMS/cross-fade rules, checkpoint loading, CLI flag
merge, bucketing/sharding) match fixtures captured from the reference; the product path fails loudly without a GPU.
No kernel is launched here."""
import ast
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")


# ------------------------------------------------------------------ C ABI

def declared_functions():
    text = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#ifdef F5E_TOOLS.*?#endif", "", text, flags=re.S)   # diagnostics of the tools build, not shipped
    return sorted(set(re.findall(r"\b(f5e_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from f5e_tts_amd import _C
    lib = _C.lib()
    names = declared_functions()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in f5e_abi.h but not exported"
        assert n in _C.SIGNATURES, f"{n} has no ctypes signature"
    assert lib.f5e_abi_version() == _C.ABI_VERSION == 2
    assert lib.f5e_last_error() == b""


def test_shipped_library_has_no_debug_hook():
    """The in-kernel timestamp hook is process-wide mutable state: tools build only (include/f5e_abi.h, F5E_TOOLS)."""
    from f5e_tts_amd import _C
    assert not hasattr(_C.lib(), "f5e_debug_convpos_trace")


def test_workspace_bytes_planner():
    """f5e_workspace_bytes: sizes follow the plan's shape, offsets are 256-byte aligned and disjoint, optional
    buffers appear only when the shape asks for them.  (engine.make_plan carves exactly this arena: GPU test.)"""
    import ctypes as C
    from f5e_tts_amd import _C
    lib = _C.lib()
    p, w = _C.DitPlan(), _C.DitWorkspace()
    p.S, p.B, p.N, p.D, p.H, p.FF, p.L, p.mel, p.mod_rows = 2, 1, 469, 1024, 16, 2048, 22, 100, 1
    assert lib.f5e_workspace_bytes(C.byref(p), C.byref(w)) == 0
    M, n_pad = 2 * 469, 512
    assert w.n_pad == n_pad
    want = dict(h0=M * 1024 * 4, h0_bf16=M * 1024 * 2, c1=M * 1024 * 2, x=M * 1024 * 4, hn=M * 1024 * 2,
                q=2 * 16 * n_pad * 64 * 2, k=2 * 16 * n_pad * 64 * 2, vt=2 * 16 * n_pad * 64 * 2, ao=M * 1024 * 2,
                ff=M * 2048 * 2, pred=M * 100 * 4, ln_stats=0, skip_res=0, skip_tmp=0, ln_rowmean=0)
    got = {n: int(w.bytes[i]) for i, n in enumerate(_C.WS_NAMES)}
    assert got == want
    end = 0
    for i in range(len(_C.WS_NAMES)):
        assert w.offset[i] % 256 == 0 and w.offset[i] >= end
        end = w.offset[i] + w.bytes[i]
    assert w.total >= end and w.total % 256 == 0
    p.fuse_ln, p.w_skip = 1, 8
    assert lib.f5e_workspace_bytes(C.byref(p), C.byref(w)) == 0
    got = {n: int(w.bytes[i]) for i, n in enumerate(_C.WS_NAMES)}
    assert got["ln_stats"] == M * 16 * 2 * 4 and got["skip_res"] == got["skip_tmp"] == M * 1024 * 4
    assert got["ln_rowmean"] == M * 4
    p.N = 0
    assert lib.f5e_workspace_bytes(C.byref(p), C.byref(w)) == -1 and b"workspace_bytes" in lib.f5e_last_error()


def test_abi_rejects_bad_shapes_without_launching():
    import ctypes as C
    from f5e_tts_amd import _C
    lib = _C.lib()
    rc = lib.f5e_gemm_bf16_bias(None, C.c_void_p(8), 64, C.c_void_p(8), 64, None, C.c_void_p(8), 64, 4, 4, 60, 0, 0, 0)
    assert rc == -1 and b"multiple of 64" in lib.f5e_last_error()
    rc = lib.f5e_layernorm(None, C.c_void_p(8), 100, C.c_void_p(8), 100, 1, None, None, None, None, 0, 0, 1, None, 0, 4,
                           100, 1e-6)
    assert rc == -1 and b"multiple of 256" in lib.f5e_last_error()
    rc = lib.f5e_flash_attn(None, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 1024, None, 1, 16, 100,
                            100, 0)
    assert rc == -1 and b"n_pad" in lib.f5e_last_error()
    rc = lib.f5e_adaln_pre(None, C.c_void_p(8), 1024, C.c_void_p(8), 1024, C.c_void_p(8), 1024, 1, 10, None, 0,
                           C.c_void_p(8), 16, None, 10, 1024)
    assert rc == -1 and b"adaln_pre" in lib.f5e_last_error()          # no row_mean buffer


def test_product_path_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from f5e_tts_amd import _C, ops
    from f5e_tts_amd.model import CFM, DiT, MelSpec
    with pytest.raises(_C.F5EError):
        ops.require_device()
    with pytest.raises(_C.F5EError):
        MelSpec()(torch.zeros(1, 4096))
    dit = DiT(dim=1024, depth=1, heads=16, ff_mult=2, text_dim=256, conv_layers=1, text_num_embeds=30)
    with pytest.raises(_C.F5EError):
        dit.sample(torch.zeros(1, 8, 100), torch.zeros(1, 8, 100), None, None, torch.tensor(0.5), False, False, False)
    with pytest.raises(_C.F5EError):
        CFM(transformer=dit).sample(torch.zeros(1, 8, 100), torch.zeros(1, 3, dtype=torch.long), duration=16, steps=2)
    with pytest.raises(NotImplementedError):
        dit(torch.zeros(1))


def test_no_product_import_of_oracle():
    pkg = os.path.join(ROOT, "f5e-tts_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(d, f), encoding="utf-8").read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b|f5e_oracle|oracle/", src, flags=re.M), \
                    f"{f} imports / links the oracle"


# ------------------------------------------------------------------ state_dict layout

@pytest.mark.parametrize("tag", ["b1", "b2_ppg_tts"])
def test_state_dict_layout_matches_reference(tag):
    from f5e_tts_amd.model import DiT
    z = np.load(os.path.join(GOLD, f"dit_{tag}.npz"))
    meta = ast.literal_eval(str(z["meta"]))
    ref = {k[2:]: z[k].shape for k in z.files if k.startswith("w/")}
    ppg = dict(use_ppg=meta["n_ppg"] > 0, ppg_dim=32, use_transformer=False)
    m = DiT(dim=meta["dim"], depth=meta["depth"], heads=meta["heads"], dim_head=64, ff_mult=meta["ff_mult"],
            mel_dim=meta["mel_dim"], text_num_embeds=meta["text_num_embeds"], text_dim=meta["text_dim"],
            conv_layers=meta["conv_layers"], qk_norm=meta.get("qk_norm"), pe_attn_head=meta.get("pe_attn_head"),
            long_skip_connection=meta.get("long_skip_connection", False),
            text_mask_padding=meta.get("text_mask_padding", True), ppg_config=ppg)
    mine = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert mine == {k: tuple(v) for k, v in ref.items()}
    m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}, strict=True)


def test_unett_state_dict_layout_matches_reference():
    from f5e_tts_amd.model import UNetT
    for tag, skip in (("concat_b1", "concat"), ("add_b2", "add")):
        z = np.load(os.path.join(GOLD, f"unett_{tag}.npz"))
        ref = {k[2:]: tuple(z[k].shape) for k in z.files if k.startswith("w/")}
        m = UNetT(dim=128, depth=4, heads=2, dim_head=64, ff_mult=2, mel_dim=20, text_num_embeds=50, text_dim=32,
                  conv_layers=2, skip_connect_type=skip)
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == ref
        m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}, strict=True)


def test_v1_base_layout_and_zero_init():
    from f5e_tts_amd.model import DiT
    m = DiT(dim=1024, depth=22, heads=16, ff_mult=2, text_dim=512, conv_layers=4, text_num_embeds=2545)
    sd = m.state_dict()
    assert len(sd) == 364 and sum(p.numel() for p in m.parameters()) == 337096804
    assert sd["input_embed.proj.weight"].shape == (1024, 712)
    assert float(sd["proj_out.weight"].abs().max()) == 0 and float(sd["transformer_blocks.3.attn_norm.linear.bias"].abs().max()) == 0


# ------------------------------------------------------------------ callers vs reference fixtures

def callers():
    return json.load(open(os.path.join(GOLD, "callers.json")))


def test_chunk_text_matches_reference():
    from f5e_tts_amd.infer.utils_infer import chunk_text
    for case in callers()["chunk_text"]:
        assert chunk_text(case["text"], max_chars=case["max_chars"]) == case["chunks"]


def test_infer_batch_process_rules_match_reference():
    from f5e_tts_amd.infer import utils_infer as U

    class Model:
        def __init__(self):
            self.calls = []

        def sample(self, **kw):
            self.calls.append(kw)
            return torch.zeros(1, kw["duration"], 100), None

    class Voc:
        def decode(self, mel):
            n = 256 * (mel.shape[-1] - 1)
            return (torch.arange(n, dtype=torch.float32)[None] % 97) / 97.0 - 0.5

    g = torch.Generator().manual_seed(21)
    for case in callers()["batch"]:
        audio = case["amp"] * torch.randn(2, case["nw"], generator=g)
        m = Model()
        wave, sr, spec = next(U.infer_batch_process((audio, 24000), case["ref_text"], case["gens"], m, Voc(),
                                                    cross_fade_duration=case["cross_fade"], speed=case["speed"],
                                                    fix_duration=case["fix_duration"], device="cpu"))
        assert [c["duration"] for c in m.calls] == case["durations"]
        assert [list(c["cond"].shape) for c in m.calls] == case["cond_shapes"]
        assert all(c["steps"] == 32 and c["cfg_strength"] == 2.0 and c["sway_sampling_coef"] == -1 for c in m.calls)
        assert len(wave) == case["wave_len"] and list(spec.shape) == case["spec_shape"]
        np.testing.assert_allclose(wave[:8], case["wave_head"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(float(np.sum(wave)), case["wave_sum"], rtol=1e-5, atol=1e-3)
        np.testing.assert_allclose(float(np.abs(wave).sum()), case["wave_abs_sum"], rtol=1e-5)


def test_ascii_tokeniser_and_duration_rule():
    from f5e_tts_amd.infer.utils_infer import convert_char_to_pinyin, plan_batch
    assert convert_char_to_pinyin(["end.Next one;ok"]) == [list("end. Next one, ok")]
    assert convert_char_to_pinyin(["it's 2 fast"]) == [list("it's 2 fast")]
    assert plan_batch(187, "Some call me nature. ", "Hi.", 1.0, None) == (187 + int(187 / 21 * 3 / 0.3), 0.3)
    assert plan_batch(100, "abcd", "x" * 40, 2.0, None) == (100 + int(100 / 4 * 40 / 2.0), 2.0)
    assert plan_batch(100, "abcd", "x" * 40, 1.0, 6.5)[0] == int(6.5 * 24000 / 256)


@pytest.mark.parametrize("ext", ["pt", "safetensors"])
def test_load_checkpoint_matches_reference_key_handling(tmp_path, ext):
    from f5e_tts_amd.infer.utils_infer import load_checkpoint
    ref = callers()["load_checkpoint"]
    lin = torch.nn.Linear(3, 2)
    sd = {"ema_model." + k: v.detach().clone() + 1 for k, v in lin.state_dict().items()}
    sd.update({"ema_model.mel_spec.mel_stft.mel_scale.fb": torch.zeros(2),
               "ema_model.mel_spec.mel_stft.spectrogram.window": torch.zeros(2)})
    path = str(tmp_path / f"m.{ext}")
    if ext == "pt":
        sd.update({"initted": torch.tensor(True), "step": torch.tensor(5)})
        assert sorted(sd) == ref["in_keys"]
        torch.save({"ema_model_state_dict": sd}, path)
    else:
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in sd.items()}, path)
    loaded = load_checkpoint(torch.nn.Linear(3, 2), path, "cpu", use_ema=True)
    assert sorted(loaded.state_dict()) == ref["loaded_keys"]
    assert abs(float((loaded.weight - lin.weight).mean()) - ref["weight_delta"]) < 1e-6


def test_cli_flag_merge_precedence_and_falsy_quirk():
    """flag > toml > default; falsy flag values fall through (reference infer_cli.py:181-211, restated from the source
    text: the module executes at import time, so it cannot be imported to capture fixtures)."""
    from f5e_tts_amd.infer.infer_cli import build_parser, resolve_settings, split_voices
    P = build_parser()
    s = resolve_settings(P.parse_args([]), {})
    assert (s["model"], s["nfe_step"], s["cfg_strength"], s["sway_sampling_coef"], s["speed"]) == \
        ("F5TTS_v1_Base", 32, 2.0, -1.0, 1.0)
    assert s["target_rms"] == 0.1 and s["cross_fade_duration"] == 0.15 and s["fix_duration"] is None
    s = resolve_settings(P.parse_args(["--nfe_step", "16", "-t", "hi"]), {"nfe_step": 8, "speed": 1.5, "gen_text": "toml"})
    assert s["nfe_step"] == 16 and s["speed"] == 1.5 and s["gen_text"] == "hi"
    s = resolve_settings(P.parse_args(["--cfg_strength", "0", "--sway_sampling_coef", "0"]), {"cfg_strength": 3.0})
    assert s["cfg_strength"] == 3.0 and s["sway_sampling_coef"] == -1.0       # falsy flags fall through
    s = resolve_settings(P.parse_args(["-s", ""]), {"ref_text": "from toml"})
    assert s["ref_text"] == ""                                                   # ref_text uses `is not None`
    assert split_voices("[main] Hello. [town] Hi there. plain") == [("main", "Hello."), ("town", "Hi there. plain")]
    assert split_voices("no tags") == [("main", "no tags")]
    flags = {a.option_strings[-1] for a in P._actions}
    for f in ("--config", "--model", "--model_cfg", "--ckpt_file", "--vocab_file", "--ref_audio", "--ref_text",
              "--gen_text", "--gen_file", "--output_dir", "--output_file", "--save_chunk", "--remove_silence",
              "--load_vocoder_from_local", "--vocoder_name", "--target_rms", "--cross_fade_duration", "--nfe_step",
              "--cfg_strength", "--sway_sampling_coef", "--speed", "--fix_duration", "--device"):
        assert f in flags


def test_arch_config_and_vocab():
    from f5e_tts_amd.infer.infer_cli import load_arch
    from f5e_tts_amd.model.utils import get_tokenizer, list_str_to_idx
    arch = load_arch("F5TTS_v1_Base", "")
    assert arch == dict(dim=1024, depth=22, heads=16, ff_mult=2, text_dim=512, text_mask_padding=True, qk_norm=None,
                        conv_layers=4, pe_attn_head=None)
    vocab, size = get_tokenizer(os.path.join(ROOT, "f5e-tts_amd", "infer", "examples", "vocab.txt"))
    assert size == 2545 and vocab[" "] == 0
    ids = list_str_to_idx([list("ab c"), list("a")], vocab)
    assert ids.shape == (2, 4) and ids[1, 1:].tolist() == [-1, -1, -1] and ids[0, 2] == 0


# ------------------------------------------------------------------ bucketing / sharding

def test_bucketing_and_partitions():
    from f5e_tts_amd.eval.eval_infer_batch import (bucket_batches, flop_fwd, lpt_partition, split_between_processes,
                                                    total_mel_len)
    assert abs(flop_fwd(469) / 1e9 - 197.8) < 0.1 and abs(flop_fwd(938) / 1e9 - 435.0) < 0.2
    items = list(range(11))
    parts = [split_between_processes(items, r, 4) for r in range(4)]
    assert parts == [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10]]
    lens = [300 + (37 * i) % 3000 for i in range(97)]
    b1 = bucket_batches(lens, infer_batch_size=1)
    assert sorted(i for b in b1 for i in b) == list(range(97)) and all(len(b) == 1 for b in b1)
    assert b1 == bucket_batches(lens, infer_batch_size=1)              # seed-666 shuffle is deterministic
    b2 = bucket_batches(lens, infer_batch_size=4000)
    assert sorted(i for b in b2 for i in b) == list(range(97)) and max(len(b) for b in b2) > 1
    with pytest.raises(ValueError):
        bucket_batches([100])
    costs = [flop_fwd(n) for n in lens]
    lp = lpt_partition(costs, 8)
    assert sorted(i for p in lp for i in p) == list(range(97))
    loads = [sum(costs[i] for i in p) for p in lp]
    assert max(loads) / (sum(loads) / 8) < 1.05                         # near-perfect balance
    assert total_mel_len(187, "Some call me nature. ", "Hello world") == 187 + int(187 / 21 * 11)


def test_eval_prompt_bucketing_and_ascii_tokens_equal_the_reference_capture():
    """Integer / index work of the eval driver, bit-exact against tests/golden/eval_prompts.json -- captured by
    make_golden.py from the reference's own get_inference_prompt (eval/utils_eval.py:77-219) and convert_char_to_pinyin
    (model/utils.py:270-311): the trailing-space rule, total_mel_len, bucket index, flush order, residual buckets in bucket
    order, the seed-666 shuffle -> the ORDERED batches; and the ASCII token lists."""
    from f5e_tts_amd.eval.eval_infer_batch import bucket_batches, total_mel_len
    from f5e_tts_amd.infer.utils_infer import convert_char_to_pinyin
    gold = json.load(open(os.path.join(GOLD, "eval_prompts.json")))
    utts, ref_lens, totals, texts = [], [], [], []
    for utt, ptxt, wav, gtxt in gold["meta"]:
        n = int(os.path.basename(wav)[:-4].split("_")[0][1:])
        if len(ptxt[-1].encode("utf-8")) == 1:
            ptxt = ptxt + " "
        utts.append(utt)
        ref_lens.append(n // 256)
        totals.append(total_mel_len(n // 256, ptxt, gtxt))
        texts.append(ptxt + gtxt)
    for case in gold["cases"]:
        want = [b["utts"] for b in case["batches"]]
        got = bucket_batches(totals, infer_batch_size=case["infer_batch_size"], num_buckets=case["num_buckets"])
        assert [[utts[i] for i in b] for b in got] == want, case["infer_batch_size"]
        for b, idx in zip(case["batches"], got):
            assert b["total_mel_lens"] == [totals[i] for i in idx] and b["ref_mel_lens"] == [ref_lens[i] for i in idx]
            assert b["mel_shape"] == [len(idx), max(ref_lens[i] for i in idx) + 1, 100]
            assert b["tokens_first"] == convert_char_to_pinyin([texts[idx[0]]])[0]
    assert any(len(b["utts"]) > 1 for b in gold["cases"][1]["batches"])
    for c in gold["pinyin_ascii"]:
        assert convert_char_to_pinyin([c["text"]])[0] == c["tokens"], c["text"]


def test_rank_workers_order_warmup_and_errors():
    """eval_infer_batch.RankWorkers (the in-rank thread pool of the eval driver and of bench.py's C4 / concurrent legs):
    results come back in input order, every item runs exactly once, warm() runs the whole list on EVERY worker thread,
    the threads persist between calls (the samplers key their loop states by thread), an exception is re-raised."""
    import threading
    import time as _t
    from f5e_tts_amd.eval.eval_infer_batch import RankWorkers, run_sharded
    seen, lock = [], threading.Lock()

    def fn(x):
        _t.sleep(0.001 * (x % 3))
        with lock:
            seen.append((threading.get_ident(), x))
        return x * x

    with RankWorkers(3) as pool:
        pool.warm(fn, [100, 101], rounds=2)
        warm_threads = {t for t, _ in seen}
        assert len(warm_threads) == 3 and len(seen) == 3 * 2 * 2           # every worker ran both items twice
        assert all(sum(1 for t, x in seen if t == th and x == 100) == 2 for th in warm_threads)
        seen.clear()
        out = pool.map(fn, range(40))
        assert out == [i * i for i in range(40)] and sorted(x for _, x in seen) == list(range(40))
        assert {t for t, _ in seen} <= warm_threads                         # the same threads: their warm state is reused
        with pytest.raises(ZeroDivisionError):
            pool.map(lambda x: 1 // (x - 5), range(10))
    assert RankWorkers(1).map(fn, [3, 4]) == [9, 16]                        # no pool: the caller's thread
    work = [(f"u{i}", 10, 20 + i) for i in range(9)]
    done = []
    res = run_sharded(work, lambda it: done.append(it[0]), 0, 1, None, workers=3)
    assert sorted(done) == sorted(w[0] for w in work) and res["frames"] == sum(w[2] for w in work)


def _gloo_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from f5e_tts_amd.eval.eval_infer_batch import run_sharded
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    work = [(f"utt{i}", 100 + i, 300 + 53 * (i % 7)) for i in range(13)]
    done = []
    res = run_sharded(work, lambda item: done.append(item[0]), rank, world, dist)
    with open(os.path.join(out_dir, f"r{rank}.json"), "w") as f:
        json.dump(dict(done=done, frames=res["frames"], seconds=res["seconds"]), f)
    dist.destroy_process_group()


def test_sharded_driver_world2_gloo(tmp_path):
    import torch.multiprocessing as mp
    port = 29500 + (os.getpid() % 2000)
    mp.spawn(_gloo_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r = [json.load(open(tmp_path / f"r{i}.json")) for i in range(2)]
    all_done = sorted(r[0]["done"] + r[1]["done"])
    assert all_done == sorted(f"utt{i}" for i in range(13)) and not set(r[0]["done"]) & set(r[1]["done"])
    total = sum(300 + 53 * (i % 7) for i in range(13))
    assert r[0]["frames"] == r[1]["frames"] == total                   # SUM all-reduce
    assert r[0]["seconds"] == r[1]["seconds"] > 0                      # MAX all-reduce


def _bench_c4_worker(rank, world, port, out_dir):
    """bench.py --workload C4 minus the GPU: the same work list, LPT partition and job reductions, `one_pass` stubbed."""
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from f5e_tts_amd.eval.eval_infer_batch import c4_work_list, flop_fwd, lpt_partition, reduce_job_totals
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    steps, warmup = 5, 2
    utts = c4_work_list(os.path.join(GOLD, "c4_durations.csv"), world * (steps + warmup))
    mine = [utts[i] for i in lpt_partition([flop_fwd(t) for _, t in utts], world)[rank]]
    timed = mine[warmup:][:steps]
    frames, gen = sum(t for _, t in timed), sum(t - r for r, t in timed)
    red = reduce_job_totals(dist, frames, gen, 0.25 + 0.5 * rank, "cpu")      # stub wall time: rank 1 is the slow one
    with open(os.path.join(out_dir, f"b{rank}.json"), "w") as f:
        json.dump(dict(red, mine=mine, my_frames=frames, my_gen=gen), f)
    dist.destroy_process_group()


def test_bench_c4_partition_and_reductions_world2_gloo(tmp_path):
    """The N > 1 leg of bench.py (C4 stream): every utterance lands on exactly one rank, frame counts are SUM-reduced, the
    wall time MAX-reduced, and the line can show that `world` ranks took part (per-rank records, backend name)."""
    import torch.multiprocessing as mp
    from f5e_tts_amd.eval.eval_infer_batch import c4_work_list
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_bench_c4_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r = [json.load(open(tmp_path / f"b{i}.json")) for i in range(2)]
    utts = c4_work_list(os.path.join(GOLD, "c4_durations.csv"), 14)
    assert sorted(map(tuple, r[0]["mine"] + r[1]["mine"])) == sorted(utts) and len(r[0]["mine"]) == len(r[1]["mine"]) == 7
    for x in r:
        assert x["world_size"] == 2 and x["backend"] == "gloo"
        assert x["frames"] == r[0]["my_frames"] + r[1]["my_frames"] and x["gen_frames"] == r[0]["my_gen"] + r[1]["my_gen"]
        assert x["seconds"] == 0.75 and x["per_rank_seconds"] == [0.25, 0.75]
        assert x["per_rank_frames"] == [r[0]["my_frames"], r[1]["my_frames"]]
    assert all(600 < t <= 2048 and 0 < rr < t for rr, t in utts)


def _run_bench(argv, env_extra=None, launcher=None):
    import subprocess
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    env.update(env_extra or {})
    cmd = (launcher or [sys.executable]) + [os.path.join(ROOT, "bench.py")] + argv
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)


def test_bench_gpus_flag_launches_that_many_ranks():
    """`python bench.py --gpus 2` (no launcher) must BE a two-rank job: it starts torch.distributed.run as a child process
    (reference: `accelerate launch`, eval/eval_infer_batch.sh:4-6) and relays exactly one JSON line whose n_gpus /
    world_size / per-rank records show two ranks; the fixed-total C4 leg splits every utterance onto exactly one rank.
    --stub: gloo and a sleep instead of RCCL and the GPU pass (the launch / partition / reduction code is the same)."""
    pr = _run_bench(["--gpus", "2", "--stub", "--full", "--steps", "4", "--warmup", "1", "--c4-total", "21"])
    assert pr.returncode == 0, pr.stderr[-2000:]
    lines = [ln for ln in pr.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, pr.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == line["world_size"] == 2 and line["backend"] == "gloo" and line["data"] == "stub"
    assert len(line["per_rank_frames"]) == len(line["per_rank_seconds"]) == 2
    assert line["per_rank_frames"][0] == line["per_rank_frames"][1] == 4 * 469          # weak scaling: same work per rank
    c4 = line["scaling_c4"]
    assert c4["scaling"] == "strong" and c4["utterances"] == 21 and sum(c4["per_rank_utterances"]) == 21
    from f5e_tts_amd.eval.eval_infer_batch import c4_work_list
    assert sum(c4["per_rank_frames"]) == sum(t for _, t in c4_work_list(os.path.join(GOLD, "c4_durations.csv"), 21))
    assert abs(c4["per_rank_utterances"][0] - c4["per_rank_utterances"][1]) <= 1


def test_bench_under_the_drivers_launcher_and_world_mismatch():
    """The driver's own form (torch.distributed.run ... bench.py --gpus N) runs the ranks in place -- no second launch --
    and a --gpus that disagrees with WORLD_SIZE is an error, not a silent one-rank run."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    launcher = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                "127.0.0.1", "--master-port", str(port)]
    pr = _run_bench(["--gpus", "2", "--stub", "--steps", "3", "--warmup", "0", "--c4-total", "0"], launcher=launcher)
    assert pr.returncode == 0, pr.stderr[-2000:]
    line = json.loads([ln for ln in pr.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and len(line["per_rank_frames"]) == 2 and line["scaling_c4"] is None
    bad = _run_bench(["--gpus", "4", "--stub"], env_extra={"WORLD_SIZE": "1", "RANK": "0"})
    assert bad.returncode != 0 and "WORLD_SIZE" in (bad.stderr + bad.stdout)


def test_full_size_layouts_match_reference_including_codebook():
    """F5TTS_v1_Base and BASELINE config 5 (Small + PPG + Gumbel codebook) built from this package's yaml files have
    exactly the reference's state_dict names and shapes (tests/golden/layouts.json, written by the reference)."""
    import yaml

    import f5e_tts_amd
    from f5e_tts_amd.model import DiT
    from f5e_tts_amd.train.parse_cfg import parse_model_yaml
    ref = json.load(open(os.path.join(GOLD, "layouts.json")))
    cfgdir = os.path.join(os.path.dirname(os.path.abspath(f5e_tts_amd.__file__)), "configs")
    for tag, name in (("v1_base", "F5TTS_v1_Base"), ("small_ppg_codebook", "F5TTS_Small_PPG")):
        mc = parse_model_yaml(yaml.safe_load(open(os.path.join(cfgdir, name + ".yaml"))))
        m = DiT(**mc["arch"], text_num_embeds=2545, mel_dim=100, ppg_config=mc["transformer_ppg_config"],
                cb_config=mc["transformer_codebook_config"])
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == ref[tag], tag
    assert len(ref["v1_base"]) == 364 and any(k.startswith("quantizer.") for k in ref["small_ppg_codebook"])


def test_mish_closed_form_matches_the_definition():
    """csrc/f5e_common.h mish_f: x tanh(softplus(x)) = x n / (n + 2), n = e (e + 2), e = exp(min(x, 20)); x > 20 -> x
    (torch's softplus threshold, modules.py:167-190 uses nn.Mish).  The algebra is pinned here in fp32 against
    F.mish in fp64; the GPU instruction accuracy is covered by the conv / activation parity tests."""
    x = torch.linspace(-40, 40, 200001, dtype=torch.float32)
    e = torch.exp(torch.clamp(x, max=20.0))
    n = e * (e + 2)
    y = torch.where(x > 20, x, x * (n / (n + 2)))
    ref = torch.nn.functional.mish(x.double())
    err = (y.double() - ref).abs()
    assert bool((err <= 1e-7 + 1e-6 * ref.abs()).all()), float(err.max())



def test_every_environment_switch_is_documented():
    """INTEGRATION.md section D is the one table of F5E_* switches: every variable the sources read must be in it."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pat = re.compile(r'(?:getenv\(|environ\.get\(|environ\[)\s*"(F5E_[A-Z0-9_]+)"')
    used = set()
    for base, _, files in os.walk(os.path.join(root, "f5e-tts_amd")):
        if "build" in base.split(os.sep):
            continue
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                used |= set(pat.findall(open(os.path.join(base, f), errors="ignore").read()))
    used |= set(pat.findall(open(os.path.join(root, "bench.py")).read()))
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    missing = sorted(v for v in used if f"`{v}`" not in doc)
    assert not missing, f"undocumented environment switches: {missing}"
    assert len(used) >= 6


def test_shipped_library_reads_no_environment_variable():
    """include/f5e_abi.h promises no process-wide state: every getenv in csrc/ sits inside an F5E_TOOLS block (diagnostics
    build), and the shipped libf5e_hip.so does not even import getenv."""
    import subprocess
    csrc = os.path.join(ROOT, "f5e-tts_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h")):
            continue
        stack = []          # one entry per open #if: True while inside the F5E_TOOLS branch of an #ifdef F5E_TOOLS
        for ln in open(os.path.join(csrc, f)):
            t = ln.strip()
            if t.startswith("#if"):
                stack.append(t.startswith("#ifdef F5E_TOOLS"))
            elif t.startswith("#else") and stack:
                stack[-1] = False
            elif t.startswith("#endif") and stack:
                stack.pop()
            if "getenv(" in ln and not t.startswith("//"):
                assert any(stack), f"{f}: getenv outside an F5E_TOOLS block: {t}"
    und = subprocess.run(["nm", "-D", "--undefined-only", os.path.join(ROOT, "f5e-tts_amd", "libf5e_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und


def test_library_exports_only_the_declared_c_abi():
    """-fvisibility=hidden + the linker version script: the dynamic symbol table of libf5e_hip.so holds exactly the functions
    f5e_abi.h declares -- no C++-mangled internals, no kernels, no per-unit markers."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "f5e-tts_amd", "libf5e_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip())
    assert exported == declared_functions(), sorted(set(exported) ^ set(declared_functions()))


def test_prof_ops_derive_short_and_long_dispatches():
    """tools/prof_ops.py derive(): on a long dispatch the GRBM quotient is a clock; on a short one (counter window longer than
    the kernel's span) it must be nulled and the span-based lower bound of the matrix pipe's share reported instead."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("prof_ops", os.path.join(ROOT, "tools", "prof_ops.py"))
    po = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(po)
    long_row, short_row = {}, {}
    # 400 us at 2.2 GHz: 880 000 cycles per XCD x 8; matrix pipe 40 % busy on 1024 SIMDs
    c_long = {"GRBM_GUI_ACTIVE": 8 * 880_000.0, "SQ_VALU_MFMA_BUSY_CYCLES": 0.4 * 1024 * 880_000.0,
              "SQ_WAVE_CYCLES": 1e9, "SQ_WAIT_ANY": 4e8}
    po.derive(long_row, c_long, 400.0)
    assert abs(long_row["eff_clock_ghz"] - 2.2) < 1e-3 and abs(long_row["mfma_busy"] - 0.4) < 1e-4
    assert "mfma_busy_span_min" not in long_row and abs(long_row["wave_cycles_parked"] - 0.4) < 1e-4
    # 12 us kernel whose counter window is 1.5 x its span at 2.4 GHz
    win = 12.0e3 * 2.4 * 1.5
    c_short = {"GRBM_GUI_ACTIVE": 8 * win, "SQ_VALU_MFMA_BUSY_CYCLES": 0.2 * 1024 * 12.0e3 * 2.4}
    po.derive(short_row, c_short, 12.0)
    assert short_row["eff_clock_ghz"] is None and abs(short_row["counter_window_over_span"] - 1.5) < 1e-2
    assert abs(short_row["mfma_busy_span_min"] - 0.2) < 1e-4 and abs(short_row["mfma_busy"] - 0.2 / 1.5) < 1e-4


def test_profile_summaries_are_read_back_only_on_matching_kernel_sources(tmp_path, monkeypatch):
    """bench.py carries rocprofv3 / PMC summaries from profiles/ only when they were measured on the kernel sources that run
    (tools/src_hash.py): a summary with another hash is refused with the reason; stale committed ones only warn here."""
    import importlib.util
    from tools.src_hash import csrc_sha256
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    h = csrc_sha256()
    stale_names = [name for name in ("ops_trace_c2", "ops_trace_c3", "ops_pmc_c2", "ops_pmc_c3", "pmc_traffic_c2")
                   if json.load(open(os.path.join(ROOT, "profiles", name + ".json"))).get("csrc_sha256") != h]
    if stale_names:   # mid-round state (kernels changed, profile not re-taken yet): bench.py then emits nulls + the reason
        import warnings
        warnings.warn(f"profiles/{stale_names} were measured on other kernel sources: re-run tools/gpu_profile.sh")
    ops_, note = bench.stamped_ops("ops_trace_c2")
    if not stale_names:
        assert ops_ is not None and set(ops_) >= {"QKV", "ATTN", "OUT", "FF1", "FF2"}
    else:
        assert ops_ is None and "mismatch" in note
    # a summary stamped with another hash is refused, with the reason in the note
    fake_root = tmp_path / "repo"
    (fake_root / "profiles").mkdir(parents=True)
    stale = dict(json.load(open(os.path.join(ROOT, "profiles", "ops_trace_c2.json"))), csrc_sha256="0" * 64)
    (fake_root / "profiles" / "ops_trace_c2.json").write_text(json.dumps(stale))
    monkeypatch.setattr(bench, "ROOT", str(fake_root))
    ops2, note2 = bench.stamped_ops("ops_trace_c2")
    assert ops2 is None and "mismatch" in note2
    ops3, note3 = bench.stamped_ops("ops_trace_c9")
    assert ops3 is None and "no profiles/" in note3


def test_bench_dump_outputs_are_float32_and_a_fixed_sample_past_the_budget(tmp_path, monkeypatch):
    """bench.py --dump-outputs: every array as <name>.npy in float32, whole while the total fits 64 MB; past the budget
    each array is cut to the same fraction by a fixed seed, so two runs write the same elements."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    g = torch.Generator().manual_seed(3)
    arrays = {"mel": torch.randn(2, 50, 100, generator=g), "wave": torch.randn(2, 4000, generator=g).to(torch.bfloat16)}
    shapes = bench.dump_outputs(str(tmp_path / "a"), arrays)
    for k, v in arrays.items():
        a = np.load(str(tmp_path / "a" / f"{k}.npy"))
        assert a.dtype == np.float32 and shapes[k] == [list(v.shape), list(v.shape)]
        assert np.array_equal(a, v.float().numpy())
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 8000)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    bench.dump_outputs(str(tmp_path / "c"), arrays)
    total = 0
    for k, v in arrays.items():
        b, c = np.load(str(tmp_path / "b" / f"{k}.npy")), np.load(str(tmp_path / "c" / f"{k}.npy"))
        assert b.dtype == np.float32 and b.ndim == 1 and 0 < b.size < v.numel() and np.array_equal(b, c)
        assert np.isin(b, v.float().numpy().reshape(-1)).all()
        total += b.nbytes
    assert total <= 8000
