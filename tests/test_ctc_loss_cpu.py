"""CTC transcript scoring and best-of-N synthesis, host side: tests/ctc_loss_ref.py (the restatement of f5e_ctc_loss) against
torch.nn.functional.ctc_loss on the float64 log_softmax and against the reference's own ``CTC.forward``
(tests/golden/ctc_loss.npz, made by tests/golden/make_ctc_loss_golden.py); the two new C-ABI entries are declared, exported
and bound and check their arguments without a GPU; ``ConformerPPG.ctc_loss`` and ``infer_batch_process`` refuse caller bugs
before any device is touched; the selection rule of best-of-N on a stub model, vocoder and scorer; the new command-line
flags.  No kernel is launched here.

Tolerance of every fp32 comparison: |got - ref| <= (4 + T) * 2^-24 * max(1, |ref|) -- one fp32 rounding at the magnitude of
the running value per frame, plus the closing logaddexp and the normaliser (``ctc_loss_ref.tolerance``)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import ctc_loss_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def labels_with_repeats(L, V, seed, repeats=0):
    """L ids in [1, V), neighbours distinct except for ``repeats`` planted adjacent pairs."""
    rng = np.random.default_rng(seed)
    lab = np.zeros(L, np.int64)
    for i in range(L):
        v = int(rng.integers(1, V))
        while i > 0 and v == lab[i - 1]:
            v = int(rng.integers(1, V))
        lab[i] = v
    for k in range(repeats):
        i = 1 + (k * 7) % max(1, L - 1)
        lab[i] = lab[i - 1]
    return lab


def n_repeats(lab):
    lab = np.asarray(lab)
    return int((lab[1:] == lab[:-1]).sum())


def check_against_torch(scores, lab):
    """fp32 restatement within the tolerance of float64 torch; float64 restatement to 1e-9 relative."""
    T = scores.shape[0]
    want = LR.torch_logp(scores[None], np.asarray(lab, np.int64)[None] if len(lab) else np.zeros((1, 0), np.int64), [T],
                         [len(lab)])[0]
    got32 = float(LR.loss_one(scores, lab, dtype=np.float32))
    got64 = float(LR.loss_one(scores, lab, dtype=np.float64))
    if np.isneginf(want):
        assert np.isneginf(got32) and np.isneginf(got64)
        return want
    assert math.isfinite(want)
    assert abs(got64 - want) <= 1e-9 * max(1.0, abs(want)), (got64, want)
    tol = LR.tolerance(T, want)
    print(f"T={T} L={len(lab)} V={scores.shape[1]}: ref {want:.6f} fp32 error {abs(got32 - want):.3e} = "
          f"{100 * abs(got32 - want) / tol:.1f}% of the bound")
    assert abs(got32 - want) <= tol, (got32, want, tol)
    return want


# ------------------------------------------------------------------ the restatement against torch

@pytest.mark.parametrize("T,V,L,repeats", [(1, 5, 0, 0), (40, 12, 7, 0), (64, 20, 31, 2), (200, 50, 63, 0), (300, 218, 127, 0),
                                           (600, 4233, 255, 0), (2000, 218, 256, 0)])
def test_restatement_equals_torch_ctc_loss(T, V, L, repeats):
    rng = np.random.default_rng(1000 + T)
    lab = labels_with_repeats(L, V, 2000 + T, repeats)
    assert n_repeats(lab) >= repeats
    scores = (2.0 * rng.standard_normal((T, V))).astype(np.float32)
    want = check_against_torch(scores, lab)
    assert math.isfinite(want)
    # raw logits and their log_softmax are the same input
    lp = torch.log_softmax(torch.from_numpy(scores).double(), -1).numpy().astype(np.float32)
    assert abs(float(LR.loss_one(lp, lab)) - want) <= LR.tolerance(T, want)


def test_restatement_single_path_and_one_frame_too_few():
    V = 9
    rng = np.random.default_rng(31)
    for lab in ([3, 3, 4, 4, 4, 1], [2, 5, 7], [6, 6]):
        T = len(lab) + n_repeats(lab)
        scores = rng.standard_normal((T, V)).astype(np.float32)
        want = check_against_torch(scores, lab)
        # exactly one path: every label once, a blank between equal neighbours -> the sum of its log-probabilities
        path = []
        for i, y in enumerate(lab):
            if i and y == lab[i - 1]:
                path.append(0)
            path.append(y)
        lp = torch.log_softmax(torch.from_numpy(scores).double(), -1).numpy()
        assert abs(float(lp[np.arange(T), path].sum()) - want) <= 1e-9 * abs(want)
        # one frame too few: no path, -inf against torch's +inf
        short = check_against_torch(scores[:T - 1], lab) if T > 1 else -np.inf
        assert np.isneginf(short)
    assert np.isneginf(LR.loss_one(np.zeros((4, V), np.float32), [1, V]))          # a label that is no class
    assert np.isneginf(LR.loss(np.zeros((1, 4, V), np.float32), np.ones((1, 2), np.int64), [5], [2])[0])   # t_len > T
    assert np.isneginf(LR.loss(np.zeros((1, 4, V), np.float32), np.ones((1, 2), np.int64), [4], [3])[0])   # l_len > L


def test_restatement_empty_transcript_is_the_all_blank_path():
    rng = np.random.default_rng(5)
    scores = rng.standard_normal((17, 6)).astype(np.float32)
    want = check_against_torch(scores, [])
    lp = torch.log_softmax(torch.from_numpy(scores).double(), -1).numpy()
    assert abs(float(lp[:, 0].sum()) - want) <= 1e-12 * abs(want)


def test_restatement_true_minus_infinity_that_still_leaves_a_path():
    rng = np.random.default_rng(77)
    T, V, lab = 30, 8, [1, 2, 2, 5]
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((T, V))).double(), -1).numpy().astype(np.float32)
    lp[::3, 3] = -np.inf                         # a class no label uses
    lp[:4, 5] = -np.inf                          # the last label cannot start early
    lp[10, 0] = -np.inf                          # one frame cannot be blank
    want = check_against_torch(lp, lab)
    assert math.isfinite(want)
    lp2 = lp.copy()
    lp2[12, :] = -np.inf                         # a frame nothing can pass: no NaN, the sum of no paths
    assert np.isneginf(LR.loss_one(lp2, lab)) and np.isneginf(LR.loss_one(lp2, lab, dtype=np.float64))
    lp3 = lp.copy()
    lp3[:, 2] = -np.inf                          # a label that can never be emitted
    assert np.isneginf(check_against_torch(lp3, lab))


def test_restatement_reproduces_the_reference_ctc_forward():
    z = np.load(os.path.join(GOLD, "ctc_loss.npz"))
    W, bias = z["ctc_lo_weight"].astype(np.float64), z["ctc_lo_bias"].astype(np.float64)
    sizes = set()
    for i in range(int(z["n_cases"])):
        hs, hl, ys, yl = z[f"hs_pad_{i}"], z[f"hlens_{i}"], z[f"ys_pad_{i}"], z[f"ys_lens_{i}"]
        B, T = hs.shape[:2]
        sizes.add(B)
        assert (ys[np.arange(ys.shape[1])[None] >= yl[:, None]] == -1).all()          # the reference's padding
        logits = hs.astype(np.float64) @ W.T + bias
        for dtype in (np.float64, np.float32):
            nll = -LR.loss(logits.astype(dtype), ys, hl, yl, dtype=dtype).astype(np.float64)
            for b in range(B):
                tol = LR.tolerance(int(hl[b]), z[f"per_utt_{i}"][b]) + 2.0 ** -23 * abs(z[f"per_utt_{i}"][b])   # + the fixture's fp32
                assert abs(nll[b] - z[f"per_utt_{i}"][b]) <= tol
            assert abs(nll.sum() / B - float(z[f"loss_{i}"])) <= sum(LR.tolerance(int(t), v) for t, v in
                                                                     zip(hl, z[f"per_utt_{i}"])) / B + 2.0 ** -23 * float(z[f"loss_{i}"])
    assert sizes == {1, 3}


# ------------------------------------------------------------------ the C ABI without a device

ENTRIES = [("f5e_ctc_loss_workspace_bytes", 3), ("f5e_ctc_loss", 16)]


def test_new_entries_are_declared_exported_and_bound():
    from f5e_tts_amd import _C
    text = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    lib = _C.lib()
    for name, arity in ENTRIES:
        m = re.search(r"F5E_API int " + name + r"\((.*?)\);", text, flags=re.S)
        assert m, f"{name} is not declared in f5e_abi.h"
        assert len(m.group(1).split(",")) == arity == len(_C.SIGNATURES[name])
        assert hasattr(lib, name)
    assert "f5e_*" in open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "exports.map")).read()
    assert lib.f5e_abi_version() == _C.ABI_VERSION == 2


def on_own_thread(fn):
    """f5e_last_error is thread-local and nothing clears it: the calls that are MEANT to fail run on a thread of their own."""
    import threading
    box = []

    def run():
        try:
            fn()
        except BaseException as e:      # noqa: BLE001 -- handed to the caller's thread
            box.append(e)
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if box:
        raise box[0]


def test_workspace_query_and_every_argument_check_without_launching():
    on_own_thread(_argument_checks)


def _argument_checks():
    from f5e_tts_amd import _C, ops
    lib = _C.lib()
    assert ops.ctc_loss_workspace_bytes(1, 300) == 300 * 4
    assert ops.ctc_loss_workspace_bytes(4, 16384) == 4 * 16384 * 4
    n = C.c_ulonglong()
    assert lib.f5e_ctc_loss_workspace_bytes(1, 16385, C.byref(n)) == -1 and b"16384" in lib.f5e_last_error()
    assert lib.f5e_ctc_loss_workspace_bytes(0, 16, C.byref(n)) == -1 and lib.f5e_ctc_loss_workspace_bytes(1, 16, None) == -1
    p, big = C.c_void_p(8), 10 ** 9

    def loss(scores=p, bs=0, ld=50, labels=p, ldl=10, t=p, l=p, blank=0, out=p, ws=p, wsb=big, B=1, T=100, L=10, V=50):
        return lib.f5e_ctc_loss(None, scores, bs, ld, labels, ldl, t, l, blank, out, ws, wsb, B, T, L, V)

    for bad in (dict(scores=None), dict(labels=None), dict(t=None), dict(l=None), dict(out=None), dict(ws=None)):
        assert loss(**bad) == -1 and b"null" in lib.f5e_last_error()
    assert loss(V=1, ld=1) == -1 and b"V >= 2" in lib.f5e_last_error()
    assert loss(blank=50) == -1 and loss(blank=-1) == -1
    assert loss(ld=49) == -1 and b"ld" in lib.f5e_last_error()
    assert loss(ldl=9) == -1
    assert loss(B=2, bs=99 * 50 + 49) == -1 and b"batch_stride" in lib.f5e_last_error()
    assert loss(wsb=100 * 4 - 1) == -1 and b"workspace" in lib.f5e_last_error()
    assert loss(ws=C.c_void_p(6)) == -1 and b"aligned" in lib.f5e_last_error()
    assert loss(L=2048, ldl=2048) == -1 and b"2047" in lib.f5e_last_error()
    assert loss(L=-1) == -1
    assert loss(T=16385) == -1 and b"16384" in lib.f5e_last_error()
    assert loss(T=0) == -1 and loss(B=0) == -1 and loss(B=65536, bs=10 ** 6, wsb=10 ** 12) == -1


def test_wrapper_has_no_cpu_path():
    from f5e_tts_amd import _C, ops
    i32 = torch.int32
    lab, t, l = torch.ones(1, 2, dtype=i32), torch.tensor([8], dtype=i32), torch.tensor([2], dtype=i32)
    for scores in (torch.zeros(1, 8, 5), torch.zeros(8, 5), torch.zeros(1, 8, 5, dtype=torch.float64),
                   torch.zeros(1, 8, 10)[:, :, ::2], torch.empty(1, 8, 5, device="meta")):
        with pytest.raises(_C.F5EError, match="ctc_loss: scores must be an f32 GPU tensor .* there is no CPU path"):
            ops.ctc_loss(scores, lab, t, l)


# ------------------------------------------------------------------ ConformerPPG.ctc_loss: caller bugs

def test_model_ctc_loss_refuses_caller_bugs_before_the_device():
    from f5e_tts_amd import _C
    from f5e_tts_amd.ppg.ppg_model import ConformerPPG, check_ctc_loss_lengths
    kw = dict(input_dim=80, vocab_size=40, output_size=64, attention_heads=4, linear_units=128, num_blocks=1)
    plain, m = ConformerPPG(**kw), ConformerPPG(**kw, ctc=True)            # both on the CPU: nothing below may reach the engine
    feats, lens = torch.zeros(2, 30, 80), torch.tensor([30, 22])
    with pytest.raises(_C.F5EError, match="CTC head"):
        plain.ctc_loss(feats, lens, [[1, 2], [3]])
    with pytest.raises(_C.F5EError, match="batch of 2"):
        m.ctc_loss(feats, lens, [[1, 2]])                                  # one row for two utterances
    with pytest.raises(_C.F5EError, match="batch of 2"):
        m.ctc_loss(feats, lens, torch.ones(2, 3, dtype=torch.int32), [3])  # one length for two rows
    with pytest.raises(_C.F5EError, match="batch of 2"):
        m.ctc_loss(feats, lens, torch.ones(2, dtype=torch.int32))          # not [B, L]
    with pytest.raises(_C.F5EError, match="label ids"):
        m.ctc_loss(feats, lens, [[1, 40], [3]])                            # id = vocab
    with pytest.raises(_C.F5EError, match="label ids"):
        m.ctc_loss(feats, lens, torch.tensor([[1, -1], [3, 2]]), [2, 1])   # padding counted as a label
    with pytest.raises(_C.F5EError, match="no CTC path"):
        m.ctc_loss(feats, lens, torch.ones(2, 3, dtype=torch.int32), [3, 4])   # longer than the buffer
    with pytest.raises(_C.F5EError, match="no CTC path"):
        m.ctc_loss(feats, lens, [[1], [2]], [1, -1])
    with pytest.raises(_C.F5EError, match=r"text_lengths\[1\] = 2 exceeds the 1 ids"):
        m.ctc_loss(feats, lens, [[1, 2, 3], [2]], [3, 2])                  # the padding is the blank id, never a label
    # what may pass: repeats, an empty transcript, -1 padding past the length; and the frame rule
    check_ctc_loss_lengths([[1, 1, 2], [-1, -1, -1]], [3, 0], [4, 1], 3, vocab=40)
    check_ctc_loss_lengths(None, [3, 0], None, 3)
    for labels, l, t in (([[1, 1, 2]], [3], [3]), ([[]], [0], [0]), ([[5, 6]], [2], [1])):
        with pytest.raises(_C.F5EError, match="no CTC path"):
            check_ctc_loss_lengths(labels, l, t, max(1, len(labels[0])), vocab=40)
    assert "gradient" in ConformerPPG.ctc_loss.__doc__


# ------------------------------------------------------------------ best-of-N: the selection rule on stubs

class Model:
    """``sample`` returns a mel filled with the seed, so the vocoder stub's wave says which candidate it is."""

    def __init__(self):
        self.calls = []

    def sample(self, **kw):
        self.calls.append(kw)
        fill = -1.0 if kw["seed"] is None else float(kw["seed"])
        return torch.full((1, kw["duration"], 100), fill), None


class Voc:
    def decode(self, mel):
        return mel[:, 0, :1].expand(1, 256 * (mel.shape[-1] - 1)).clone()


class Scorer:
    def __init__(self, planted):
        self.planted, self.calls = list(planted), []

    def score_batch(self, waves, sr, text):
        self.calls.append((waves.clone(), sr, text))
        return torch.tensor(self.planted.pop(0), dtype=torch.float32)


def run(gens, **kw):
    from f5e_tts_amd.infer import utils_infer as U
    g = torch.Generator().manual_seed(3)
    audio = 0.5 * torch.randn(1, 24000, generator=g)                      # rms above target_rms: no rescaling of the output
    m = Model()
    wave, sr, spec = next(U.infer_batch_process((audio, 24000), "A reference text. ", gens, m, Voc(), cross_fade_duration=0.0,
                                                device="cpu", **kw))
    return wave, m


def test_best_of_refuses_caller_bugs_before_the_model_is_called():
    for kw in (dict(best_of=0), dict(best_of=-3), dict(best_of=2), dict(best_of=2, scorer=object())):
        from f5e_tts_amd.infer import utils_infer as U
        m = Model()
        with pytest.raises(ValueError, match="best_of"):
            next(U.infer_batch_process((torch.randn(1, 24000), 24000), "Ref. ", ["Some text to say."], m, Voc(), device="cpu", **kw))
        assert m.calls == []


@pytest.mark.parametrize("planted,chosen", [
    ([1.0, 5.0, 5.0, 2.0], 1),                                             # the first maximum
    ([float("nan"), -float("inf"), -9.0, float("nan")], 2),                # NaN and -inf rank last
    ([-float("inf"), float("nan"), -float("inf"), float("nan")], 0),       # nothing finite: candidate 0
    ([float("inf"), 3.0, 2.0, 1.0], 1),                                    # +inf is not a likelihood either
    ([-4.0, -5.0, -6.0, -7.0], 0),
])
def test_selection_rule(planted, chosen):
    from f5e_tts_amd.infer.utils_infer import pick_best
    assert pick_best(planted) == chosen
    report, sc = [], Scorer([planted])
    wave, m = run(["Some text to say."], best_of=4, scorer=sc, seed=40, report=report)
    assert [c["seed"] for c in m.calls] == [40, 41, 42, 43]
    assert len(sc.calls) == 1 and sc.calls[0][1] == 24000 and sc.calls[0][2] == "Some text to say."
    stack = sc.calls[0][0]
    assert stack.shape[0] == 4 and stack.ndim == 2 and [float(r[0]) for r in stack] == [40.0, 41.0, 42.0, 43.0]
    assert (wave == 40.0 + chosen).all()
    assert len(report) == 1 and report[0]["seeds"] == [40, 41, 42, 43] and report[0]["chosen"] == chosen
    assert all(a == b or (math.isnan(a) and math.isnan(b)) for a, b in zip(report[0]["scores"], planted))


def test_two_chunks_are_scored_against_their_own_text_with_the_seed_formula():
    gens = ["The first chunk of text.", "And the second one."]
    report, sc = [], Scorer([[0.0, 1.0, -1.0], [2.0, 0.5, 0.1]])
    wave, m = run(gens, best_of=3, scorer=sc, seed=7, report=report)
    assert [c["seed"] for c in m.calls] == [7, 8, 9, 10, 11, 12]          # seed + c * best_of + i
    assert [c[2] for c in sc.calls] == gens
    assert [r["seeds"] for r in report] == [[7, 8, 9], [10, 11, 12]] and [r["chosen"] for r in report] == [1, 0]
    durs = [m.calls[0]["duration"], m.calls[3]["duration"]]
    ref_len = 24000 // 256
    n0 = 256 * (durs[0] - ref_len - 1)
    assert (wave[:n0] == 8.0).all() and (wave[n0:] == 10.0).all() and len(wave) == n0 + 256 * (durs[1] - ref_len - 1)
    # streaming: the same choice, chunk by chunk
    from f5e_tts_amd.infer import utils_infer as U
    sc2, m2 = Scorer([[0.0, 1.0, -1.0], [2.0, 0.5, 0.1]]), Model()
    g = torch.Generator().manual_seed(3)
    audio = 0.5 * torch.randn(1, 24000, generator=g)
    pieces = [p for p, _ in U.infer_batch_process((audio, 24000), "A reference text. ", gens, m2, Voc(), device="cpu",
                                                  streaming=True, chunk_size=4096, best_of=3, scorer=sc2, seed=7)]
    assert np.array_equal(np.concatenate(pieces), wave) and [c["seed"] for c in m2.calls] == [7, 8, 9, 10, 11, 12]


def test_unseeded_candidates_draw_from_the_global_generator_in_order():
    torch.manual_seed(123)
    want = [int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) for _ in range(4)]
    torch.manual_seed(123)
    report = []
    _, m = run(["One chunk.", "Two chunks."], best_of=2, scorer=Scorer([[0.0, 1.0], [1.0, 0.0]]), report=report)
    assert [c["seed"] for c in m.calls] == want and [r["seeds"] for r in report] == [want[:2], want[2:]]


def test_best_of_one_is_the_call_that_exists():
    gens = ["The first chunk of text.", "And the second one."]
    w0, m0 = run(gens)
    w1, m1 = run(gens, best_of=1, scorer=None, seed=None, report=None)
    assert np.array_equal(w0, w1) and m0.calls.__len__() == m1.calls.__len__() == 2
    for a, b in zip(m0.calls, m1.calls):
        assert a.keys() == b.keys() and a["seed"] is None and b["seed"] is None and a["duration"] == b["duration"]
    # a seed alone: one seeded call per chunk, no scorer needed
    report = []
    w2, m2 = run(gens, seed=5, report=report)
    assert [c["seed"] for c in m2.calls] == [5, 6] and [r["seeds"] for r in report] == [[5], [6]]


# ------------------------------------------------------------------ the command line

def test_parser_accepts_the_new_flags_and_refuses_best_of_without_an_asr_model():
    from f5e_tts_amd.infer import infer_cli
    p = infer_cli.build_parser()
    a = p.parse_args([])
    assert a.best_of == 1 and a.seed is None and a.asr_model is None and a.asr_config is None and a.asr_dict is None
    infer_cli.require_scorer_args(a)
    a = p.parse_args(["--best_of", "4", "--seed", "11", "--asr_model", "m.pt", "--asr_config", "t.yaml", "--asr_dict", "d.txt"])
    assert (a.best_of, a.seed, a.asr_model, a.asr_config, a.asr_dict) == (4, 11, "m.pt", "t.yaml", "d.txt")
    infer_cli.require_scorer_args(a)
    with pytest.raises(SystemExit, match="--asr_config, --asr_dict missing"):
        infer_cli.require_scorer_args(p.parse_args(["--best_of", "2", "--asr_model", "m.pt"]))
    with pytest.raises(SystemExit, match="at least 1"):
        infer_cli.require_scorer_args(p.parse_args(["--best_of", "0"]))
    with pytest.raises(SystemExit, match="--asr_model"):
        infer_cli.main(["--best_of", "2"])                                 # before anything is loaded
    # two [voice] segments never share a seed: 3 chunks at best_of 4 from seed 10 use 10 .. 21
    assert infer_cli.next_segment_seed(10, 3, 4) == 22 and infer_cli.next_segment_seed(5, 2, 1) == 7
