"""CTC decoding and the speech-editing driver, host side: tests/ctc_ref.py equals the reference's own ``forced_align`` and
``ctc_greedy_search`` on the fixtures of tests/golden/make_ctc_golden.py; the new C-ABI entries are declared, exported, bound
and validate their arguments without a GPU; ``plan_edit`` equals a literal restatement of the reference's recipe; the diff ->
parts mapping, the tokeniser and ``frames_timestamp``; ``ConformerPPG`` keeps its state_dict.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ctc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")


# ------------------------------------------------------------------ the restatement against the reference's outputs

def test_restatement_equals_every_reference_alignment():
    z = np.load(os.path.join(GOLD, "ctc_align.npz"))
    n = int(z["n_cases"])
    assert n >= 5
    seen = set()
    for i in range(n):
        logp, labels, want = z[f"logp_{i}"], z[f"labels_{i}"], z[f"align_{i}"]
        T = logp.shape[0]
        al, states, start, stop, score = R.align_one(logp, labels)
        assert np.array_equal(al, want)
        assert R.is_ctc_path(al, labels) and (stop > start).all() and (start[1:] >= stop[:-1]).all()
        assert np.isclose(R.path_score(logp, al), float(score), rtol=1e-5)
        # batched form, padded: the same rows, -1 past the length
        pad = np.zeros((1, T + 3, logp.shape[1]), np.float32)
        pad[0, :T] = logp
        lab = np.zeros((1, len(labels) + 2), np.int32)
        lab[0, :len(labels)] = labels
        a2, s2, e2, sc2 = R.align(pad, lab, [T], [len(labels)])
        assert np.array_equal(a2[0, :T], want) and (a2[0, T:] == -1).all() and sc2[0] == score
        assert np.array_equal(s2[0, :len(labels)], start) and (e2[0, len(labels):] == 0).all()
        seen |= {"repeat"} if (labels[1:] == labels[:-1]).any() else set()
        seen |= {"single"} if len(labels) == 1 else set()
        seen |= {"tight"} if T <= 2 * len(labels) + 1 else set()
    assert seen == {"repeat", "single", "tight"}


def test_restatement_degenerate_sequences_and_ties():
    sc = np.zeros((4, 9, 5), np.float32)
    lab = np.array([[1, 2, 3], [1, 1, 1], [1, 2, 7], [1, 2, 3]], np.int32)
    al, ts, te, score = R.align(sc, lab, [9, 4, 9, 10], [3, 3, 3, 0])
    # a constant matrix is all ties: stay wins every comparison and the end state is the last blank, so the backtrack stays
    # there for as long as that state was reachable (t >= 3: 1 -> 3 -> 5 -> 6, all label-to-label skips) and then must move
    assert al[0].tolist() == [1, 2, 3, 0, 0, 0, 0, 0, 0] and score[0] == 0.0
    assert ts[0].tolist() == [0, 1, 2] and te[0].tolist() == [1, 2, 3]
    for b in (1, 2, 3):       # 3 equal labels need 5 frames; a label outside [0, V); lengths beyond the buffer / l = 0
        assert (al[b] == -1).all() and (ts[b] == 0).all() and (te[b] == 0).all() and score[b] == -np.inf


def test_restatement_equals_the_reference_greedy_search():
    z = np.load(os.path.join(GOLD, "ctc_asr.npz"))
    logp, enc_len = z["logp"], z["enc_len"]
    V = logp.shape[-1]
    hyps, frame_logp = R.greedy(logp, enc_len, blank=0, pad_id=V - 1)
    want = [z["hyps"][b, :n].tolist() for b, n in enumerate(z["hyp_len"])]
    assert hyps == want and want[1][-1] == V - 1 and enc_len[1] < logp.shape[1]        # the eos tail of the shorter utterance
    assert np.allclose(frame_logp.max(1), z["scores"][:, 0], rtol=1e-5, atol=1e-6)
    no_pad, _ = R.greedy(logp, enc_len, blank=0, pad_id=-1)
    assert no_pad[0] == want[0] and no_pad[1] == want[1][:-1]
    # the stored log-probs are the stored head applied to the stored encoder output
    logits = z["encoder_out"] @ z["w/ctc.ctc_lo.weight"].T + z["w/ctc.ctc_lo.bias"]
    assert np.allclose(R.log_softmax(logits), logp, atol=2e-5)


# ------------------------------------------------------------------ the C ABI

ENTRIES = (("f5e_ctc_align", 19), ("f5e_ctc_align_workspace_bytes", 4), ("f5e_ctc_greedy", 13))


def test_new_entries_are_declared_exported_and_bound():
    from f5e_tts_amd import _C
    text = open(os.path.join(ROOT, "include", "f5e_abi.h")).read()
    lib = _C.lib()
    for name, arity in ENTRIES:
        m = re.search(r"F5E_API int " + name + r"\((.*?)\);", text, flags=re.S)
        assert m, f"{name} is not declared in f5e_abi.h"
        assert len(m.group(1).split(",")) == arity == len(_C.SIGNATURES[name])
        assert hasattr(lib, name)
    assert lib.f5e_abi_version() == _C.ABI_VERSION == 2
    assert "ctc.hip" in open(os.path.join(ROOT, "f5e-tts_amd", "csrc", "Makefile")).read()


def on_own_thread(fn):
    """f5e_last_error is thread-local and nothing clears it: the calls that are MEANT to fail run on a thread of their own, so
    this thread's record stays what the other host tests expect."""
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
    assert ops.ctc_align_workspace_bytes(1, 300, 60) == 300 * 2 * 16          # S = 121 states: two word pairs per row
    assert ops.ctc_align_workspace_bytes(16, 1500, 300) == 16 * 1500 * 10 * 16
    assert ops.ctc_align_workspace_bytes(1, 16384, 2047) == 16384 * 64 * 16
    n = C.c_ulonglong()
    assert lib.f5e_ctc_align_workspace_bytes(1, 16, 2048, C.byref(n)) == -1 and b"2047" in lib.f5e_last_error()
    assert lib.f5e_ctc_align_workspace_bytes(1, 16385, 10, C.byref(n)) == -1 and b"16384" in lib.f5e_last_error()
    assert lib.f5e_ctc_align_workspace_bytes(1, 16, 10, None) == -1
    p, big = C.c_void_p(8), 10 ** 9

    def align(scores=p, bs=0, ld=50, labels=p, ldl=10, t=p, l=p, blank=0, out=p, ws=p, wsb=big, B=1, T=100, L=10, V=50):
        return lib.f5e_ctc_align(None, scores, bs, ld, labels, ldl, t, l, blank, out, None, None, None, ws, wsb, B, T, L, V)

    for bad in (dict(scores=None), dict(labels=None), dict(t=None), dict(l=None), dict(out=None), dict(ws=None)):
        assert align(**bad) == -1 and b"null" in lib.f5e_last_error()
    assert align(V=1, ld=1) == -1 and b"V >= 2" in lib.f5e_last_error()
    assert align(blank=50) == -1 and align(blank=-1) == -1
    assert align(ld=49) == -1 and b"ld" in lib.f5e_last_error()
    assert align(ldl=9) == -1
    assert align(B=2, bs=99 * 50 + 49) == -1 and b"batch_stride" in lib.f5e_last_error()      # overlapping batch stride
    assert align(wsb=100 * 1 * 16 - 1) == -1 and b"workspace" in lib.f5e_last_error()         # too small
    assert align(ws=C.c_void_p(12)) == -1 and b"aligned" in lib.f5e_last_error()              # misaligned
    assert align(L=2048, ldl=2048) == -1 and b"2047" in lib.f5e_last_error()
    assert align(T=16385) == -1 and b"16384" in lib.f5e_last_error()
    assert align(T=0) == -1 and align(B=0) == -1

    def greedy(scores=p, bs=0, ld=50, t=p, blank=0, pad=-1, hyp=p, hl=p, B=1, T=100, V=50):
        return lib.f5e_ctc_greedy(None, scores, bs, ld, t, blank, pad, hyp, hl, None, B, T, V)

    for bad in (dict(scores=None), dict(t=None), dict(hyp=None), dict(hl=None)):
        assert greedy(**bad) == -1 and b"null" in lib.f5e_last_error()
    assert greedy(V=1, ld=1) == -1 and greedy(blank=50) == -1 and greedy(pad=50) == -1 and greedy(pad=-2) == -1
    assert greedy(ld=49) == -1 and greedy(B=2, bs=99 * 50 + 49) == -1
    assert greedy(T=16385) == -1 and b"16384" in lib.f5e_last_error()


def test_wrappers_check_their_tensors_before_anything_else():
    """Device, dtype and stride of the operands are checked before the device is asked for: the messages are the wrappers'."""
    from f5e_tts_amd import _C, ops
    i32 = torch.int32
    lab, t, l = torch.ones(1, 2, dtype=i32), torch.tensor([8], dtype=i32), torch.tensor([2], dtype=i32)
    for scores in (torch.zeros(1, 8, 5), torch.zeros(8, 5), torch.zeros(1, 8, 5, dtype=torch.float64),
                   torch.zeros(1, 8, 10)[:, :, ::2]):
        with pytest.raises(_C.F5EError, match="ctc_align: scores must be an f32 GPU tensor"):
            ops.ctc_align(scores, lab, t, l)
        with pytest.raises(_C.F5EError, match="ctc_greedy: scores must be an f32 GPU tensor"):
            ops.ctc_greedy(scores, t)
    meta = torch.empty(1, 8, 5, device="meta")               # not a GPU tensor either
    with pytest.raises(_C.F5EError, match="scores must be"):
        ops.ctc_align(meta, lab, t, l)


# ------------------------------------------------------------------ plan_edit against the reference recipe

@pytest.mark.parametrize("fix", [[1.2, 1], None])
@pytest.mark.parametrize("n", [24000 * 6, 24000 * 5 + 1234])
def test_plan_edit_equals_the_reference_recipe(fix, n):
    from f5e_tts_amd.infer import speech_edit as SE
    parts = [[1.42, 2.44], [4.04, 4.9]]
    audio = torch.randn(1, n, generator=torch.Generator().manual_seed(9))
    want_audio, want_mask = R.speech_edit_recipe(audio, 24000, 256, parts, fix)
    pieces, mask = SE.plan_edit(n, 24000, 256, parts, fix)
    assert torch.equal(SE.assemble(audio, pieces), want_audio)
    assert mask == want_mask[0].tolist() and len(mask) == want_audio.shape[-1] // 256 + 1
    assert fix is None or fix == [1.2, 1]                           # the caller's list is not consumed
    assert sum(1 for m in mask if not m) == sum(round((f if fix else e - s) * 24000 / 256)
                                                 for f, (s, e) in zip(fix or [0, 0], parts))


def test_plan_edit_rejects_a_short_fix_duration():
    from f5e_tts_amd.infer import speech_edit as SE
    with pytest.raises(ValueError):
        SE.plan_edit(24000, 24000, 256, [[0.1, 0.2], [0.5, 0.6]], [0.3])


# ------------------------------------------------------------------ diff -> parts

def spans_of(words, t0=0.5, each=0.4):
    from f5e_tts_amd.ppg.ctc_align import WordSpan
    return [WordSpan(w, t0 + i * each, t0 + (i + 1) * each) for i, w in enumerate(words)]


def test_diff_maps_replace_delete_and_insert_to_parts():
    from f5e_tts_amd.infer import speech_edit as SE
    from f5e_tts_amd.ppg.ctc_align import split_words
    origin = split_words("Some call me nature, others call me mother nature.")
    spans = spans_of(origin)
    parts, fix = SE.diff_parts(spans, split_words("Some call me optimist, others call me realist."))
    assert fix is None and len(parts) == 2
    assert parts[0] == [spans[3].start_s, spans[3].end_s]                      # nature, -> optimist,
    assert parts[1] == [spans[7].start_s, spans[8].end_s]                      # mother nature. -> realist.
    parts, fix = SE.diff_parts(spans, split_words("Some call me optimist, others call me realist."), [1.2, 1])
    assert fix == [1.2, 1] and len(parts) == 2
    parts, _ = SE.diff_parts(spans, split_words("Some call me nature, others call me nature."))   # a deletion
    assert parts == [[spans[7].start_s, spans[7].end_s]]
    target = split_words("Some call me dear nature, others call me mother nature.")               # a pure insertion
    with pytest.raises(ValueError, match="fix_duration"):
        SE.diff_parts(spans, target)
    parts, fix = SE.diff_parts(spans, target, [0.5])
    assert parts == [[spans[3].start_s, spans[3].start_s]] and fix == [0.5]
    parts, _ = SE.diff_parts(spans, origin + ["indeed"], [0.7])                                    # appended at the end
    assert parts == [[spans[-1].end_s, spans[-1].end_s]]
    with pytest.raises(ValueError):
        SE.diff_parts(spans, target, [0.5, 0.5])
    assert SE.diff_parts(spans, origin) == ([], None)


def test_speech_edit_needs_parts_or_an_aligner():
    from f5e_tts_amd.infer import speech_edit as SE

    class NoModel:
        def parameters(self):
            return iter([torch.zeros(1)])
    with pytest.raises(ValueError, match="aligner"):
        SE.speech_edit_process((torch.zeros(1, 2400), 24000), "a b", "a c", NoModel(), None)
    args = SE.build_parser().parse_args(["--audio", "a.wav", "--origin_text", "x", "--target_text", "y", "-p", "m.pt",
                                         "--parts", "1.42-2.44,4.04-4.9", "--fix_duration", "1.2,1"])
    assert SE._pairs(args.parts) == [[1.42, 2.44], [4.04, 4.9]] and args.output.endswith(".wav")


# ------------------------------------------------------------------ tokeniser, symbol table, timestamps

def test_symbol_table_and_default_tokeniser(tmp_path):
    from f5e_tts_amd.ppg import ctc_align as CA
    path = tmp_path / "words.txt"
    path.write_text("<blank> 0\n<unk> 1\na 2\nb 3\nC 4\n你 5\n好 6\n' 7\n<sos/eos> 8\n", encoding="utf8")
    table = CA.read_symbol_table(str(path))
    assert table["<blank>"] == 0 and table["好"] == 6 and len(table) == 9
    words, ids = CA.default_tokenize("Ab  c你好 a'b", table)
    assert words == ["Ab", "c", "你", "好", "a'b"]
    assert ids == [[2, 3], [4], [5], [6], [2, 7, 3]]                 # as-is, lower-cased, upper-cased
    assert CA.default_tokenize("z", table)[1] == [[1]]               # <unk>
    del table["<unk>"]
    words, ids = CA.default_tokenize("az ?? b", table)
    assert words == ["az", "??", "b"] and ids == [[2], [], [3]]      # dropped characters; a word left with no tokens
    spans = CA.word_spans(words, ids, [4, 9], 12, frame_s=0.02)
    assert [tuple(s) for s in spans] == [("az", 0.0, 0.08), ("??", 0.08, 0.08), ("b", 0.08, 0.24)]
    spans = CA.word_spans(["??", "b"], [[], [3]], [7], 10, frame_s=0.02, total_s=0.19)
    assert [tuple(s) for s in spans] == [("??", 0.0, 0.0), ("b", 0.0, 0.19)]
    with pytest.raises(ValueError):
        CA.word_spans(["??"], [[]], [], 10)
    bad = tmp_path / "bad.txt"
    bad.write_text("a 1 2\n")
    with pytest.raises(ValueError):
        CA.read_symbol_table(str(bad))


def test_frames_timestamp_properties():
    from f5e_tts_amd.ppg import ctc_align as CA
    rng = np.random.default_rng(3)
    for trial in range(30):
        L = int(rng.integers(1, 9))
        labels = rng.integers(1, 6, size=L)
        T = L + int((labels[1:] == labels[:-1]).sum()) + int(rng.integers(0, 25))
        al, _, start, stop, _ = R.align_one(R.log_softmax(R.planted(T, labels, 6, 100 + trial)), labels)
        segs = CA.frames_timestamp(al.tolist())
        assert len(segs) == L and sum(segs, []) == al.tolist()                      # the segments partition the frames
        for seg, y in zip(segs, labels):
            assert {c for c in seg if c != 0} == {int(y)}                           # one non-blank id per segment
        assert segs[-1][-1] == al[-1]                                               # trailing blanks join the last
        edges = np.cumsum([len(s) for s in segs])
        assert edges[-1] == T and np.array_equal(edges[:-1], stop[:-1])             # = the kernel's tok_end convention
    assert CA.frames_timestamp([0, 0, 3, 3, 0, 3, 0, 0]) == [[0, 0, 3, 3], [0, 3, 0, 0]]
    with pytest.raises(ValueError):
        CA.frames_timestamp([0, 0, 0])


# ------------------------------------------------------------------ the model mirror

def test_conformer_ppg_state_dict_is_unchanged_without_ctc_and_two_keys_longer_with_it():
    from f5e_tts_amd import _C
    from f5e_tts_amd.ppg.ppg_model import ConformerPPG
    kw = dict(input_dim=80, vocab_size=40, output_size=64, attention_heads=4, linear_units=128, num_blocks=2)
    plain, with_ctc = ConformerPPG(**kw), ConformerPPG(**kw, ctc=True)
    keys = list(plain.state_dict())
    z = np.load(os.path.join(GOLD, "ppg_conformer.npz"))
    fixture = {k[2:] for k in z.files if k.startswith("w/") and not k.startswith("w/encoder.global_cmvn")}
    assert fixture <= set(keys) and not any(k.startswith("ctc.") for k in keys)
    assert {k for k in keys if "concat_linear" not in k} == fixture
    extra = [k for k in with_ctc.state_dict() if k not in keys]
    assert extra == ["ctc.ctc_lo.weight", "ctc.ctc_lo.bias"] and len(with_ctc.state_dict()) == len(keys) + 2
    assert tuple(with_ctc.ctc.ctc_lo.weight.shape) == (40, 64) and with_ctc.eos == 39
    cfg = dict(input_dim=80, output_dim=40, cmvn_file=None, encoder_conf=dict(output_size=64, linear_units=128, num_blocks=1))
    assert list(ConformerPPG.from_config(cfg).state_dict()) == list(ConformerPPG.from_config(cfg, ctc=False).state_dict())
    assert "ctc.ctc_lo.bias" in ConformerPPG.from_config(cfg, ctc=True).state_dict()
    feats, lens = torch.zeros(1, 20, 80), torch.tensor([20])
    with pytest.raises(_C.F5EError, match="CTC head"):
        plain.ctc_greedy_search(feats, lens)
    with pytest.raises(_C.F5EError, match="CTC head"):
        plain.ctc_forced_align(feats, lens, [[1, 2]])


def test_host_label_lengths_are_validated_on_the_host():
    from f5e_tts_amd import _C
    from f5e_tts_amd.ppg.ppg_model import check_ctc_lengths
    check_ctc_lengths([[1, 2, 2]], [3], [4], 3)
    check_ctc_lengths(None, [3], [3], 3)                     # ids on the device: the lengths alone
    for l, t, L in (([0], [9], 3), ([4], [9], 3), ([3], [2], 3)):
        with pytest.raises(_C.F5EError, match="no CTC path"):
            check_ctc_lengths(None, l, t, L)
    with pytest.raises(_C.F5EError, match="label ids"):
        check_ctc_lengths([[1, 40]], [2], [9], 2, vocab=40)
    for labels, l, t in (([[1, 2, 2]], [3], [3]), ([[1, 2]], [0], [9]), ([[1, 2]], [3], [9]), ([[1, 1, 1]], [3], [4])):
        with pytest.raises(_C.F5EError, match="no CTC path"):
            check_ctc_lengths(labels, l, t, len(labels[0]))
