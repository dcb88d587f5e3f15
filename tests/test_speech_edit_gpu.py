"""Speech editing through the user-facing path (infer/speech_edit.py) on a tiny synthetic CFM + Vocos, and the CTC aligner
(ppg/ctc_align.py) end to end on the ASR model of tests/golden/ctc_asr.npz with a synthetic symbol table."""
import os

import numpy as np
import pytest
import torch

import ctc_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SR, HOP = 24000, 256
KW = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
PARTS, FIX = [[0.4, 0.7], [1.2, 1.5]], [0.35, 0.2]
ORIGIN, TARGET = "some call me nature others say mother", "some call me artist others say father"


def noise(secs, sr, seed, amp):
    return amp * torch.randn(1, int(secs * sr), generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def rig():
    from f5e_tts_amd.model import CFM, DiT
    from f5e_tts_amd.vocoder import Vocos
    from tools import synth as SY
    arch = dict(dim=1024, depth=2, heads=16, ff_mult=2, text_dim=256, conv_layers=2, text_num_embeds=300)
    dit = DiT(**arch)
    dit.load_state_dict(SY.init_dit_state(SY.DiTConfig(**arch), 21), strict=True)
    vocab = {c: i for i, c in enumerate(" abcdefghijklmnopqrstuvwxyz,.'")}
    cfm = CFM(transformer=dit, vocab_char_map=vocab).cuda().eval()
    voc = Vocos()
    voc.load_state_dict(SY.init_vocos_state(), strict=False)
    return cfm, voc.cuda().eval()


@pytest.fixture(scope="module")
def explicit(rig):
    from f5e_tts_amd.infer import speech_edit as SE
    cfm, voc = rig
    audio = noise(2.0, SR, 5, amp=0.3)                       # louder than target_rms: the samples go in as they are
    return audio, SE.speech_edit_process((audio, SR), ORIGIN, TARGET, cfm, voc, parts_to_edit=PARTS, fix_duration=FIX, **KW)


def test_explicit_parts_equal_the_direct_sampler_call(rig, explicit):
    from f5e_tts_amd.infer import utils_infer as U
    cfm, voc = rig
    audio, (wave, sr, mel) = explicit
    assembled, edit_mask = R.speech_edit_recipe(audio, SR, HOP, PARTS, FIX)
    assert assembled.shape[-1] == 48000 + round(0.35 * SR) + round(0.2 * SR) - round(0.3 * SR) - round(0.3 * SR) + 0
    with torch.inference_mode():
        gen, _ = cfm.sample(cond=assembled.cuda(), text=U.convert_char_to_pinyin([TARGET]),
                            duration=assembled.shape[-1] // HOP, steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3,
                            edit_mask=edit_mask.cuda())
        want_mel = gen.float().permute(0, 2, 1)
        cond_mel = cfm.mel_spec(assembled.cuda())            # [1, 100, frames]
    assert sr == SR and np.array_equal(mel, want_mel[0].cpu().numpy())
    frames = mel.shape[1]
    keep = edit_mask[0].numpy()
    assert len(keep) == assembled.shape[-1] // HOP + 1 == cond_mel.shape[-1] and frames >= len(keep)
    # the sampler keeps conditioned frames: where the mask is True the output IS the mel of the assembled audio
    assert np.array_equal(mel[:, :len(keep)][:, keep], cond_mel[0].cpu().numpy()[:, keep])
    edited = mel[:, :len(keep)][:, ~keep]
    assert (~keep).sum() == round(0.35 * SR / HOP) + round(0.2 * SR / HOP) and np.isfinite(edited).all()
    assert (np.abs(edited).max(0) > 0).all()                 # generated frames are not the zeros they were conditioned on
    assert not np.array_equal(edited, cond_mel[0].cpu().numpy()[:, ~keep])
    # the project's Vocos (ISTFT head, padding "center") returns hop * (frames - 1) samples
    assert wave.dtype == np.float32 and wave.shape == (HOP * (frames - 1),) and np.isfinite(wave).all()
    assert float(np.abs(wave).max()) > 0


def test_quiet_recording_is_raised_for_the_model_and_restored_after(rig):
    from f5e_tts_amd.infer import speech_edit as SE
    from f5e_tts_amd.infer import utils_infer as U
    cfm, voc = rig
    audio = noise(1.0, SR, 6, amp=0.02)
    wave, _, mel = SE.speech_edit_process((audio, SR), "a b c", "a d c", cfm, voc, parts_to_edit=[[0.3, 0.6]], **KW)
    rms = torch.sqrt(torch.mean(torch.square(audio)))
    with torch.inference_mode():
        lifted = (audio.cuda() * 0.1 / rms.cuda())
        pieces, mask = SE.plan_edit(audio.shape[-1], SR, HOP, [[0.3, 0.6]], None)
        gen, _ = cfm.sample(cond=SE.assemble(lifted, pieces), text=U.convert_char_to_pinyin(["a d c"]), duration=audio.shape[-1] // HOP, steps=4,
                            cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3,
                            edit_mask=torch.tensor([mask], device="cuda"))
        want = (voc.decode(gen.float().permute(0, 2, 1)) * rms.cuda() / 0.1).squeeze().cpu().numpy()
    assert np.array_equal(wave, want)


class StubAligner:
    """Fixed word spans for ORIGIN: 'nature' = [0.4, 0.7], 'mother' = [1.2, 1.5]."""

    def __init__(self):
        self.calls = []

    def align(self, audio, sr, text):
        from f5e_tts_amd.ppg.ctc_align import WordSpan, split_words
        self.calls.append((tuple(audio.shape), sr, text))
        edges = [0.0, 0.1, 0.25, 0.4, 0.7, 0.95, 1.2, 1.5]
        words = split_words(text)
        assert len(words) == 7
        return [WordSpan(w, a, b) for w, a, b in zip(words, edges[:-1], edges[1:])]


def test_parts_derived_from_an_aligner_equal_the_explicit_call(rig, explicit):
    from f5e_tts_amd.infer import speech_edit as SE
    from f5e_tts_amd.ppg.ctc_align import split_words
    cfm, voc = rig
    audio, (wave, _, mel) = explicit
    stub = StubAligner()
    parts, fix = SE.diff_parts(stub.align(audio, SR, ORIGIN), split_words(TARGET), FIX)
    assert parts == PARTS and fix == FIX
    wave2, _, mel2 = SE.speech_edit_process((audio, SR), ORIGIN, TARGET, cfm, voc, fix_duration=FIX, aligner=stub, **KW)
    assert stub.calls[-1] == ((1, 48000), SR, ORIGIN)
    assert np.array_equal(mel2, mel) and np.array_equal(wave2, wave)
    # fix_duration=None keeps every span's own duration: as many frames out as the recording has
    _, _, mel3 = SE.speech_edit_process((audio, SR), ORIGIN, TARGET, cfm, voc, aligner=stub, **KW)
    assert mel3.shape[1] == 48000 // HOP + 2
    with pytest.raises(ValueError, match="aligner"):
        SE.speech_edit_process((audio, SR), ORIGIN, TARGET, cfm, voc, **KW)
    with pytest.raises(ValueError, match="fix_duration"):
        SE.speech_edit_process((audio, SR), ORIGIN, "some call me dear nature others say mother", cfm, voc, aligner=stub,
                               **KW)


def test_ctc_aligner_end_to_end_on_the_fixture_model():
    from f5e_tts_amd.ppg import ConformerPPG
    from f5e_tts_amd.ppg.ctc_align import CTCAligner
    base, z = np.load(os.path.join(GOLD, "ppg_conformer.npz")), np.load(os.path.join(GOLD, "ctc_asr.npz"))
    sd = {k[2:]: torch.from_numpy(f[k]) for f in (base, z) for k in f.files if k.startswith("w/")}
    m = ConformerPPG(80, 40, 64, 4, 128, 2, 15, global_cmvn=(sd["encoder.global_cmvn.mean"], sd["encoder.global_cmvn.istd"]),
                     ctc=True)
    full = m.state_dict()
    full.update(sd)
    m.load_state_dict(full)
    table = {"<blank>": 0, "<sos/eos>": 39}                          # no <unk>: characters without an entry are dropped
    table.update({c: 2 + i for i, c in enumerate("abcdefghijklmnopqrstuvwxyz'")})
    al = CTCAligner(device="cuda", model=m.cuda().eval(), symbol_table=table)
    audio = noise(1.3, 22050, 7, amp=0.2)
    text = "Some call  me ?? nature"
    spans = al.align(audio, 22050, text)
    assert [s.word for s in spans] == ["Some", "call", "me", "??", "nature"]
    assert spans[0].start_s == 0.0 and 1.2 < spans[-1].end_s <= 1.3                # the segments cover the recording (whole encoder frames)
    for a, b in zip(spans[:-1], spans[1:]):
        assert a.start_s <= a.end_s == b.start_s <= b.end_s <= 1.3 + 1e-9         # monotone, no overlap, inside the audio
    assert spans[3].start_s == spans[3].end_s == spans[2].end_s                   # a word without tokens: an empty span
    assert all(s.end_s > s.start_s for i, s in enumerate(spans) if i != 3)
    heard = al.transcribe(audio, 22050)
    assert isinstance(heard, str)
    with pytest.raises(ValueError):
        al.align(audio, 22050, "?? !!")
    # a symbol-table id the model has no class for: an error, never spans built from a "no path" row
    from f5e_tts_amd import _C
    bad = CTCAligner(device="cuda", model=al.model, symbol_table=dict(table, z=40))
    with pytest.raises(_C.F5EError, match="label ids"):
        bad.align(audio, 22050, "a z")
