"""WER of generated wavs against their texts, the way Seed-TTS scores it: the counterpart of the reference's ``run_asr_wer``
(eval/utils_eval.py:494-562) on the project's own recogniser (``CTCAligner.transcribe`` on a wenet conformer, any of the
2x / 4x / 6x / 8x fronts) in place of faster-whisper / paraformer.

    python -m f5e_tts_amd.eval.eval_wer --gen_wav_dir D --metalst F --lang en|zh --asr_model M --asr_config C --asr_dict T
                                        [--mode ctc_greedy_search|ctc_prefix_beam_search|attention_rescoring]
    python -m f5e_tts_amd.eval.eval_wer --gen_wav_dir D --metalst F --lang en --asr whisper --whisper_dir W [--language english]
                                        [--whisper_beam 5] [--whisper_long [--whisper_fallback [--whisper_seed S]]
                                        [--whisper_prompt TEXT] [--whisper_condition]]
                                        [--whisper_assistant DIR [--whisper_assistant_tokens N]
                                         [--whisper_assistant_shares_encoder]]
                                        [--whisper_step_graph [--whisper_step_gemm skinny]]
    python -m f5e_tts_amd.eval.eval_wer --gen_wav_dir D --metalst F --lang zh --asr paraformer --paraformer_dir P

``--asr paraformer`` is the reference's Chinese recogniser (``load_asr_model("zh")``, eval/utils_eval.py:472-482: funasr
paraformer-zh) on the device (eval/paraformer.py), with ``normalize`` as the clean-up; parity with funasr is unpinned.

``--asr whisper`` is the reference's English recogniser of the voice-conversion and LibriSpeech evaluations
(``run_asr_wer_whisper_large_v3``, eval/utils_eval.py:631-712: whisper-large-v3, greedy, prompt ``english / transcribe``) on the
device (eval/whisper.py), with that function's own clean-up (``normalize_whisper_en``) in place of ``normalize``.
``--whisper_beam N`` (default 1 = greedy) searches with N beams instead: the setting of the reference's headline English WER
(``run_asr_wer``, eval/utils_eval.py:517-526, ``beam_size=5``), here with the semantics of ``transformers``'
``generate(num_beams=N)`` -- K open rows and a length-normalised pool of finished hypotheses -- not CTranslate2's.
``--beam_size`` stays the wenet flag; the Whisper recogniser ignores it.

Host code.  Deviations from the reference, parity unpinned (``jiwer``, ``zhon`` and ``zhconv`` are not dependencies here):
  * punctuation is ``string.punctuation`` plus every character of Unicode category P* (the reference: ``zhon.hanzi.punctuation
    + string.punctuation``);
  * no traditional -> simplified conversion of a zh hypothesis (the reference: ``zhconv.convert(hypo, "zh-cn")``);
  * the edit distance is a plain Levenshtein table over whitespace-split words (``jiwer.compute_measures`` in the
    reference).  WER = (S + D + I) / N is the minimum over all alignments and does not depend on how ties between them are
    broken; the S / D / I SPLIT does, and here the backtrace prefers a diagonal step (hit or substitution), then a
    deletion, then an insertion."""
from __future__ import annotations

import argparse
import json
import os
import re
import string
import unicodedata
from pathlib import Path
from typing import Dict, Iterable, List, Sequence, Tuple

LANGS = ("en", "zh")


def is_punctuation(ch: str) -> bool:
    return ch in string.punctuation or unicodedata.category(ch).startswith("P")


def normalize(text: str, lang: str) -> str:
    """The reference's clean-up in its order (utils_eval.py:531-543): punctuation removed, ONE pass of double space ->
    space, then ``zh``: every character its own word (spaces included, as there); ``en``: lower case."""
    if lang not in LANGS:
        raise NotImplementedError(f"lang {lang!r}: only 'zh' and 'en' are supported")
    text = "".join(ch for ch in text if not is_punctuation(ch))
    text = text.replace("  ", " ")
    return " ".join(text) if lang == "zh" else text.lower()


_SMALL = ("zero one two three four five six seven eight nine ten eleven twelve thirteen fourteen fifteen sixteen seventeen "
          "eighteen nineteen").split()
_TENS = "- - twenty thirty forty fifty sixty seventy eighty ninety".split()


def spell_number(n: int) -> str:
    """British-style cardinal, as the reference spells digits in a Whisper hypothesis (utils_eval.py:566-603): "and" after the
    hundreds when anything follows, and after the thousands when less than a hundred follows."""
    if n == 0:
        return _SMALL[0]
    words = []
    if n >= 1000000:
        words.append(spell_number(n // 1000000) + " million")
        n %= 1000000
    if n >= 1000:
        words.append(spell_number(n // 1000) + " thousand")
        n %= 1000
        if 0 < n < 100:
            words.append("and")
    if n >= 100:
        words.append(_SMALL[n // 100] + " hundred")
        n %= 100
        if n:
            words.append("and")
    if n >= 20:
        words.append(_TENS[n // 10])
        n %= 10
    if n:
        words.append(_SMALL[n])
    return " ".join(words).replace(" and zero", "").replace("  ", " ")


def replace_mixed_numbers(text: str) -> str:
    """Every run of digits spelled out and set off by spaces ("18th" -> "eighteen th"); whitespace runs collapse
    (utils_eval.py:605-616)."""
    parts = [spell_number(int(p)) if p.isdigit() else p for p in re.findall(r"\d+|\D+", text)]
    return re.sub(r"\s+", " ", " ".join(parts)).strip()


def replace_special(text: str) -> str:
    """utils_eval.py:618-627: a "$" moves to a closing "dollars", "supercomputer" splits, "18th" / "19th" are spelled.  (After
    ``replace_mixed_numbers`` and the punctuation pass of ``normalize_whisper_en`` only the second can still apply; the order
    is the reference's.)"""
    if "$" in text:
        text = text.replace("$", "") + "dollars"
    return text.replace("supercomputer", "super computer").replace("18th", "eighteenth").replace("19th", "nineteenth")


def normalize_whisper_en(text: str, hypo: bool) -> str:
    """The clean-up of the reference's Whisper WER path in its order (utils_eval.py:674-693).  Both sides: ASCII punctuation and
    the typographic apostrophe removed, ONE pass of double space -> space, lower case.  The hypothesis also: "-" -> " " (a no-op
    by then: the hyphen went with the punctuation, "twenty-one" is "twentyone"), everything but word characters, whitespace and
    "'" removed, digits spelled out, ``replace_special``."""
    for ch in string.punctuation:
        text = text.replace(ch, "")
    text = text.replace("\u2019", "").replace("  ", " ")
    if not hypo:
        return text.lower()
    text = re.sub(r"[^\w\s']", "", text.replace("-", " ")).lower()
    return replace_special(replace_mixed_numbers(text))


def word_errors(ref: Sequence, hyp: Sequence) -> Tuple[int, int, int, int]:
    """(hits, substitutions, deletions, insertions) of a minimum-cost alignment of ``hyp`` to ``ref`` (unit costs):
    hits + subs + dels = len(ref), hits + subs + ins = len(hyp).  Tie-break of the backtrace: diagonal, deletion,
    insertion."""
    n, m = len(ref), len(hyp)
    d = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(1, n + 1):
        d[i][0] = i
    for j in range(1, m + 1):
        d[0][j] = j
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            d[i][j] = min(d[i - 1][j - 1] + (ref[i - 1] != hyp[j - 1]), d[i - 1][j] + 1, d[i][j - 1] + 1)
    hits = subs = dels = ins = 0
    i, j = n, m
    while i > 0 or j > 0:
        if i > 0 and j > 0 and d[i][j] == d[i - 1][j - 1] + (ref[i - 1] != hyp[j - 1]):
            if ref[i - 1] == hyp[j - 1]:
                hits += 1
            else:
                subs += 1
            i, j = i - 1, j - 1
        elif i > 0 and d[i][j] == d[i - 1][j] + 1:
            dels, i = dels + 1, i - 1
        else:
            ins, j = ins + 1, j - 1
    return hits, subs, dels, ins


def wer(truth: str, hypo: str) -> float:
    """(S + D + I) / N over whitespace-split words; an empty reference has no error rate."""
    ref, hyp = truth.split(), hypo.split()
    if not ref:
        raise ValueError("wer: the reference has no words after normalisation")
    _, s, d, i = word_errors(ref, hyp)
    return (s + d + i) / len(ref)


def run_asr_wer(items: Iterable[Tuple[str, str, str]], aligner, lang: str, mode: str = "ctc_greedy_search",
                whisper_cleanup: bool = False, **decode) -> List[Dict]:
    """``items``: (gen_wav, prompt_wav, truth) as ``eval_sim.get_test_set`` returns them; ``aligner``: anything with
    ``transcribe(wav_path, None, mode=..., **decode) -> str`` (a ``CTCAligner``).  -> the reference's per-utterance dicts
    ``{"wav", "truth", "hypo", "wer"}`` with the RAW texts.  ``whisper_cleanup``: ``normalize_whisper_en`` instead of
    ``normalize`` (the reference's Whisper path, ``en`` only)."""
    if whisper_cleanup and lang != "en":
        raise NotImplementedError("the Whisper WER path is the reference's English recogniser: --lang en")
    if lang not in LANGS:
        raise NotImplementedError(f"lang {lang!r}: only 'zh' and 'en' are supported")
    results = []
    for gen_wav, _prompt_wav, truth in items:
        hypo = aligner.transcribe(gen_wav, None, mode=mode, **decode)
        if whisper_cleanup:
            score = wer(normalize_whisper_en(truth, False), normalize_whisper_en(hypo, True))
        else:
            score = wer(normalize(truth, lang), normalize(hypo, lang))
        results.append({"wav": Path(gen_wav).stem, "truth": truth, "hypo": hypo, "wer": score})
    return results


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="WER of generated wavs against their texts on the project's recogniser")
    ap.add_argument("--metalst", required=True, help="utt|prompt_text|prompt_wav|gt_text per line")
    ap.add_argument("--gen_wav_dir", required=True)
    ap.add_argument("--lang", required=True, choices=LANGS)
    ap.add_argument("--asr", default="wenet", choices=("wenet", "whisper", "paraformer"),
                    help="wenet: the project's conformer recogniser; whisper: the reference's English WER recogniser on the device; "
                         "paraformer: the reference's Chinese WER recogniser (funasr paraformer-zh) on the device")
    ap.add_argument("--paraformer_dir", default=None, help="--asr paraformer: a local funasr model directory (config.yaml, "
                    "model.pt, am.mvn, tokens.json)")
    ap.add_argument("--whisper_dir", default=None, help="--asr whisper: a local whisper-large-v3 directory (config.json, "
                    "generation_config.json, model.safetensors, vocab.json, added_tokens.json)")
    ap.add_argument("--language", default="english", help="--asr whisper: the language token of the forced prompt")
    ap.add_argument("--whisper_long", action="store_true",
                    help="--asr whisper: transcribe recordings beyond 30 s to their end, window after window with timestamp "
                         "tokens (the sequential algorithm of the reference's recogniser) instead of cutting them with a warning")
    ap.add_argument("--whisper_fallback", action="store_true",
                    help="--whisper_long: temperature fallback (0.0, 0.2, ... 1.0) with compression_ratio_threshold 1.35 and "
                         "logprob_threshold -1.0: a window that loops or is very unlikely is decoded again, sampled")
    ap.add_argument("--whisper_seed", type=int, default=0, help="--whisper_fallback: the seed of the sampled decodes")
    ap.add_argument("--whisper_prompt", default=None, metavar="TEXT",
                    help="--whisper_long: an initial prompt (a name, a domain word). Without --whisper_condition it leads EVERY window of a "
                         "recording; with it, it leads the first window's previous text and then scrolls out of it")
    ap.add_argument("--whisper_condition", action="store_true",
                    help="--whisper_long: condition every window on the text of the windows before it")
    ap.add_argument("--whisper_assistant", default=None, metavar="DIR",
                    help="--asr whisper: a local draft model directory (whisper-large-v3-turbo, a distil-whisper checkpoint) for "
                         "assisted generation: the same transcripts with fewer passes of the large decoder; greedy only")
    ap.add_argument("--whisper_assistant_tokens", type=int, default=5, help="--whisper_assistant: tokens drafted per round")
    ap.add_argument("--whisper_assistant_shares_encoder", action="store_true",
                    help="--whisper_assistant: the draft reads the large model's encoder output instead of running its own")
    ap.add_argument("--whisper_step_graph", action="store_true",
                    help="--asr whisper: replay every pick from one decode step captured as a hipGraph (the same transcripts; "
                         "greedy, --whisper_beam 1, no --whisper_assistant; the time is won with --whisper_step_gemm skinny)")
    ap.add_argument("--whisper_step_gemm", choices=("f32", "skinny"), default="f32",
                    help="--whisper_step_graph: the GEMM of the captured step; skinny spreads each weight read over the whole chip")
    ap.add_argument("--whisper_weights", choices=("f32", "fp16", "bf16", "auto"), default="f32",
                    help="--asr whisper: the type the matrices are held in on the device; fp16 / bf16 halve the weight memory and "
                         "the bytes of a decode step (an fp16 checkpoint then gives the f32 transcripts, bit for bit); auto: the "
                         "type the checkpoint stores")
    ap.add_argument("--whisper_beam", type=int, default=1,
                    help="--asr whisper: 1 = greedy (run_asr_wer_whisper_large_v3); N > 1 = the pooled beam search of "
                         "generate(num_beams=N) (--beam_size is the wenet flag and does not reach Whisper)")
    ap.add_argument("--asr_model", default=None, help="wenet conformer checkpoint (CTC head; decoder for rescoring)")
    ap.add_argument("--asr_config", default=None, help="its train.yaml (input_layer conv2d / conv2d4 / conv2d6 / conv2d8)")
    ap.add_argument("--asr_dict", default=None, help="its `token id` symbol table")
    ap.add_argument("--mode", default="ctc_greedy_search",
                    choices=("ctc_greedy_search", "ctc_prefix_beam_search", "attention_rescoring"))
    ap.add_argument("--beam_size", type=int, default=10)
    ap.add_argument("--out", default=None, help="per-utterance JSON (default: <gen_wav_dir>/_wer_results.json)")
    ap.add_argument("--device", default="cuda")
    return ap


def main(argv=None, aligner=None) -> float:
    from .eval_sim import get_test_set
    ap = build_parser()
    args = ap.parse_args(argv)
    if aligner is None:
        need = {"whisper": ("whisper_dir",), "paraformer": ("paraformer_dir",)}.get(args.asr, ("asr_model", "asr_config", "asr_dict"))
        missing = [f"--{n}" for n in need if getattr(args, n) is None]
        if missing:
            ap.error(f"the following arguments are required: {', '.join(missing)}")
    test_set = get_test_set(args.metalst, args.gen_wav_dir)
    if not test_set:
        raise SystemExit(f"{args.metalst}: no utterance has a generated wav under {args.gen_wav_dir}")
    if aligner is None and args.asr == "whisper":
        from .whisper import Fallback, WhisperRecognizer
        if args.whisper_fallback and not args.whisper_long:
            ap.error("--whisper_fallback needs --whisper_long")
        fb = Fallback(compression_ratio_threshold=1.35, logprob_threshold=-1.0, seed=args.whisper_seed) if args.whisper_fallback \
            else None
        if (args.whisper_prompt is not None or args.whisper_condition) and not args.whisper_long:
            ap.error("--whisper_prompt and --whisper_condition need --whisper_long")
        ctx = {}
        if args.whisper_prompt is not None or args.whisper_condition:
            ctx = dict(initial_prompt=args.whisper_prompt, condition_on_previous_text=args.whisper_condition)
        if args.whisper_assistant is not None:
            ctx.update(assistant_dir=args.whisper_assistant, num_assistant_tokens=args.whisper_assistant_tokens,
                       assistant_shares_encoder=args.whisper_assistant_shares_encoder)
        if args.whisper_step_gemm != "f32" and not args.whisper_step_graph:
            ap.error("--whisper_step_gemm needs --whisper_step_graph")
        if args.whisper_step_graph:
            ctx.update(step_graph=True, step_gemm=args.whisper_step_gemm)
        if args.whisper_weights != "f32":
            ctx.update(weights=args.whisper_weights)
        aligner = WhisperRecognizer(args.whisper_dir, args.device, args.language, beam_size=args.whisper_beam,
                                    long_form=args.whisper_long, **({} if fb is None else dict(fallback=fb)), **ctx)
    elif aligner is None and args.asr == "paraformer":
        from .paraformer import ParaformerRecognizer
        aligner = ParaformerRecognizer(args.paraformer_dir, args.device)
    elif aligner is None:
        from ..ppg.ctc_align import CTCAligner
        aligner = CTCAligner(args.asr_model, args.asr_config, args.asr_dict, args.device, asr=True,
                             decoder=args.mode == "attention_rescoring")
    results = run_asr_wer(test_set, aligner, args.lang, args.mode, whisper_cleanup=args.asr == "whisper", beam_size=args.beam_size)
    for r in results:
        print(f"{r['wav']}\t{r['wer']:.4f}\t{r['hypo']}")
    mean = sum(r["wer"] for r in results) / len(results)
    out = args.out or os.path.join(args.gen_wav_dir, "_wer_results.json")
    with open(out, "w") as f:
        json.dump(results, f, indent=1, ensure_ascii=False)
    print(f"WER: {mean:.5f} over {len(results)} utterances -> {out}")
    return mean


if __name__ == "__main__":
    main()
