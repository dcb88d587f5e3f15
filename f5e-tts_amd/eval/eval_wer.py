"""WER of generated wavs against their texts, the way Seed-TTS scores it: the counterpart of the reference's ``run_asr_wer``
(eval/utils_eval.py:494-562) on the project's own recogniser (``CTCAligner.transcribe`` on a wenet conformer, any of the
2x / 4x / 6x / 8x fronts) in place of faster-whisper / paraformer.

    python -m f5e_tts_amd.eval.eval_wer --gen_wav_dir D --metalst F --lang en|zh --asr_model M --asr_config C --asr_dict T
                                        [--mode ctc_greedy_search|ctc_prefix_beam_search|attention_rescoring]

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
                **decode) -> List[Dict]:
    """``items``: (gen_wav, prompt_wav, truth) as ``eval_sim.get_test_set`` returns them; ``aligner``: anything with
    ``transcribe(wav_path, None, mode=..., **decode) -> str`` (a ``CTCAligner``).  -> the reference's per-utterance dicts
    ``{"wav", "truth", "hypo", "wer"}`` with the RAW texts."""
    if lang not in LANGS:
        raise NotImplementedError(f"lang {lang!r}: only 'zh' and 'en' are supported")
    results = []
    for gen_wav, _prompt_wav, truth in items:
        hypo = aligner.transcribe(gen_wav, None, mode=mode, **decode)
        results.append({"wav": Path(gen_wav).stem, "truth": truth, "hypo": hypo,
                        "wer": wer(normalize(truth, lang), normalize(hypo, lang))})
    return results


def main(argv=None, aligner=None) -> float:
    from .eval_sim import get_test_set
    ap = argparse.ArgumentParser(description="WER of generated wavs against their texts on the project's recogniser")
    ap.add_argument("--metalst", required=True, help="utt|prompt_text|prompt_wav|gt_text per line")
    ap.add_argument("--gen_wav_dir", required=True)
    ap.add_argument("--lang", required=True, choices=LANGS)
    ap.add_argument("--asr_model", required=aligner is None, help="wenet conformer checkpoint (CTC head; decoder for rescoring)")
    ap.add_argument("--asr_config", required=aligner is None, help="its train.yaml (input_layer conv2d / conv2d4 / conv2d6 / conv2d8)")
    ap.add_argument("--asr_dict", required=aligner is None, help="its `token id` symbol table")
    ap.add_argument("--mode", default="ctc_greedy_search",
                    choices=("ctc_greedy_search", "ctc_prefix_beam_search", "attention_rescoring"))
    ap.add_argument("--beam_size", type=int, default=10)
    ap.add_argument("--out", default=None, help="per-utterance JSON (default: <gen_wav_dir>/_wer_results.json)")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    test_set = get_test_set(args.metalst, args.gen_wav_dir)
    if not test_set:
        raise SystemExit(f"{args.metalst}: no utterance has a generated wav under {args.gen_wav_dir}")
    if aligner is None:
        from ..ppg.ctc_align import CTCAligner
        aligner = CTCAligner(args.asr_model, args.asr_config, args.asr_dict, args.device, asr=True,
                             decoder=args.mode == "attention_rescoring")
    results = run_asr_wer(test_set, aligner, args.lang, args.mode, beam_size=args.beam_size)
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
