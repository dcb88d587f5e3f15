"""Command-line entry with the argument surface of reference infer/infer_cli.py:34-171 and its three-layer setting
resolution (flag > TOML > module default, including the ``x or default`` quirk that lets falsy flag values such as
``--cfg_strength 0`` fall through, reference :181-211).  Model/vocoder weights are local files only (no network).

Beyond the reference: ``--mode tts|vc`` reach the PPG / codebook model family (``sample_tts`` through the same text
chunking; ``--source_audio`` converted to the prompt's voice through ``utils_infer.infer_vc_process``), which the
reference only drives from its eval scripts.  ``--best_of N`` draws N candidates per text chunk and keeps the one the ASR
model's CTC head finds most consistent with the text (``--asr_model`` / ``--asr_config`` / ``--asr_dict``, the names of
``speech_edit.py``; ``--seed`` makes the draw reproducible).  Without the new flags ``main`` does what it always did."""
from __future__ import annotations

import argparse
import os
import re
from datetime import datetime

import numpy as np

from . import utils_infer as U

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python3 infer-cli.py",
                                description="Commandline interface for E2/F5 TTS with Advanced Batch Processing.",
                                epilog="Specify options above to override one or more settings from config.")
    p.add_argument("-c", "--config", type=str, default="", help="TOML configuration file")
    p.add_argument("-m", "--model", type=str, help="The model name: F5TTS_v1_Base | ...")
    p.add_argument("-mc", "--model_cfg", type=str, help="The path to the model config file .yaml")
    p.add_argument("-p", "--ckpt_file", type=str, help="The path to model checkpoint .pt/.safetensors")
    p.add_argument("-v", "--vocab_file", type=str, help="The path to vocab file .txt")
    p.add_argument("-r", "--ref_audio", type=str, help="The reference audio file.")
    p.add_argument("-s", "--ref_text", type=str, help="The transcript/subtitle for the reference audio")
    p.add_argument("-t", "--gen_text", type=str, help="The text to make model synthesize a speech")
    p.add_argument("-f", "--gen_file", type=str, help="The file with text to generate, will ignore --gen_text")
    p.add_argument("-o", "--output_dir", type=str, help="The path to output folder")
    p.add_argument("-w", "--output_file", type=str, help="The name of output file")
    p.add_argument("--save_chunk", action="store_true", help="To save each audio chunks during inference")
    p.add_argument("--remove_silence", action="store_true", help="To remove long silence found in output")
    p.add_argument("--load_vocoder_from_local", action="store_true", help="To load vocoder from local dir")
    p.add_argument("--vocoder_name", type=str, choices=["vocos", "bigvgan"], help="vocoder")
    p.add_argument("--target_rms", type=float, help="Target output speech loudness normalization value")
    p.add_argument("--cross_fade_duration", type=float, help="Duration of cross-fade between audio segments in seconds")
    p.add_argument("--nfe_step", type=int, help="The number of function evaluation (denoising steps)")
    p.add_argument("--cfg_strength", type=float, help="Classifier-free guidance strength")
    p.add_argument("--sway_sampling_coef", type=float, help="Sway Sampling coefficient")
    p.add_argument("--speed", type=float, help="The speed of the generated audio")
    p.add_argument("--fix_duration", type=float, help="Fix the total duration (ref and gen audios) in seconds")
    p.add_argument("--device", type=str, help="Specify the device to run on")
    p.add_argument("--mode", type=str, choices=["cfg", "tts", "vc"],
                   help="cfg: sample with --cfg_strength (default); tts: sample_tts of a PPG model with --alpha_spk / "
                        "--alpha_txt; vc: convert --source_audio to the voice of --ref_audio (default when "
                        "--source_audio is given)")
    p.add_argument("--source_audio", type=str, help="vc mode: the audio file whose content is converted")
    p.add_argument("--alpha_spk", type=float, help="tts / vc: speaker guidance strength")
    p.add_argument("--alpha_txt", type=float, help="tts: text guidance strength")
    p.add_argument("--alpha_ppg", type=float, help="vc: PPG guidance strength")
    p.add_argument("--ppg_model", type=str, help="vc: PPG checkpoint (default: ppg_config.model_path of the model yaml)")
    p.add_argument("--ppg_config", type=str, help="vc: PPG train.yaml (default: ppg_config.config of the model yaml)")
    p.add_argument("--ppg_stream", action="store_true",
                   help="vc: extract the PPGs chunk by chunk (for conversion models trained on streaming PPGs)")
    p.add_argument("--best_of", type=int, default=1,
                   help="cfg / tts: draw N candidates per text chunk and keep the one the ASR model scores highest "
                        "(needs --asr_model, --asr_config and --asr_dict)")
    p.add_argument("--seed", type=int, help="cfg / tts: candidate i of chunk c is sampled with seed + c * best_of + i, the "
                                            "chunks counted through all [voice] segments of the text")
    p.add_argument("--asr_model", type=str, help="best_of: ASR checkpoint with a CTC head (a PPG model's .pt)")
    p.add_argument("--asr_config", type=str, help="best_of: the ASR model's train.yaml")
    p.add_argument("--asr_dict", type=str, help="best_of: the ASR model's symbol table (`token id` lines)")
    p.add_argument("--whisper_dir", type=str, help="a local whisper-large-v3(-turbo) directory: a voice whose ref_text is empty "
                                                   "is transcribed with it (without it an empty ref_text is an error)")
    p.add_argument("--ref_language", type=str, default="english", help="--whisper_dir: the language spoken in the reference audio; auto: detected "
                   "from the audio")
    p.add_argument("--whisper_beam", type=int, default=1, help="--whisper_dir: 1 = greedy; N > 1 = beam search with N beams")
    p.add_argument("--whisper_weights", type=str, choices=("f32", "fp16", "bf16", "auto"), default="f32",
                   help="--whisper_dir: the type the model's matrices are held in on the device (fp16 / bf16: half the memory; auto: "
                        "the type the checkpoint stores)")
    p.add_argument("--whisper_assistant", type=str, default=None, metavar="DIR",
                   help="--whisper_dir: a local draft model directory (whisper-large-v3-turbo, distil-whisper) for assisted "
                        "generation: the same transcript with fewer passes of the large decoder; greedy only")
    p.add_argument("--whisper_step_graph", action="store_true",
                   help="--whisper_dir: replay every pick of the transcription from one decode step captured as a hipGraph (the "
                        "same transcript; --whisper_beam 1, no --whisper_assistant)")
    p.add_argument("--whisper_prompt", type=str, default=None, metavar="TEXT",
                   help="--whisper_dir: an initial prompt for the transcription (a name, a domain word), in front of every window; the "
                        "reference audio is then transcribed with the long-form loop")
    return p


def require_scorer_args(args: argparse.Namespace) -> None:
    """--best_of is checked before anything is loaded."""
    if args.best_of < 1:
        raise SystemExit("--best_of must be at least 1")
    if args.best_of > 1:
        missing = [f"--{k}" for k in ("asr_model", "asr_config", "asr_dict") if not getattr(args, k)]
        if missing:
            raise SystemExit(f"--best_of {args.best_of} ranks the candidates with an ASR model: {', '.join(missing)} missing")


def next_segment_seed(seed: int, n_chunks: int, best_of: int) -> int:
    """``--seed`` numbers the candidates of the whole run: a ``[voice]`` segment of n chunks uses seed .. seed + n * best_of
    - 1 (candidate i of its chunk c: seed + c * best_of + i), and the next segment starts behind them -- with the same seed
    again, two segments would be sampled from identical noise."""
    return seed + n_chunks * best_of


# local vocoder directories when the config names none (reference infer_cli.py:264-267; no download here)
DEFAULT_VOCODER_PATH = {"vocos": "pretrained_models/vocos-mel-24khz",
                        "bigvgan": "pretrained_models/bigvgan_v2_24khz_100band_256x"}


def resolve_settings(args: argparse.Namespace, config: dict) -> dict:
    """flag > toml > default, with the reference's falsy-``or`` semantics (only ref_text uses ``is not None``)."""
    g = config.get
    s = dict(
        model=args.model or g("model", "F5TTS_v1_Base"),
        model_cfg=args.model_cfg or g("model_cfg", ""),
        ckpt_file=args.ckpt_file or g("ckpt_file", ""),
        vocab_file=args.vocab_file or g("vocab_file", ""),
        ref_audio=args.ref_audio or g("ref_audio", "infer/examples/basic/basic_ref_en.wav"),
        ref_text=args.ref_text if args.ref_text is not None
        else g("ref_text", "Some call me nature, others call me mother nature."),
        gen_text=args.gen_text or g("gen_text", "Here we generate something just for test."),
        gen_file=args.gen_file or g("gen_file", ""),
        output_dir=args.output_dir or g("output_dir", "tests"),
        output_file=args.output_file or g("output_file", f"infer_cli_{datetime.now().strftime(r'%Y%m%d_%H%M%S')}.wav"),
        save_chunk=args.save_chunk or g("save_chunk", False),
        remove_silence=args.remove_silence or g("remove_silence", False),
        load_vocoder_from_local=args.load_vocoder_from_local or g("load_vocoder_from_local", False),
        vocoder_name=args.vocoder_name or g("vocoder_name", U.mel_spec_type),
        target_rms=args.target_rms or g("target_rms", U.target_rms),
        cross_fade_duration=args.cross_fade_duration or g("cross_fade_duration", U.cross_fade_duration),
        nfe_step=args.nfe_step or g("nfe_step", U.nfe_step),
        cfg_strength=args.cfg_strength or g("cfg_strength", U.cfg_strength),
        sway_sampling_coef=args.sway_sampling_coef or g("sway_sampling_coef", U.sway_sampling_coef),
        speed=args.speed or g("speed", U.speed),
        fix_duration=args.fix_duration or g("fix_duration", U.fix_duration),
        device=args.device or g("device", U.device),
        source_audio=args.source_audio or g("source_audio", ""),
        alpha_spk=args.alpha_spk or g("alpha_spk", 2.5),
        alpha_txt=args.alpha_txt or g("alpha_txt", 3.0),
        alpha_ppg=args.alpha_ppg or g("alpha_ppg", 3.0),
        ppg_model=args.ppg_model or g("ppg_model", ""),
        ppg_config=args.ppg_config or g("ppg_config", ""),
        ppg_stream=args.ppg_stream or g("ppg_stream", False),
    )
    # --source_audio without a mode means voice conversion
    s["mode"] = args.mode or g("mode", "") or ("vc" if s["source_audio"] else "cfg")
    if s["mode"] not in ("cfg", "tts", "vc"):
        raise SystemExit(f"unknown mode {s['mode']!r} in the config (cfg / tts / vc)")
    return s


def load_arch(model: str, model_cfg: str) -> dict:
    import yaml
    path = model_cfg or os.path.join(_PKG, "configs", f"{model}.yaml")
    with open(path, "r") as f:
        cfg = yaml.safe_load(f)
    arch = dict(cfg["model"]["arch"])
    arch.pop("checkpoint_activations", None)
    return arch


def load_model_config(model: str, model_cfg: str) -> dict:
    """The ``train.parse_cfg.parse_model_yaml`` split of the model yaml: ``arch`` (what ``load_arch`` returns), the backbone
    / CFM dicts of the PPG and codebook blocks (``transformer_ppg_config``, ``cfm_ppg_config``,
    ``transformer_codebook_config``, ``cfm_codebook_config``) and ``frontend_ppg_config`` for the PPG extractor."""
    import yaml

    from ..train.parse_cfg import parse_model_yaml
    path = model_cfg or os.path.join(_PKG, "configs", f"{model}.yaml")
    with open(path, "r") as f:
        return parse_model_yaml(yaml.safe_load(f))


def require_ppg_model(mode: str, mc: dict) -> None:
    if mode in ("tts", "vc") and not mc["transformer_ppg_config"]["use_ppg"]:
        raise SystemExit(f"--mode {mode} needs a model with use_ppg: True in its yaml (a PPG-conditioned model)")


def split_voices(gen_text: str):
    """``[voice]`` tags split the text into (voice, text) chunks (reference infer_cli.py:306-321)."""
    out = []
    for chunk in re.split(r"(?=\[\w+\])", gen_text):
        if not chunk.strip():
            continue
        m = re.match(r"\[(\w+)\]", chunk)
        out.append((m[1] if m else "main", re.sub(r"\[(\w+)\]", "", chunk).strip()))
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    require_scorer_args(args)
    config = {}
    if args.config:
        import tomli
        with open(args.config, "rb") as f:
            config = tomli.load(f)
    s = resolve_settings(args, config)
    if s["mode"] == "vc" and args.best_of > 1:
        raise SystemExit("--best_of is for text-to-speech (--mode cfg / tts); voice conversion has no text to score")
    if s["gen_file"]:
        with open(s["gen_file"], "r", encoding="utf-8") as f:
            s["gen_text"] = f.read()
    from ..model import DiT
    mc = None
    if s["mode"] != "cfg":      # refuse a model without PPG conditioning before anything is loaded
        mc = load_model_config(s["model"], s["model_cfg"])
        require_ppg_model(s["mode"], mc)
        if s["mode"] == "vc" and not s["source_audio"]:
            raise SystemExit("--mode vc needs --source_audio")
    vocoder = U.load_vocoder(s["vocoder_name"], is_local=True,
                             local_path=config.get("vocoder_local_path", DEFAULT_VOCODER_PATH[s["vocoder_name"]]),
                             device=s["device"])
    mc = mc or load_model_config(s["model"], s["model_cfg"])
    family = {}
    if mc["transformer_ppg_config"]["use_ppg"]:     # a PPG / codebook yaml: the plain load_model call cannot build it
        family = dict(ppg_config=(mc["transformer_ppg_config"], mc["cfm_ppg_config"]),
                      cb_config=(mc["transformer_codebook_config"], mc["cfm_codebook_config"]))
    model = U.load_model(DiT, load_arch(s["model"], s["model_cfg"]), s["ckpt_file"], mel_spec_type=s["vocoder_name"],
                         vocab_file=s["vocab_file"], device=s["device"], **family)
    if s["mode"] == "vc":
        return main_vc(s, mc, model, vocoder)
    rank = {}
    if args.best_of > 1 or args.seed is not None:
        rank = dict(best_of=args.best_of, seed=args.seed, report=[])
        if args.best_of > 1:
            from ..ppg.ctc_align import CTCAligner
            rank["scorer"] = CTCAligner(args.asr_model, args.asr_config, args.asr_dict, s["device"], asr=True)
            rank["scorer"].warm()
    voices = dict(config.get("voices", {}))
    voices["main"] = {"ref_audio": s["ref_audio"], "ref_text": s["ref_text"]}
    transcriber = None
    if args.whisper_dir and any(not v["ref_text"].strip() for v in voices.values()):
        from ..eval.whisper import WhisperRecognizer
        prompt = {} if args.whisper_prompt is None else dict(long_form=True, initial_prompt=args.whisper_prompt)
        if args.whisper_assistant is not None:
            prompt["assistant_dir"] = args.whisper_assistant
        if args.whisper_step_graph:
            prompt["step_graph"] = True
        if args.whisper_weights != "f32":
            prompt["weights"] = args.whisper_weights
        transcriber = WhisperRecognizer(args.whisper_dir, s["device"], args.ref_language, beam_size=args.whisper_beam, **prompt)
    for v in voices.values():   # reference infer_cli.py:297-303
        v["ref_audio"], v["ref_text"] = U.preprocess_ref_audio_text(v["ref_audio"], v["ref_text"], transcriber=transcriber)
    segments = []
    for voice, text in split_voices(s["gen_text"]):
        v = voices.get(voice, voices["main"])
        seg, sr, _ = U.infer_process(v["ref_audio"], v["ref_text"], text, model, vocoder,
                                     mel_spec_type=s["vocoder_name"], target_rms=s["target_rms"],
                                     cross_fade_duration=s["cross_fade_duration"], nfe_step=s["nfe_step"],
                                     cfg_strength=s["cfg_strength"], sway_sampling_coef=s["sway_sampling_coef"],
                                     speed=s["speed"], fix_duration=s["fix_duration"], device=s["device"],
                                     mode=s["mode"], alpha_spk=s["alpha_spk"], alpha_txt=s["alpha_txt"], **rank)
        if rank.get("seed") is not None:    # the next [voice] segment goes on where this one's chunks stopped
            rank["seed"] = next_segment_seed(rank["seed"], len(rank["report"]), args.best_of)
            rank["report"].clear()
        segments.append(seg)
        if s["save_chunk"]:
            os.makedirs(os.path.join(s["output_dir"], "chunks"), exist_ok=True)
            U.save_wav(os.path.join(s["output_dir"], "chunks", f"{len(segments) - 1}.wav"), seg, sr)
    if segments:
        os.makedirs(s["output_dir"], exist_ok=True)
        path = os.path.join(s["output_dir"], s["output_file"])
        U.save_wav(path, np.concatenate(segments), U.target_sample_rate)
        if s["remove_silence"]:
            U.remove_silence_for_generated_wav(path)
        print(path)


def main_vc(s: dict, mc: dict, model, vocoder):
    """--mode vc: the content of --source_audio in the voice of --ref_audio, one wav out."""
    from ..ppg import PPGModelWapper
    fc = mc["frontend_ppg_config"]
    ppg_front = PPGModelWapper(s["ppg_model"] or fc["model_path"], s["ppg_config"] or fc["config"], s["device"],
                               output_type=fc["output_type"], ppg_frame_length=fc["frame_length"],
                               mel_f_shift=fc["mel_frame_shift"], map_mix_ratio=fc["map_mix_ratio"],
                               global_phn_center_path=fc["global_phn_center_path"],
                               para_softmax_path=fc["para_softmax_path"], stream=s["ppg_stream"])
    wave, sr, _ = U.infer_vc_process(s["ref_audio"], s["source_audio"], model, vocoder, ppg_front,
                                     mel_spec_type=s["vocoder_name"], target_rms=s["target_rms"],
                                     cross_fade_duration=s["cross_fade_duration"], nfe_step=s["nfe_step"],
                                     alpha_spk=s["alpha_spk"], alpha_ppg=s["alpha_ppg"],
                                     sway_sampling_coef=s["sway_sampling_coef"], speed=s["speed"], device=s["device"])
    if wave is None:
        raise SystemExit("--mode vc: the source audio is too short to convert")
    os.makedirs(s["output_dir"], exist_ok=True)
    path = os.path.join(s["output_dir"], s["output_file"])
    U.save_wav(path, wave, sr)
    if s["remove_silence"]:
        U.remove_silence_for_generated_wav(path)
    print(path)


if __name__ == "__main__":
    main()
