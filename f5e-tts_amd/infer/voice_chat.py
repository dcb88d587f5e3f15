"""Voice chat: the reference's third mode (infer_gradio.py "Voice Chat") without the UI.  The user speaks or types; a spoken
message is transcribed with Whisper (the ``transcriber=`` path of ``preprocess_ref_audio_text``), the chat model answers
(``infer/qwen2.py``), and the answer is spoken in the reference voice with ``infer_process``.

    python -m f5e_tts_amd.infer.voice_chat --chat_model DIR [--chat_weights auto] --ref_audio ref.wav --ref_text "..." \\
        --input_text "Hello" --input_text "And then?" [--input_audio q.wav --whisper_dir DIR] --output_dir out

writes ``turn_NN.wav`` per turn and ``conversation.json``.  Deviations from the reference, which are DESIGN 4s's: the session
keeps the chat model's caches across turns and prefills only a turn's new text; an empty reply skips synthesis and returns an
empty wave (the reference would fail inside ``infer``)."""
from __future__ import annotations

import argparse
import json
import os
import tempfile
from typing import List, Optional, Tuple

import numpy as np

# the reference's defaults: the system prompt of its UI (infer_gradio.py:811) and the three arguments of its generate call
DEFAULT_SYSTEM_PROMPT = ("You are not an AI assistant, you are whoever the user says you are. You must stay in character. Keep your "
                         "responses concise since they will be spoken out loud.")
MAX_NEW_TOKENS, TEMPERATURE, TOP_P = 512, 0.7, 0.95
CROSS_FADE, SPEED = 0.15, 1.0


class VoiceChat:
    """``chat``: a ``qwen2.Qwen2`` with its tokenizer (or anything with ``ChatSession``'s ``say`` / ``clear`` / ``messages`` when
    ``session=`` is given).  ``model_obj`` / ``vocoder``: what ``infer_process`` takes.  ``transcriber``: anything with
    ``transcribe(wav_path) -> str``; needed for spoken messages only."""

    def __init__(self, chat, model_obj, vocoder, ref_audio: str, ref_text: str, transcriber=None,
                 system_prompt: str = DEFAULT_SYSTEM_PROMPT, max_new_tokens: int = MAX_NEW_TOKENS, greedy: bool = False,
                 temperature: float = TEMPERATURE, top_p: float = TOP_P, step_graph: bool = False, remove_silence: bool = False,
                 session=None, infer_kwargs: Optional[dict] = None):
        from . import utils_infer as U
        if session is None:
            from .qwen2 import ChatSession
            session = ChatSession(chat, system_prompt)
        self.session, self.model_obj, self.vocoder, self.transcriber = session, model_obj, vocoder, transcriber
        self.max_new_tokens, self.step_graph, self.remove_silence = int(max_new_tokens), bool(step_graph), bool(remove_silence)
        self.gen = dict(do_sample=False) if greedy else dict(do_sample=True, temperature=float(temperature), top_p=float(top_p))
        self.infer_kwargs = dict(infer_kwargs or {})
        self.ref_audio, self.ref_text = U.preprocess_ref_audio_text(ref_audio, ref_text, transcriber=transcriber)
        self.turns = 0

    def clear(self) -> None:
        self.session.clear()
        self.turns = 0

    @property
    def conversation(self) -> List[dict]:
        return list(self.session.messages)

    def hear(self, audio: str) -> str:
        """A spoken message -> its text (the reference transcribes it with ``preprocess_ref_audio_text``)."""
        from . import utils_infer as U
        if self.transcriber is None:
            raise RuntimeError("VoiceChat: a spoken message needs a transcriber (--whisper_dir)")
        _, text = U.preprocess_ref_audio_text(audio, "", transcriber=self.transcriber)
        return text.strip()

    def say(self, text: Optional[str] = None, audio: Optional[str] = None, seed: Optional[int] = None
            ) -> Optional[Tuple[str, np.ndarray, int]]:
        """One turn -> (reply_text, wave, sample_rate); None for an empty message, as the reference returns nothing."""
        from . import utils_infer as U
        if (text is None or not text.strip()) and audio:
            text = self.hear(audio)
        if text is None or not text.strip():
            return None
        reply = self.session.say(text.strip(), self.max_new_tokens, seed=self.turns if seed is None else int(seed),
                                 step_graph=self.step_graph, **self.gen)
        self.turns += 1
        if not reply.strip():
            return reply, np.zeros(0, dtype=np.float32), U.target_sample_rate
        wave, sr, _ = U.infer_process(self.ref_audio, self.ref_text, reply, self.model_obj, self.vocoder,
                                      cross_fade_duration=CROSS_FADE, speed=SPEED, **self.infer_kwargs)
        wave = np.asarray(wave, dtype=np.float32)
        if self.remove_silence:
            with tempfile.NamedTemporaryFile(suffix=".wav", delete=False) as f:
                path = f.name
            try:
                U.save_wav(path, wave, sr)
                U.remove_silence_for_generated_wav(path)
                wave = U.load_wav(path)[0][0].numpy()
            finally:
                os.unlink(path)
        return reply, wave, sr


def build_parser() -> argparse.ArgumentParser:
    from .infer_cli import build_parser as cli_parser
    p = cli_parser()
    p.prog = "python3 -m f5e_tts_amd.infer.voice_chat"
    p.description = "Voice chat: Whisper -> Qwen2 -> speech in the reference voice, turn by turn."
    p.add_argument("--chat_model", type=str, required=True, help="A Qwen2 checkpoint directory (config.json, safetensors, tokenizer)")
    p.add_argument("--chat_weights", type=str, default="auto", choices=["auto", "bf16", "fp16", "f32"])
    p.add_argument("--input_text", dest="turns", action=_Turn, help="A typed message; repeatable, turns in order")
    p.add_argument("--input_audio", dest="turns", action=_Turn, help="A spoken message (wav); repeatable, turns in order")
    p.add_argument("--system_prompt", type=str, default=DEFAULT_SYSTEM_PROMPT)
    p.add_argument("--max_new_tokens", type=int, default=MAX_NEW_TOKENS)
    p.add_argument("--temperature", type=float, default=TEMPERATURE)
    p.add_argument("--top_p", type=float, default=TOP_P)
    p.add_argument("--greedy", action="store_true", help="The arg max instead of sampling")
    p.add_argument("--chat_seed", type=int, default=0, help="Turn t draws with seed chat_seed + t")
    p.add_argument("--chat_step_graph", action="store_true", help="Replay one captured decode step per token")
    return p


class _Turn(argparse.Action):
    """--input_text / --input_audio share one list, so the turns keep the order of the command line."""

    def __call__(self, parser, ns, value, option_string=None):
        turns = list(getattr(ns, "turns", None) or [])
        turns.append(("audio" if option_string == "--input_audio" else "text", value))
        ns.turns = turns


def run_turns(vc: VoiceChat, turns, output_dir: str, seed: int = 0, save_wav=None) -> List[dict]:
    """Every turn through ``vc``: ``turn_NN.wav`` and ``conversation.json`` under ``output_dir`` -> the conversation."""
    from . import utils_infer as U
    save_wav = save_wav or U.save_wav
    os.makedirs(output_dir, exist_ok=True)
    for t, (kind, value) in enumerate(turns):
        res = vc.say(**{kind: value}, seed=seed + t)
        if res is None:
            continue
        reply, wave, sr = res
        if len(wave):
            save_wav(os.path.join(output_dir, f"turn_{t:02d}.wav"), wave, sr)
    conv = vc.conversation
    with open(os.path.join(output_dir, "conversation.json"), "w", encoding="utf-8") as f:
        json.dump(conv, f, ensure_ascii=False, indent=1)
    return conv


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not args.turns:
        raise SystemExit("voice_chat: give at least one --input_text or --input_audio")
    if any(k == "audio" for k, _ in args.turns) and not args.whisper_dir:
        raise SystemExit("voice_chat: --input_audio needs --whisper_dir")
    from . import utils_infer as U
    from .infer_cli import DEFAULT_VOCODER_PATH, load_arch, resolve_settings
    from .qwen2 import Qwen2
    from ..model import DiT
    config = {}
    if args.config:
        import tomli
        with open(args.config, "rb") as f:
            config = tomli.load(f)
    s = resolve_settings(args, config)
    vocoder = U.load_vocoder(s["vocoder_name"], is_local=True,
                             local_path=config.get("vocoder_local_path", DEFAULT_VOCODER_PATH[s["vocoder_name"]]), device=s["device"])
    model = U.load_model(DiT, load_arch(s["model"], s["model_cfg"]), s["ckpt_file"], mel_spec_type=s["vocoder_name"],
                         vocab_file=s["vocab_file"], device=s["device"])
    transcriber = None
    if args.whisper_dir:
        from ..eval.whisper import WhisperRecognizer
        transcriber = WhisperRecognizer(args.whisper_dir, s["device"], args.ref_language)
    chat = Qwen2.from_pretrained_dir(args.chat_model, args.chat_weights, s["device"])
    vc = VoiceChat(chat, model, vocoder, s["ref_audio"], s["ref_text"], transcriber, args.system_prompt, args.max_new_tokens,
                   args.greedy, args.temperature, args.top_p, args.chat_step_graph, s["remove_silence"],
                   infer_kwargs=dict(mel_spec_type=s["vocoder_name"], target_rms=s["target_rms"], nfe_step=s["nfe_step"],
                                     cfg_strength=s["cfg_strength"], sway_sampling_coef=s["sway_sampling_coef"], device=s["device"]))
    run_turns(vc, args.turns, s["output_dir"], args.chat_seed)
    print(os.path.join(s["output_dir"], "conversation.json"))


if __name__ == "__main__":
    main()
