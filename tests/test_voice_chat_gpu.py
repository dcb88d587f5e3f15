"""Voice chat end to end on the GPU (infer/voice_chat.py): the command line with a tiny DiT, a local Vocos and the tiny Qwen2 of
tests/golden/qwen2.npz written out as a checkpoint directory with the tokeniser of tests/golden/qwen2_tok (they share the ids
381 .. 383), two typed turns, greedy.  The two messages were chosen with the float64 restatement (tests/qwen2_ref.py): both
replies are ASCII (the text front-end needs optional packages otherwise) and every step's top-2 gap is >= 2e-2."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import qwen2_ref as Q
from tools import synth as SY

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SYSTEM, TURNS, NEW = "Be brief.", ("ok", "line one"), 12
GEN = dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.8, repetition_penalty=1.05, eos_token_id=[383, 381], pad_token_id=381)


def chat_dir(tmp_path):
    from safetensors.torch import save_file
    fx, sd, cfg = Q.load_fixture()
    d = tmp_path / "chat"
    d.mkdir()
    for f in ("vocab.json", "merges.txt", "tokenizer_config.json"):
        shutil.copy(os.path.join(GOLD, "qwen2_tok", f), d / f)
    (d / "config.json").write_text(json.dumps(dict(cfg["hf"], model_type="qwen2")))
    (d / "generation_config.json").write_text(json.dumps(GEN))
    save_file({k: torch.from_numpy(v.copy()).to(torch.bfloat16) for k, v in sd.items()}, str(d / "model.safetensors"))
    return d


def test_voice_chat_command_line_two_typed_turns(tmp_path):
    import yaml
    from safetensors.torch import save_file

    from f5e_tts_amd.infer import utils_infer as U, voice_chat as VC
    from f5e_tts_amd.infer.qwen2 import ChatSession, Qwen2
    from f5e_tts_amd.model import CFM, DiT
    from f5e_tts_amd.vocoder import Vocos
    arch = dict(dim=1024, depth=2, heads=16, ff_mult=2, text_dim=256, conv_layers=1)
    (tmp_path / "arch.yaml").write_text(yaml.safe_dump({"model": {"arch": dict(arch, checkpoint_activations=False)}}))
    torch.manual_seed(3)
    dit = DiT(**arch, text_num_embeds=2545, mel_dim=100)
    for p in dit.parameters():          # un-zero the AdaLN-zero tensors
        if float(p.detach().abs().max()) == 0:
            torch.nn.init.normal_(p, std=0.02)
    save_file({"ema_model." + k: v.contiguous() for k, v in CFM(transformer=dit).state_dict().items()}, str(tmp_path / "model.safetensors"))
    vdir = tmp_path / "vocos"
    vdir.mkdir()
    (vdir / "config.yaml").write_text(yaml.safe_dump({
        "backbone": {"init_args": dict(input_channels=100, dim=512, intermediate_dim=1536, num_layers=8)},
        "head": {"init_args": dict(dim=512, n_fft=1024, hop_length=256, padding="center")}}))
    torch.save(Vocos().state_dict(), str(vdir / "pytorch_model.bin"))
    U.save_wav(str(tmp_path / "ref.wav"), SY.synthetic_ref_wave(190)[0].numpy() * 3.0, 24000)
    (tmp_path / "cfg.toml").write_text(f'vocoder_local_path = "{vdir}"\nnfe_step = 4\n')
    cdir = chat_dir(tmp_path)
    out = tmp_path / "out"
    VC.main(["-c", str(tmp_path / "cfg.toml"), "-mc", str(tmp_path / "arch.yaml"), "-p", str(tmp_path / "model.safetensors"),
             "-r", str(tmp_path / "ref.wav"), "-s", "A short reference text.", "-o", str(out), "--device", "cuda",
             "--chat_model", str(cdir), "--system_prompt", SYSTEM, "--max_new_tokens", str(NEW), "--greedy",
             "--input_text", TURNS[0], "--input_text", TURNS[1]])
    with open(out / "conversation.json") as f:
        conv = json.load(f)
    assert [m["role"] for m in conv] == ["system", "user", "assistant", "user", "assistant"]
    assert conv[0]["content"] == SYSTEM and (conv[1]["content"], conv[3]["content"]) == TURNS
    # the replies equal Qwen2.generate called directly on the rendered conversation, turn by turn
    m = Qwen2.from_pretrained_dir(str(cdir))
    assert m.weights == "bf16" and m.gen.eos_token_id == (383, 381) and m.gen.repetition_penalty == 1.05
    for upto in (2, 4):
        toks, n = m.generate(conv[:upto], NEW, do_sample=False)
        reply = m.tokenizer.decode_ids(toks[0, :n[0]].tolist())
        assert reply == conv[upto]["content"] and reply.strip() and reply.isascii(), (upto, reply)
    assert conv[2]["content"] != conv[4]["content"]
    for t in (0, 1):
        wave, sr = U.load_wav(str(out / f"turn_{t:02d}.wav"))
        assert sr == 24000 and wave.shape[1] > 2400 and torch.isfinite(wave).all() and float(wave.abs().max()) > 0
    # the session behind the driver: the second turn prefills only its own tokens behind the one that was never fed
    s = ChatSession(m, SYSTEM, positions=128)
    r1 = s.say(TURNS[0], NEW, do_sample=False)
    r2 = s.say(TURNS[1], NEW, step_graph=True, do_sample=False)
    assert (r1, r2) == (conv[2]["content"], conv[4]["content"])
    tok = m.tokenizer
    turn2 = tok.encode(f"\n<|im_start|>user\n{TURNS[1]}<|im_end|>\n<|im_start|>assistant\n")
    first = len(tok.encode(VC_template(SYSTEM, TURNS[0])))
    assert s.prefilled[0] == first and s.prefilled[1] in (1 + len(turn2), 2 + len(turn2)) and s.prefilled[1] < 24
    ids, cached = list(s.ids), s.cached
    with pytest.raises(Exception, match="position cap"):          # a refused turn leaves the session as it was
        s.say("too long", 4096)
    assert (s.ids, s.cached) == (ids, cached) and len(s.messages) == 5


def VC_template(system, user):
    from f5e_tts_amd.infer.qwen2 import apply_chat_template
    return apply_chat_template([dict(role="system", content=system), dict(role="user", content=user)])
