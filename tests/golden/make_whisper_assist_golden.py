"""Makes tests/golden/whisper_assist.npz from ``transformers`` (5.15.0 when this was run): assisted generation (speculative
decoding) on the tiny model, wave and cases of tests/golden/whisper.npz -- nothing is downloaded.

Draft: a seeded ``WhisperForConditionalGeneration`` of ANOTHER width with its own encoder (d_model 32, 1 + 1 layers, 2 heads, ffn 64;
the target's vocabulary, mel bins, positions and suppress lists), scaled and rounded to bf16-representable values the way
make_whisper_golden.py treats the target.  Its weights are stored (``w/<name>``, the upper 16 bits), with its ``config_json``.

Per case (the 0.9 s, 2.5 s and 3 s prefixes of the wave, and the 0.9 s prefix on the model whose <|endoftext|> row is scaled so that
it ends by itself): ``GenerationMixin.generate(model, features, decoder_input_ids=prompt, assistant_model=draft, do_sample=False,
max_new_tokens=M)`` with the assistant's generation config set to ``num_assistant_tokens = 4``, ``num_assistant_tokens_schedule =
"constant"`` and ``assistant_confidence_threshold = 0.0``.  M = 48 - 4 - 4 keeps prompt + new tokens + drafts within the 48 target
positions of the TARGET.

``transformers`` 5.15.0 feeds a Whisper assistant at drifting positions: every round its ``generate`` is handed the whole sequence
behind a cache that was not cropped to it, so the draft's position ids start further out each round (6, 13, 21, 30, 40, ... on
this model) and run off a 48-row position table in the sixth round, whatever ``max_new_tokens`` is.  The run here therefore uses
a copy of the draft whose position table is extended to ``RUN_POSITIONS`` rows (rows 0 .. 47 are the stored draft's, the rest
seeded noise).  The copy's ``generate`` is ``GenerationMixin.generate`` as well: ``WhisperGenerationMixin.generate`` resets the begin
index of the logits processors it is handed, and the candidate generator hands the assistant the TARGET's processor objects, so
with it ``begin_suppress_tokens`` (<|endoftext|> among them) would be banned at the first position of every round and a
sequence would never end.  Both changes alter what the draft proposes at most, not what comes out: in greedy assisted generation the returned tokens are
the target's own for ANY draft, which is what is recorded and asserted -- the returned tokens equal the plain greedy tokens of
whisper.npz cut at the bound, and the float64 restatement tests/whisper_assist_ref.py reproduces them with the STORED draft (48
positions, fed at the right ones).

    python tests/golden/make_whisper_assist_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_whisper_golden as MG        # noqa: E402
import whisper_assist_ref as AR         # noqa: E402
import whisper_ref as WR                # noqa: E402

NUM_ASSISTANT_TOKENS = 4
DRAFT_SEED = 4242
RUN_POSITIONS = 2048   # the position table of the copy of the draft that ``transformers`` runs (see the module text)


def draft_config():
    from transformers import WhisperConfig
    return WhisperConfig(
        vocab_size=160, num_mel_bins=128, d_model=32, encoder_layers=1, decoder_layers=1, encoder_attention_heads=2,
        decoder_attention_heads=2, encoder_ffn_dim=64, decoder_ffn_dim=64, max_source_positions=150,
        max_target_positions=MG.MAX_TARGET, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, encoder_layerdrop=0.0,
        decoder_layerdrop=0.0, pad_token_id=MG.EOS, bos_token_id=MG.EOS, eos_token_id=MG.EOS, decoder_start_token_id=MG.SOT,
        suppress_tokens=MG.SUPPRESS, begin_suppress_tokens=MG.BEGIN_SUPPRESS)


def build_draft():
    from transformers import WhisperForConditionalGeneration
    torch.manual_seed(DRAFT_SEED)
    model = WhisperForConditionalGeneration(draft_config()).eval()
    g = torch.Generator().manual_seed(DRAFT_SEED + 1000)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name == "model.decoder.embed_positions.weight":
                p.copy_(torch.randn(p.shape, generator=g))
            elif name == "model.encoder.embed_positions.weight":
                pass
            elif "layer_norm" in name:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            elif p.ndim >= 2:
                p.mul_(6.0)
        emb = model.model.decoder.embed_tokens.weight
        emb[MG.EOS] = emb[:MG.N_SPECIAL0].std() * torch.randn(emb.shape[1], generator=g)
        for p in model.parameters():
            p.copy_(p.bfloat16().float())
    return model


def run_copy(draft):
    """The draft with its position table extended to RUN_POSITIONS rows (module text): what ``transformers`` is handed."""
    from transformers import WhisperForConditionalGeneration
    from transformers.generation import GenerationMixin

    class PlainGenerate(WhisperForConditionalGeneration):
        generate = GenerationMixin.generate

    cfg = draft_config()
    cfg.max_target_positions = RUN_POSITIONS
    big = PlainGenerate(cfg).eval()
    sd = {k: v.clone() for k, v in draft.state_dict().items()}
    pos = torch.randn(RUN_POSITIONS, cfg.d_model, generator=torch.Generator().manual_seed(DRAFT_SEED + 2000))
    pos[:MG.MAX_TARGET] = sd["model.decoder.embed_positions.weight"]
    sd["model.decoder.embed_positions.weight"] = pos
    big.load_state_dict(sd, strict=True)
    return big


def load_target(fx, eos_case):
    """The target of whisper.npz as a ``transformers`` model (``eos_case``: with the scaled <|endoftext|> row)."""
    from transformers import GenerationConfig, WhisperForConditionalGeneration
    model = WhisperForConditionalGeneration(MG.hf_config()).eval()
    sd = {k: torch.from_numpy(np.array(v)) for k, v in fx["sd"].items()}
    if eos_case:
        sd["model.decoder.embed_tokens.weight"][MG.EOS] = torch.from_numpy(np.array(fx["eos_row_f32"]))
    sd["proj_out.weight"] = sd["model.decoder.embed_tokens.weight"]
    model.load_state_dict(sd, strict=True)
    model.generation_config = GenerationConfig(**MG.generation_config_dict())
    return model


def assisted(model, draft, feats, prompt, max_new):
    from transformers import GenerationConfig
    from transformers.generation import GenerationMixin
    draft.generation_config = GenerationConfig(**MG.generation_config_dict())
    draft.generation_config.num_assistant_tokens = NUM_ASSISTANT_TOKENS
    draft.generation_config.num_assistant_tokens_schedule = "constant"
    draft.generation_config.assistant_confidence_threshold = 0.0
    with torch.no_grad():
        out = GenerationMixin.generate(model, feats, decoder_input_ids=torch.tensor([prompt]), assistant_model=draft,
                                       do_sample=False, max_new_tokens=max_new)
    out = out[0].tolist()
    return out if out[:len(prompt)] == list(prompt) else list(prompt) + out


def main():
    from transformers import WhisperFeatureExtractor
    fx = WR.load_fixture()
    fe = WhisperFeatureExtractor(feature_size=128, chunk_length=3)
    wave, prompt = fx["wave_f32"], [int(t) for t in fx["prompt"]]
    max_new = MG.MAX_TARGET - len(prompt) - NUM_ASSISTANT_TOKENS
    draft = build_draft()
    runner = run_copy(draft)
    dsd = {k: v.detach().numpy() for k, v in draft.state_dict().items() if k != "proj_out.weight"}
    dcfg = draft_config().to_dict()
    gen = fx["generation_config"]
    cases = []
    for name, n, eos_case in [(str(int(n)), int(n), False) for n in fx["cases"]] + [("eos", int(fx["cases"][0]), True)]:
        model = load_target(fx, eos_case)
        feats = torch.from_numpy(fe(wave[:n], sampling_rate=16000, return_tensors="np").input_features)
        got = assisted(model, runner, feats, prompt, max_new)
        plain = [int(t) for t in fx["tokens_" + name]][:len(prompt) + max_new]
        while len(got) > len(plain) and got[-1] == MG.EOS:              # padding behind the end
            got.pop()
        if plain[-1] == MG.EOS and got == plain[:-1]:                   # returned without the closing eos
            got = got + [MG.EOS]
        assert got == plain, (name, got, plain)
        # the restatement, with this draft
        tsd = dict(fx["sd"])
        if eos_case:
            emb = tsd["model.decoder.embed_tokens.weight"].copy()
            emb[MG.EOS] = fx["eos_row_f32"]
            tsd["model.decoder.embed_tokens.weight"] = emb
        ref, dref = WR.Ref(tsd, fx["config"]), WR.Ref(dsd, dcfg)
        f64 = feats[0].t().double().numpy()
        rows, _, stats, adv = AR.assisted_ref(AR.model_fn(ref, [ref.encoder(f64)]), AR.model_fn(dref, [dref.encoder(f64)]), [prompt],
                                             len(prompt) + max_new, NUM_ASSISTANT_TOKENS, MG.EOS, AR.plain_pick(gen))
        assert rows[0] == got, (name, rows[0], got)
        print(name, len(got), stats, adv)
        cases.append(dict(name=name, samples=n, eos_case=eos_case, max_new_tokens=max_new, tokens=got, ref_stats=stats))
    out = {"config_json": np.array(json.dumps(dcfg)), "cases_json": np.array(json.dumps(cases)),
           "num_assistant_tokens": np.int32(NUM_ASSISTANT_TOKENS), "seed": np.int32(DRAFT_SEED)}
    for k, v in draft.state_dict().items():
        if k != "proj_out.weight":
            out["w/" + k] = MG.bf16_bits(v)
    path = os.path.join(HERE, "whisper_assist.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
