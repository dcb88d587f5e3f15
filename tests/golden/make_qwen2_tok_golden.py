"""Makes tests/golden/qwen2_tok/ with ``tokenizers`` (0.22.2 when this was run): a small byte-level BPE trained offline with the NFC
normaliser, Qwen2's pre-tokeniser pattern and the three ChatML specials (ids 381 .. 383, so the vocabulary fits the tiny model of
qwen2.npz).  Files: ``vocab.json``, ``merges.txt``, ``tokenizer_config.json`` (``added_tokens_decoder``) and ``cases.json``: the
ids the trained tokeniser gives for strings that cover contractions, digits, CJK, runs of newlines and spaces, specials inside
text, a decomposed accent and a rendered conversation.

    python tests/golden/make_qwen2_tok_golden.py
"""
import json
import os

PATTERN = (r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+")
SPECIALS = ("<|endoftext|>", "<|im_start|>", "<|im_end|>")
CORPUS = [
    "the quick brown fox jumps over the lazy dog and then the dog runs away from the fox",
    "you are a helpful assistant and the user is asking the assistant a question about the weather",
    "I'm sure it's fine, they're here and we've done what you'll need; he'd say don't",
    "system user assistant system user assistant hello hello there how are you today",
    "numbers 123 4567 2024 and 3.14159 are written with digits 0 1 2 3 4 5 6 7 8 9",
    "你好，世界。今天天气很好。 你好吗？ 我很好。",
    "line one\nline two\n\nline four\r\n   indented   spaces\t\ttabs",
    "café naïve résumé über straße ¿qué? ¡sí!",
] * 4
CASES = [
    "Hello, world!", "I'm sure it's fine; they're here, we've done it, you'll see, he'd say DON'T.", "I'M HERE AND HE'LL GO",
    "1234567890 and 3.14", "year 2024, 12:30pm", "你好，世界。", "今天天气很好 ok", "a\nb", "a\n\n\nb", "a \n b", "  two  spaces  ",
    "trailing spaces   ", "\ttab\tseparated", "line\r\nfeed", "x   \n\n   y", "", " ", "\n", "...", "!!! ???", "(parens) [brackets] {braces}",
    "snake_case and kebab-case", "é decomposed becomes é", "café", "über straße", "emoji \U0001F600 here",
    "<|im_start|>user\nhi<|im_end|>\n", "text<|endoftext|>more text", "<|im_start|><|im_end|>", "almost <|im_start special",
    "<|im_start|>system\nYou are a helpful assistant.<|im_end|>\n<|im_start|>user\nWhat's 2+2?<|im_end|>\n<|im_start|>assistant\n",
    "the quick brown fox", "The Quick Brown Fox", "don't can't won't", "It's 5 o'clock", "a1b2c3", "mixed 你好 and hello",
    "tabs\t\tand  spaces", "end with newline\n", "\n\nstart with newlines", "hello   \n", "price: $4.99!",
]


def main():
    from tokenizers import Regex, Tokenizer, models, normalizers, pre_tokenizers, trainers
    tok = Tokenizer(models.BPE())
    tok.normalizer = normalizers.NFC()
    tok.pre_tokenizer = pre_tokenizers.Sequence([pre_tokenizers.Split(Regex(PATTERN), behavior="isolated", invert=False),
                                                 pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)])
    trainer = trainers.BpeTrainer(vocab_size=381, special_tokens=[], initial_alphabet=pre_tokenizers.ByteLevel.alphabet(),
                                  show_progress=False)
    tok.train_from_iterator(CORPUS, trainer)
    assert tok.get_vocab_size() == 381, tok.get_vocab_size()
    tok.add_special_tokens(list(SPECIALS))
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "qwen2_tok")
    os.makedirs(out, exist_ok=True)
    tok.model.save(out)
    with open(os.path.join(out, "tokenizer_config.json"), "w") as f:
        json.dump(dict(added_tokens_decoder={str(tok.token_to_id(s)): dict(content=s, special=True) for s in SPECIALS},
                       eos_token="<|im_end|>", pad_token="<|endoftext|>"), f, indent=1)
    with open(os.path.join(out, "cases.json"), "w") as f:
        json.dump([dict(text=c, ids=tok.encode(c).ids) for c in CASES], f, ensure_ascii=True, indent=0)
    print(tok.get_vocab_size(), [tok.token_to_id(s) for s in SPECIALS], len(CASES), "cases")


if __name__ == "__main__":
    main()
