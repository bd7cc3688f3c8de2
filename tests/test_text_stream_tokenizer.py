"""ByteLevelBPE.incremental(): the ids of a text fed piece by piece equal encode(whole text) for every way of cutting it,
and feed() never returns an id that a continuation (or finish()) would have to take back.  The vocabulary is trained as
tests/test_tokenizer.py trains its own; that file pins encode() itself against the `tokenizers` library."""
import json
import random

import pytest

from qwen3_tts_axera_russian_amd.tokenizer import PRETOKENIZE, ByteLevelBPE
from tests.test_tokenizer import CORPUS

SAMPLES = [
    "Привет, как дела? Сегодня хорошая погода.",
    "It's 12:30, isn't it?  We'll see — they've gone, I'm sure. ",
    "Она сказала: «Я приду в 7 часов», — и ушла…  \n\nНовая строка.\tTab.   ",
    "é vs é, й и й, ạ̈ (marks), 각 각 jamo",
    "<|im_start|>assistant\nПривет<|im_end|> <tts_pad><|im_ <3 <|im_start",
    "Числа 1234567890 и 3.14159;  user@example.com   \r\n\r\n  x'l 'L 'Re'",
    "emoji 🙂 and 中文 bytes 42км/ч",
]


@pytest.fixture(scope="module")
def bpe(tmp_path_factory):
    pytest.importorskip("tokenizers")
    from tokenizers import Regex, Tokenizer, decoders, models, normalizers, pre_tokenizers, trainers
    tok = Tokenizer(models.BPE())
    tok.normalizer = normalizers.NFC()
    tok.pre_tokenizer = pre_tokenizers.Sequence([
        pre_tokenizers.Split(Regex(PRETOKENIZE), behavior="isolated", invert=False),
        pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)])
    tok.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=600, initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), special_tokens=[])
    tok.train_from_iterator(CORPUS, trainer)
    specials = ["<|im_start|>", "<|im_end|>", "<tts_pad>"]
    tok.add_special_tokens(specials)
    d = tmp_path_factory.mktemp("tok_stream")
    tok.model.save(str(d))
    added = {str(tok.token_to_id(t)): {"content": t} for t in specials}
    (d / "tokenizer_config.json").write_text(json.dumps({"added_tokens_decoder": added}))
    return ByteLevelBPE.from_dir(str(d))


def _fed(bpe, pieces, want):
    """Feeds the pieces; every feed()'s ids must already be a prefix of the whole text's ids -> all ids."""
    inc, got = bpe.incremental(), []
    for p in pieces:
        got += inc.feed(p)
        assert got == want[:len(got)], (pieces, got, want)
    got += inc.finish()
    assert inc.finish() == []
    return got


@pytest.mark.parametrize("text", SAMPLES)
def test_every_two_piece_split(bpe, text):
    want = bpe.encode(text)
    for i in range(len(text) + 1):
        assert _fed(bpe, [text[:i], text[i:]], want) == want, i
    raw = text.encode("utf-8")
    for i in range(len(raw) + 1):                            # bytes: the cut may fall inside a UTF-8 sequence
        assert _fed(bpe, [raw[:i], raw[i:]], want) == want, i


@pytest.mark.parametrize("text", SAMPLES)
def test_random_multi_splits_and_single_bytes(bpe, text):
    want = bpe.encode(text)
    rnd = random.Random(len(text))
    for _ in range(200):
        cuts = sorted(rnd.randrange(len(text) + 1) for _ in range(rnd.randrange(1, 9)))
        pieces = [text[a:b] for a, b in zip([0] + cuts, cuts + [len(text)])]
        assert _fed(bpe, pieces, want) == want, cuts
    raw = text.encode("utf-8")
    assert _fed(bpe, [raw[i:i + 1] for i in range(len(raw))], want) == want
    assert _fed(bpe, list(text), want) == want


def test_something_is_emitted_before_the_end(bpe):
    """The hold-back is a tail, not the text: all but the last words of a sentence are out before finish()."""
    text = SAMPLES[0]
    inc = bpe.incremental()
    early = inc.feed(text)
    want = bpe.encode(text)
    assert 0 < len(early) < len(want) and len(want) - len(early) <= 3
    assert early + inc.finish() == want
    with pytest.raises(ValueError):
        inc.feed("more")
    cut = bpe.incremental()
    cut.feed("ж".encode("utf-8")[:1])
    with pytest.raises(UnicodeDecodeError):
        cut.finish()                                         # a UTF-8 sequence cut short is an error, not a guess
