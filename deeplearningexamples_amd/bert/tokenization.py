"""WordPiece tokenisation for the BERT command-line tools (the behaviour of LanguageModeling/BERT/tokenization.py: BasicTokenizer
followed by WordpieceTokenizer over a one-token-per-line vocabulary file).

Basic step: invalid / control characters dropped and every whitespace character turned into a space; a space put around every CJK
ideograph; split on whitespace; optionally lower-cased with accents stripped (NFD, combining marks dropped); every punctuation
character split off as a token of its own.  WordPiece step: greedy longest-match-first over the vocabulary, continuation pieces
spelled `##piece`; a word with a stretch that matches nothing, or longer than 100 characters, becomes `[UNK]`.
"""
import collections
import unicodedata


def load_vocab(vocab_file):
    vocab = collections.OrderedDict()
    with open(vocab_file, "r", encoding="utf-8") as f:
        for index, line in enumerate(f):
            vocab[line.strip()] = index
    return vocab


def _is_whitespace(ch):
    return ch in " \t\n\r" or unicodedata.category(ch) == "Zs"


def _is_control(ch):
    if ch in "\t\n\r":
        return False
    return unicodedata.category(ch).startswith("C")


def _is_punctuation(ch):
    cp = ord(ch)
    # every non-alphanumeric ASCII printable counts ("^", "$", "`" included, whatever their Unicode class)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return True
    return unicodedata.category(ch).startswith("P")


def _is_cjk(cp):
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F
            or 0x2B740 <= cp <= 0x2B81F or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF or 0x2F800 <= cp <= 0x2FA1F)


NEVER_SPLIT = ("[UNK]", "[SEP]", "[PAD]", "[CLS]", "[MASK]")


class BasicTokenizer:
    def __init__(self, do_lower_case=True):
        self.do_lower_case = do_lower_case

    def tokenize(self, text):
        chars = []
        for ch in text:
            cp = ord(ch)
            if cp == 0 or cp == 0xFFFD or _is_control(ch):
                continue
            if _is_whitespace(ch):
                chars.append(" ")
            elif _is_cjk(cp):
                chars.extend((" ", ch, " "))
            else:
                chars.append(ch)
        out = []
        for token in "".join(chars).split():
            if token in NEVER_SPLIT:                     # a special token written out in the text stays whole and cased
                out.append(token)
                continue
            if self.do_lower_case:
                token = "".join(c for c in unicodedata.normalize("NFD", token.lower()) if unicodedata.category(c) != "Mn")
            out.extend(self._split_punctuation(token))
        return " ".join(out).split()

    @staticmethod
    def _split_punctuation(token):
        pieces, word = [], []
        for ch in token:
            if _is_punctuation(ch):
                if word:
                    pieces.append("".join(word))
                    word = []
                pieces.append(ch)
            else:
                word.append(ch)
        if word:
            pieces.append("".join(word))
        return pieces


class WordpieceTokenizer:
    def __init__(self, vocab, unk_token="[UNK]", max_input_chars_per_word=100):
        self.vocab, self.unk_token, self.max_chars = vocab, unk_token, max_input_chars_per_word

    def tokenize(self, text):
        out = []
        for word in text.split():
            if len(word) > self.max_chars:
                out.append(self.unk_token)
                continue
            pieces, start = [], 0
            while start < len(word):
                end = len(word)
                piece = None
                while start < end:
                    cand = ("##" if start > 0 else "") + word[start:end]
                    if cand in self.vocab:
                        piece = cand
                        break
                    end -= 1
                if piece is None:
                    pieces = None
                    break
                pieces.append(piece)
                start = end
            out.extend(pieces if pieces is not None else [self.unk_token])
        return out


class BertTokenizer:
    def __init__(self, vocab_file, do_lower_case=True):
        self.vocab = load_vocab(vocab_file)
        self.ids_to_tokens = collections.OrderedDict((i, t) for t, i in self.vocab.items())
        self.basic = BasicTokenizer(do_lower_case)
        self.wordpiece = WordpieceTokenizer(self.vocab)

    def tokenize(self, text):
        out = []
        for token in self.basic.tokenize(text):
            out.extend(self.wordpiece.tokenize(token))
        return out

    def convert_tokens_to_ids(self, tokens):
        return [self.vocab[t] for t in tokens]

    def convert_ids_to_tokens(self, ids):
        return [self.ids_to_tokens[i] for i in ids]


def truncate_pair(tokens_a, tokens_b, max_length):
    """Drop tokens from the end of the longer list (the second on a tie) until the pair fits (extract_features.py)."""
    while len(tokens_a) + len(tokens_b) > max_length:
        (tokens_a if len(tokens_a) > len(tokens_b) else tokens_b).pop()


def build_input(tokenizer, text_a, text_b, seq_length):
    """`text_a` (and `text_b`) -> (tokens, input_ids, input_mask, token_type_ids), each padded to seq_length:
    [CLS] a [SEP] with type 0, then b [SEP] with type 1; a pair is truncated to seq_length - 3, a single text to seq_length - 2."""
    ta = tokenizer.tokenize(text_a)
    tb = tokenizer.tokenize(text_b) if text_b else None
    if tb:
        truncate_pair(ta, tb, seq_length - 3)
    elif len(ta) > seq_length - 2:
        ta = ta[:seq_length - 2]
    tokens = ["[CLS]"] + ta + ["[SEP]"]
    types = [0] * len(tokens)
    if tb:
        tokens += tb + ["[SEP]"]
        types += [1] * (len(tb) + 1)
    ids = tokenizer.convert_tokens_to_ids(tokens)
    pad = seq_length - len(ids)
    return tokens, ids + [0] * pad, [1] * len(ids) + [0] * pad, types + [0] * pad


def parse_line(line):
    """`text` or `text_a ||| text_b` -> (text_a, text_b or None)."""
    line = line.strip()
    if " ||| " in line:                              # the LAST separator splits (a greedy match on the first part)
        a, b = line.rsplit(" ||| ", 1)
        return a, b
    return line, None
