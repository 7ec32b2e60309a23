"""The tokenizer of the CLIP text tower: open_clip's SimpleTokenizer algorithm (public; byte-level BPE over lower-cased text).

  vocabulary   256 byte symbols (the GPT-2 byte -> unicode map), the same with `</w>`, one symbol per merge of the BPE file (its first
               48 894 merges, header line skipped), then `<|startoftext|>` and `<|endoftext|>`
  cleaning     html.unescape twice, strip, whitespace runs -> one space, lower case.  open_clip first passes the text through
               `ftfy.fix_text`, which is not used here: it is the identity on ASCII text (every name of the scale table is ASCII) —
               the ONE cleaning deviation
  encoding     split by the pattern below, bytes -> symbols, greedy lowest-rank merges, ids
  batch        [N, context_length] int64 = BOS, tokens, EOS, zero padding; a longer prompt is cut and its last id forced to EOS

The merges file (`bpe_simple_vocab_16e6.txt.gz`, shipped inside the open_clip package) is NOT part of this repository: its path comes
from the argument or FREEPOSE_CLIP_BPE, as `.txt.gz` or `.txt`.  There is no fallback vocabulary.
"""
from __future__ import annotations

import gzip
import html
import os
from functools import lru_cache
from pathlib import Path

import regex as re
import torch

BPE_ENV = "FREEPOSE_CLIP_BPE"
N_MERGES = 49152 - 256 - 2          # 48 894: what open_clip keeps of the file
SPLIT_PATTERN = r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+"""


@lru_cache()
def bytes_to_unicode() -> dict:
    """GPT-2's reversible byte -> printable unicode character map"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(2 ** 8):
        if b not in bs:
            bs.append(b)
            cs.append(2 ** 8 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


def clean_text(text: str) -> str:
    text = html.unescape(html.unescape(text)).strip()
    return re.sub(r"\s+", " ", text).strip().lower()


def read_merges(path) -> list:
    """the merges of a BPE file (`.txt.gz` or `.txt`): one `a b` pair per line after the header line, at most N_MERGES of them"""
    p = Path(path)
    if not p.is_file():
        raise FileNotFoundError(f"CLIP BPE merges file {p} not found: pass its path or set {BPE_ENV} (it is open_clip's "
                                "bpe_simple_vocab_16e6.txt.gz, found inside the open_clip package; it is not shipped here)")
    raw = gzip.open(p).read() if p.suffix == ".gz" else p.read_bytes()
    lines = raw.decode("utf-8").split("\n")[1:1 + N_MERGES]
    return [tuple(ln.split()) for ln in lines if ln.strip()]


class SimpleTokenizer:
    def __init__(self, bpe_path=None, context_length: int = 77):
        bpe_path = bpe_path or os.environ.get(BPE_ENV)
        if not bpe_path:
            raise FileNotFoundError(f"CLIP BPE merges file not given: pass its path or set {BPE_ENV} (it is open_clip's "
                                    "bpe_simple_vocab_16e6.txt.gz, found inside the open_clip package; it is not shipped here)")
        merges = read_merges(bpe_path)
        self.byte_encoder = bytes_to_unicode()
        vocab = list(self.byte_encoder.values())
        vocab = vocab + [v + "</w>" for v in vocab] + ["".join(m) for m in merges] + ["<|startoftext|>", "<|endoftext|>"]
        self.encoder = dict(zip(vocab, range(len(vocab))))
        self.bpe_ranks = dict(zip(merges, range(len(merges))))
        self.cache = {"<|startoftext|>": "<|startoftext|>", "<|endoftext|>": "<|endoftext|>"}
        self.pat = re.compile(SPLIT_PATTERN, re.IGNORECASE)
        self.vocab_size = len(self.encoder)
        self.sot_token_id = self.encoder["<|startoftext|>"]
        self.eot_token_id = self.encoder["<|endoftext|>"]
        self.context_length = int(context_length)

    def bpe(self, token: str) -> str:
        """the symbols of one word after all applicable merges, joined by spaces (lowest rank first, every occurrence of the pair)"""
        if token in self.cache:
            return self.cache[token]
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        while len(word) > 1:
            pairs = set(zip(word[:-1], word[1:]))
            bigram = min(pairs, key=lambda pair: self.bpe_ranks.get(pair, float("inf")))
            if bigram not in self.bpe_ranks:
                break
            first, second = bigram
            merged, i = [], 0
            while i < len(word):
                if i + 1 < len(word) and word[i] == first and word[i + 1] == second:
                    merged.append(first + second)
                    i += 2
                else:
                    merged.append(word[i])
                    i += 1
            word = tuple(merged)
        out = " ".join(word)
        self.cache[token] = out
        return out

    def encode(self, text: str) -> list:
        ids = []
        for token in re.findall(self.pat, clean_text(text)):
            token = "".join(self.byte_encoder[b] for b in token.encode("utf-8"))
            ids.extend(self.encoder[sym] for sym in self.bpe(token).split(" "))
        return ids

    def __call__(self, texts, context_length: int | None = None) -> torch.Tensor:
        if isinstance(texts, str):
            texts = [texts]
        n = int(context_length or self.context_length)
        out = torch.zeros((len(texts), n), dtype=torch.long)
        for i, text in enumerate(texts):
            ids = [self.sot_token_id] + self.encode(text) + [self.eot_token_id]
            if len(ids) > n:
                ids = ids[:n]
                ids[-1] = self.eot_token_id
            out[i, :len(ids)] = torch.tensor(ids, dtype=torch.long)
        return out
