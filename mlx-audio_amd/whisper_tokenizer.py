"""A decode-only tokenizer for Whisper's transcripts: ids -> text, which is all the transcription loop needs of
mlx_audio/stt/models/whisper/tokenizer.py (`Tokenizer.decode`, :166-168: the special tokens and timestamps are dropped, the rest goes through the
byte-pair vocabulary).  The vocabulary is a tiktoken-format rank file -- one `base64(token bytes) rank` pair per line, as `multilingual.tiktoken` and
`gpt2.tiktoken` are -- that the CALLER names: no vocabulary file is part of this repository.  Decoding a byte-pair vocabulary is a table lookup and a
join; it needs nothing of the tiktoken package.  Text-to-id encoding is not built: prompts go in as token ids."""
from __future__ import annotations

import base64
from typing import Dict, Iterable


class Tokenizer:
    def __init__(self, ranks: Dict[int, bytes], eot: int):
        self.ranks, self.eot = ranks, int(eot)

    @classmethod
    def from_file(cls, path, dims) -> "Tokenizer":
        """path: the rank file; dims: the model's ModelDimensions (they fix `eot`, below which the text tokens lie)"""
        from .whisper_decoding import special_tokens

        ranks: Dict[int, bytes] = {}
        with open(path, "rb") as f:
            for n, line in enumerate(f, 1):
                line = line.strip()
                if not line:
                    continue
                parts = line.split()
                try:
                    if len(parts) != 2:
                        raise ValueError("expected two fields")
                    token, rank = base64.b64decode(parts[0], validate=True), int(parts[1])
                except ValueError as e:  # (binascii.Error is a ValueError)
                    raise ValueError(f"{path}: line {n} is not `base64 rank`: {e}") from None
                if rank < 0 or rank in ranks:
                    raise ValueError(f"{path}: line {n}: rank {rank} is negative or appears twice")
                ranks[rank] = token
        if not ranks:
            raise ValueError(f"{path}: no ranks")
        return cls(ranks, special_tokens(dims).eot)

    def decode_bytes(self, ids: Iterable[int]) -> bytes:
        out = []
        for t in ids:
            t = int(t)
            if t >= self.eot:  # special tokens and timestamps carry no text
                continue
            if t not in self.ranks:
                raise ValueError(f"token id {t} is not in the vocabulary file")
            out.append(self.ranks[t])
        return b"".join(out)

    def decode(self, ids: Iterable[int]) -> str:
        """the byte strings of the ids below `eot`, joined, as UTF-8; bytes that form no character become U+FFFD"""
        return self.decode_bytes(ids).decode("utf-8", errors="replace")
