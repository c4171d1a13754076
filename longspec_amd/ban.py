"""Banned sequences and no-repeat n-grams (``ban=`` of the generate loops and the ``begin_*_decode`` entry points).

With ``ban`` set, some next tokens are forbidden given the text so far; their entries of the TARGET's logits become ``-inf`` --
behind the penalties, next to the ``min_tokens`` ban of ``stop=``, in front of the arg-max or draw and of the log-probs.  The
text is then exactly banned decoding of the target, whichever loop produced it; draft passes are untouched.

For a row of target logits let ``t[0 .. m-1]`` be the row's text: the generated columns ``output_ids[z, :w]`` (column 0 being
the prefill's token; the prompt is NOT part of it, nothing matches across the prompt boundary) followed, in a verification
pass, by the draft tokens the row follows -- ``extra_ids[z, c]`` with ``extra_mask[z, r, c] != 0``, in increasing ``c``, which
is path order for the chain and for both level-major trees.  The row predicts ``t[m]``.

* **Sequences.**  For every listed sequence ``s`` of length ``L``: if ``L - 1 <= m`` and ``t[m-L+1 .. m-1] == s[0 .. L-2]``,
  then ``s[L-1]`` is forbidden (``L = 1``: always).
* **No-repeat.**  With ``n = no_repeat_ngram >= 1`` and ``m >= n - 1``: for every ``j`` in ``[n-1, m-1]`` with
  ``t[j-n+1 .. j-1] == t[m-n+1 .. m-1]``, ``t[j]`` is forbidden (``n = 1``: every token of ``t``).
* A forbidden id inside ``[0, V)`` gets the type's ``-inf`` pattern in that row; every other element keeps its bits.  Ids of the
  text outside ``[0, V)`` take part in the comparisons as they are and are never written.  A listed id ``>= V`` is legal and
  bans nothing.  A row in which everything is forbidden is the caller's error.

No state beyond ``output_ids``: nothing is committed or rolled back.  The device side (``ops.ban_rows``) reads one int32 table,
built once per decode state:

    [0] number of sequences   [1] no_repeat_ngram   [2] reserved (0)   [3] TABLE_WORDS
    [4 : 69]      offsets of the sequences into the token area (offset[i + 1] - offset[i] = length of sequence i)
    [69 : 1093]   the sequences' tokens, back to back, padded with -1
"""
from __future__ import annotations

import os

import torch

from .keyword import resolve_keyword

BAN_ENV = "LONGSPEC_BAN"         # "seq=13+13|198+198+198,ngram=4": the process-wide default
MAX_SEQS = 64
MAX_SEQ_LEN = 16
MAX_NGRAM = 16
OFFS_OFF = 4
TOKS_OFF = OFFS_OFF + MAX_SEQS + 1
TABLE_WORDS = TOKS_OFF + MAX_SEQS * MAX_SEQ_LEN


def _token_id(v, what):
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"Ban: {what} {v!r} is not an integer token id")
    if not (0 <= v < 2 ** 31):
        raise ValueError(f"Ban: {what} {v!r} is not a token id (0 .. 2^31 - 1)")
    return v


def _listing(v, what):
    if isinstance(v, (str, bytes)) or not hasattr(v, "__iter__"):
        raise TypeError(f"Ban: {what} must be a sequence of token ids, got {v!r}")
    return tuple(v)


class Ban:
    """``Ban(sequences=(), no_repeat_ngram=0)``: up to 64 banned sequences of 1..16 token ids each, and the length of the
    n-grams that may not occur twice in the generated text (0: off, else 1..16).  At least one of the two."""

    __slots__ = ("sequences", "no_repeat_ngram")

    def __init__(self, sequences=(), no_repeat_ngram=0):
        seqs = []
        for s in _listing(sequences, "sequences"):
            s = tuple(_token_id(v, "sequence token") for v in _listing(s, "a banned sequence"))
            if not (1 <= len(s) <= MAX_SEQ_LEN):
                raise ValueError(f"Ban: a sequence holds 1..{MAX_SEQ_LEN} token ids, got {list(s)!r}")
            seqs.append(s)
        if len(seqs) > MAX_SEQS:
            raise ValueError(f"Ban: at most {MAX_SEQS} sequences, got {len(seqs)}")
        if isinstance(no_repeat_ngram, bool) or not isinstance(no_repeat_ngram, int):
            raise TypeError(f"Ban: no_repeat_ngram must be an integer, got {no_repeat_ngram!r}")
        if not (0 <= no_repeat_ngram <= MAX_NGRAM):
            raise ValueError(f"Ban: no_repeat_ngram must be 0 (off) or 1..{MAX_NGRAM}, got {no_repeat_ngram!r}")
        if not seqs and no_repeat_ngram == 0:
            raise ValueError("Ban: no sequences and no_repeat_ngram = 0 ban nothing")
        self.sequences, self.no_repeat_ngram = tuple(seqs), no_repeat_ngram

    def __repr__(self):
        return f"Ban(sequences={self.sequences}, no_repeat_ngram={self.no_repeat_ngram})"

    def _key(self):
        return (self.sequences, self.no_repeat_ngram)

    def __eq__(self, other):
        return isinstance(other, Ban) and self._key() == other._key()

    def __hash__(self):
        return hash(("Ban",) + self._key())

    def table(self, vocab: int, device):
        """A new int32 [TABLE_WORDS] table of this object on `device` (layout: the module's docstring).  The object keeps no
        tensor: a decode state holds the table of its generation.  An id ``>= vocab`` is legal: it never bans anything."""
        words = [len(self.sequences), self.no_repeat_ngram, 0, TABLE_WORDS]
        offs, toks = [0], []
        for s in self.sequences:
            toks += list(s)
            offs.append(len(toks))
        words += offs + [offs[-1]] * (MAX_SEQS + 1 - len(offs))
        words += toks + [-1] * (MAX_SEQS * MAX_SEQ_LEN - len(toks))
        assert len(words) == TABLE_WORDS
        return torch.tensor(words, dtype=torch.int32).to(device)

    @classmethod
    def parse(cls, text: str) -> "Ban":
        """``"seq=13+13|198+198+198,ngram=4"`` (each part optional, any order, at least one)."""
        form = f"{BAN_ENV}={text!r}: expected [seq=<int>+<int>|<int>...][,ngram=<int>]"
        kw = {}
        names = {"seq": "sequences", "ngram": "no_repeat_ngram"}

        def ints(val):
            try:
                return tuple(int(v) for v in val.split("+"))
            except ValueError:
                raise ValueError(f"{form}; {val!r} is not a '+'-separated list of integers") from None

        for part in text.split(","):
            key, sep, val = part.strip().partition("=")
            key = key.strip()
            if not sep or key not in names or names[key] in kw:
                raise ValueError(form)
            if key == "seq":
                kw["sequences"] = tuple(ints(s) for s in val.split("|"))
            else:
                n = ints(val)
                if len(n) != 1:
                    raise ValueError(form)
                kw["no_repeat_ngram"] = n[0]
        return cls(**kw)


def env_ban():
    """The process-wide default (LONGSPEC_BAN), or None."""
    text = os.environ.get(BAN_ENV, "")
    return Ban.parse(text) if text else None


def resolve(ban, temperature, use_env: bool):
    """The ``Ban`` a loop runs with: the argument; else, where `use_env` and no temperature is given, the default."""
    return resolve_keyword(ban, Ban, "ban", env_ban,
                           "is not available with temperature > 0, the reference's own T > 0 path; sampled decoding "
                           "with banned tokens is sampling= with ban=",
                           temperature, use_env)
