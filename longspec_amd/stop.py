"""Stop conditions (``stop=`` of the generate loops and the ``begin_*_decode`` entry points).

With ``stop`` set, a loop ends a batch row at the first generated column where a stop token or a stop sequence matches, and
hands back a text that ends there.  For batch row ``z`` the text is ``output_ids[z, 0:n]``, the generated columns, column 0
being the prefill's token.

* A stop **matches at column c** when ``c >= min_tokens`` and either ``output_ids[z, c]`` is in ``token_ids``, or some sequence
  ``s`` of length ``L <= c + 1`` equals ``output_ids[z, c-L+1 : c+1]``.  A sequence never reaches in front of column 0: nothing
  matches across the prompt boundary.
* The row stops at the smallest such ``c``.  ``which`` is the first stop in listing order that matches there (token ids first,
  then sequences), ``length = c + 1`` and ``match_start = c - L + 1`` of that stop (``L = 1`` for a token id).  The match itself
  stays in ``output_ids``, as the loops keep their EOS; ``match_start`` lets the caller drop it.
* ``min_tokens`` ban: every row of TARGET logits that predicts a column ``< min_tokens`` has the ``token_ids`` entries set to
  ``-inf`` -- behind the penalties, in front of the arg-max or draw and of the log-probs.  Sequences are not banned: a sequence
  match that ends in front of ``min_tokens`` is ignored, and the sequence can match again later.  Draft passes are untouched.

The loops publish the result as ``model.last_stop``, a namespace of int32 ``[bsz]`` tensors ``length``, ``which`` and
``match_start`` (``length = -1`` where no stop matched), and put every column of ``output_ids`` (``spec_mask``,
``last_logprobs``) at or behind ``length`` back to the buffer's initial fill.  Their return tuples stay as they are.  KV lengths,
the penalty state and the host counters ``count`` / ``num`` / ``emitted`` are NOT rolled back: they describe what the rounds
did; a stopped state is final and ``last_stop.length`` is the authority on the text.

The device side (``ops.stop_scan`` / ``ops.stop_ban_rows``) reads one small int32 table, built once per decode state:

    [0] number of token ids   [1] number of sequences   [2] min_tokens   [3] TABLE_WORDS
    [4 : 68]     the token ids, padded with -1
    [68 : 85]    offsets of the sequences into the token area (offset[i + 1] - offset[i] = length of sequence i)
    [85 : 341]   the sequences' tokens, back to back
"""
from __future__ import annotations

import os
from types import SimpleNamespace

import torch

from .keyword import resolve_keyword

STOP_ENV = "LONGSPEC_STOP"       # "ids=128001+128009,seq=13+13|198+198+198,min=8": the process-wide default
MAX_IDS = 64
MAX_SEQS = 16
MAX_SEQ_LEN = 16
IDS_OFF = 4
OFFS_OFF = IDS_OFF + MAX_IDS
TOKS_OFF = OFFS_OFF + MAX_SEQS + 1
TABLE_WORDS = TOKS_OFF + MAX_SEQS * MAX_SEQ_LEN
STATE_WORDS = 4                  # stop_state [bsz, 4] int32: length, which, match_start, reserved


def _token_id(v, what):
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"Stop: {what} {v!r} is not an integer token id")
    if not (0 <= v < 2 ** 31):
        raise ValueError(f"Stop: {what} {v!r} is not a token id (0 .. 2^31 - 1)")
    return v


def _listing(v, what):
    if isinstance(v, (str, bytes)) or not hasattr(v, "__iter__"):
        raise TypeError(f"Stop: {what} must be a sequence of token ids, got {v!r}")
    return tuple(v)


class Stop:
    """``Stop(token_ids=(), sequences=(), min_tokens=0)``: up to 64 distinct stop token ids, up to 16 stop sequences of 1..16
    token ids each (at least one stop in all), and the number of columns in front of which nothing stops."""

    __slots__ = ("token_ids", "sequences", "min_tokens")

    def __init__(self, token_ids=(), sequences=(), min_tokens=0):
        ids = tuple(_token_id(v, "token id") for v in _listing(token_ids, "token_ids"))
        if len(ids) > MAX_IDS:
            raise ValueError(f"Stop: at most {MAX_IDS} token ids, got {len(ids)}")
        if len(set(ids)) != len(ids):
            raise ValueError(f"Stop: token ids must be distinct, got {list(ids)!r}")
        seqs = []
        for s in _listing(sequences, "sequences"):
            s = tuple(_token_id(v, "sequence token") for v in _listing(s, "a stop sequence"))
            if not (1 <= len(s) <= MAX_SEQ_LEN):
                raise ValueError(f"Stop: a sequence holds 1..{MAX_SEQ_LEN} token ids, got {list(s)!r}")
            seqs.append(s)
        if len(seqs) > MAX_SEQS:
            raise ValueError(f"Stop: at most {MAX_SEQS} sequences, got {len(seqs)}")
        if not ids and not seqs:
            raise ValueError("Stop: token_ids and sequences are both empty")
        if isinstance(min_tokens, bool) or not isinstance(min_tokens, int):
            raise TypeError(f"Stop: min_tokens must be an integer, got {min_tokens!r}")
        if not (0 <= min_tokens < 2 ** 31):
            raise ValueError(f"Stop: min_tokens must be >= 0 (and below 2^31), got {min_tokens!r}")
        self.token_ids, self.sequences, self.min_tokens = ids, tuple(seqs), min_tokens

    def __repr__(self):
        return f"Stop(token_ids={self.token_ids}, sequences={self.sequences}, min_tokens={self.min_tokens})"

    def _key(self):
        return (self.token_ids, self.sequences, self.min_tokens)

    def __eq__(self, other):
        return isinstance(other, Stop) and self._key() == other._key()

    def __hash__(self):
        return hash(("Stop",) + self._key())

    def stop_len(self, which: int) -> int:
        """Length of stop number ``which`` in listing order: 1 for a token id."""
        return 1 if which < len(self.token_ids) else len(self.sequences[which - len(self.token_ids)])

    def table(self, vocab: int, device):
        """A new int32 [TABLE_WORDS] table of this object on `device` (layout: the module's docstring).  The object keeps no
        tensor: a decode state holds the table of its generation."""
        for v in self.token_ids + tuple(t for s in self.sequences for t in s):
            if v >= vocab:
                raise ValueError(f"Stop: names token {v}, the vocabulary has {vocab}")
        words = [len(self.token_ids), len(self.sequences), self.min_tokens, TABLE_WORDS]
        words += list(self.token_ids) + [-1] * (MAX_IDS - len(self.token_ids))
        offs, toks = [0], []
        for s in self.sequences:
            toks += list(s)
            offs.append(len(toks))
        words += offs + [offs[-1]] * (MAX_SEQS + 1 - len(offs))
        words += toks + [-1] * (MAX_SEQS * MAX_SEQ_LEN - len(toks))
        assert len(words) == TABLE_WORDS
        return torch.tensor(words, dtype=torch.int32).to(device)

    @classmethod
    def parse(cls, text: str) -> "Stop":
        """``"ids=128001+128009,seq=13+13|198+198+198,min=8"`` (each part optional, any order, ids or seq required)."""
        form = f"{STOP_ENV}={text!r}: expected [ids=<int>+<int>...][,seq=<int>+<int>|<int>...][,min=<int>]"
        kw = {}
        names = {"ids": "token_ids", "seq": "sequences", "min": "min_tokens"}

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
            if key == "ids":
                kw["token_ids"] = ints(val)
            elif key == "seq":
                kw["sequences"] = tuple(ints(s) for s in val.split("|"))
            else:
                m = ints(val)
                if len(m) != 1:
                    raise ValueError(form)
                kw["min_tokens"] = m[0]
        return cls(**kw)


def env_stop():
    """The process-wide default (LONGSPEC_STOP), or None."""
    text = os.environ.get(STOP_ENV, "")
    return Stop.parse(text) if text else None


def resolve(stop, temperature, use_env: bool):
    """The ``Stop`` a loop runs with: the argument; else, where `use_env` and no temperature is given, the default."""
    return resolve_keyword(stop, Stop, "stop", env_stop,
                           "is not available with temperature > 0, the reference's own T > 0 path; sampled decoding "
                           "with stop conditions is sampling= with stop=",
                           temperature, use_env)


def new_state(bsz: int, device) -> torch.Tensor:
    """A fresh ``stop_state`` [bsz, 4] int32: (length, which, match_start) = -1, nothing has stopped; word 3 is reserved."""
    state = torch.full((bsz, STATE_WORDS), -1, dtype=torch.int32, device=device)
    state[:, 3] = 0
    return state


def result_of(state: torch.Tensor) -> SimpleNamespace:
    """``model.last_stop`` of a ``stop_state``: views of its columns."""
    return SimpleNamespace(length=state[:, 0], which=state[:, 1], match_start=state[:, 2])
