"""The DRY ("don't repeat yourself") repetition penalty (``dry=`` of the generate loops and the ``begin_*_decode`` entry points).

With ``dry`` set, a token whose emission would extend a repeat of the text loses logit mass in proportion to the length of
that repeat: ``multiplier * base ** (length - allowed_length)``.  Unlike ``Ban(no_repeat_ngram=n)`` nothing is forbidden: a
name, a number or a code idiom can still be said twice, a verbatim loop gets exponentially dearer with every token.  The
penalty acts on the TARGET's logits -- behind ``penalties=``, in front of the bans of ``stop=`` / ``ban=`` / ``guide=``, of the
arg-max or draw and of the log-probs.  The text is then exactly DRY-penalised decoding of the target, whichever loop produced
it; draft passes are untouched.

**Definition.**  For a row of target logits let ``t[0 .. m-1]`` be the row's text, exactly as for ``ban=``: the generated
columns ``output_ids[z, :w]`` (column 0 being the prefill's token; the prompt is NOT part of it, nothing matches across the
prompt boundary -- quoting the document is no loop) followed, in a verification pass, by the draft tokens the row follows --
``extra_ids[z, c]`` with ``extra_mask[z, r, c] != 0``, in increasing ``c``, which is path order.  The row predicts ``t[m]``.

* ``lo = max(0, m - last_n)`` if ``last_n > 0``, else 0: only ``t[lo .. m-1]`` is looked at.
* Nothing changes if ``m - lo < 2`` or if ``x = t[m-1]`` is a breaker.
* For every ``j`` in ``[lo, m-2]`` with ``t[j] == x``, ``L(j)`` is the largest ``L <= MAX_MATCH`` such that for all
  ``0 <= k < L``: ``j - k >= lo``, ``t[j-k] == t[m-1-k]`` and ``t[j-k]`` is not a breaker.  The candidate is ``v = t[j+1]``;
  ``len[v]`` is the maximum of ``L(j)`` over the ``j`` with that candidate.
* For every ``v`` in ``[0, vocab)`` with ``len[v] >= allowed_length``: ``logit[v] = dtype(float(logit[v]) - pen[len[v]])`` --
  one fp32 subtraction, rounded to nearest even into the logits' 16-bit type.  A NaN keeps its bits; ``-inf`` stays ``-inf``.
* ``pen[L] = multiplier * base ** (L - allowed_length)`` for ``L`` in 0..``MAX_MATCH``, computed once on the host in float64
  and rounded to fp32 (a value beyond fp32 becomes the largest fp32): the device looks it up and never calls ``pow``.
* Ids of the text outside ``[0, vocab)`` take part in the matches as they are and are never penalised.  Every element that is
  not penalised keeps its bits.

**Saturation.**  Matches are measured up to ``MAX_MATCH = 32`` tokens: a longer repeat is penalised like one of 32.  With the
default base the penalty at 32 is about 2e7 times the multiplier, far beyond any 16-bit logit, so nothing is lost.  With a
base near 1 it is: at ``base = 1`` the penalty is the multiplier at every length, and at ``base = 1.05`` it stops growing at
``1.05 ** 30`` = 4.3 times the multiplier however long the loop gets.

No state beyond ``output_ids``: nothing is committed or rolled back.  The device side (``ops.dry_rows``) reads one int32 table,
built once per decode state:

    [0] number of breakers   [1] allowed_length   [2] last_n   [3] TABLE_WORDS
    [4 : 37]     pen[0 .. 32] as fp32 bits
    [37 : 101]   the breaker ids, padded with -1
"""
from __future__ import annotations

import math
import os
import struct

import torch

from .keyword import resolve_keyword

DRY_ENV = "LONGSPEC_DRY"         # "mult=0.8,base=1.75,allow=2,last=0,break=13+198": the process-wide default
MAX_MATCH = 32                   # LS_DRY_MAX_MATCH
MAX_BREAKERS = 64
MAX_LAST_N = 2 ** 23
PEN_OFF = 4
BREAK_OFF = PEN_OFF + MAX_MATCH + 1
TABLE_WORDS = BREAK_OFF + MAX_BREAKERS
FP32_MAX = 3.4028234663852886e38


def _number(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"Dry: {what} must be a number, got {v!r}")
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"Dry: {what} must be finite, got {v!r}")
    return v


def _integer(v, what):
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"Dry: {what} must be an integer, got {v!r}")
    return v


class Dry:
    """``Dry(multiplier, base=1.75, allowed_length=2, breakers=(), last_n=0)``: the penalty of a repeat of ``L >=
    allowed_length`` tokens is ``multiplier * base ** (L - allowed_length)`` (``multiplier`` finite and > 0, ``base`` in [1, 4],
    ``allowed_length`` in 1..32); up to 64 distinct ``breakers``, token ids no match reaches across; ``last_n``: the tokens at
    the end of the generated text that are looked at (0: all of it, else up to 2^23)."""

    __slots__ = ("multiplier", "base", "allowed_length", "breakers", "last_n")

    def __init__(self, multiplier, base=1.75, allowed_length=2, breakers=(), last_n=0):
        multiplier, base = _number(multiplier, "multiplier"), _number(base, "base")
        if not multiplier > 0:
            raise ValueError(f"Dry: multiplier must be > 0, got {multiplier!r}")
        if not (1.0 <= base <= 4.0):
            raise ValueError(f"Dry: base must be in [1, 4], got {base!r}")
        if not (1 <= _integer(allowed_length, "allowed_length") <= MAX_MATCH):
            raise ValueError(f"Dry: allowed_length must be 1..{MAX_MATCH}, got {allowed_length!r}")
        if isinstance(breakers, (str, bytes)) or not hasattr(breakers, "__iter__"):
            raise TypeError(f"Dry: breakers must be a sequence of token ids, got {breakers!r}")
        breakers = tuple(breakers)
        for v in breakers:
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError(f"Dry: breaker {v!r} is not an integer token id")
            if not (0 <= v < 2 ** 31):
                raise ValueError(f"Dry: breaker {v!r} is not a token id (0 .. 2^31 - 1)")
        if len(set(breakers)) != len(breakers):
            raise ValueError(f"Dry: the breakers must be distinct, got {list(breakers)!r}")
        if len(breakers) > MAX_BREAKERS:
            raise ValueError(f"Dry: at most {MAX_BREAKERS} breakers, got {len(breakers)}")
        if not (0 <= _integer(last_n, "last_n") <= MAX_LAST_N):
            raise ValueError(f"Dry: last_n must be 0 (the whole text) or 1..2^23, got {last_n!r}")
        self.multiplier, self.base, self.allowed_length, self.breakers, self.last_n = multiplier, base, allowed_length, breakers, last_n

    def __repr__(self):
        return (f"Dry(multiplier={self.multiplier}, base={self.base}, allowed_length={self.allowed_length}, "
                f"breakers={self.breakers}, last_n={self.last_n})")

    def _key(self):
        return (self.multiplier, self.base, self.allowed_length, self.breakers, self.last_n)

    def __eq__(self, other):
        return isinstance(other, Dry) and self._key() == other._key()

    def __hash__(self):
        return hash(("Dry",) + self._key())

    def penalties(self):
        """``pen[0 .. MAX_MATCH]`` as Python floats that are exact fp32 values (the definition: float64, then one rounding)."""
        out = []
        for L in range(MAX_MATCH + 1):
            p = min(self.multiplier * self.base ** (L - self.allowed_length), FP32_MAX)
            out.append(struct.unpack("<f", struct.pack("<f", p))[0])
        return out

    def table(self, vocab: int, device):
        """A new int32 [TABLE_WORDS] table of this object on `device` (layout: the module's docstring).  The object keeps no
        tensor: a decode state holds the table of its generation.  A breaker ``>= vocab`` is legal: ids outside the
        vocabulary take part in matches."""
        words = [len(self.breakers), self.allowed_length, self.last_n, TABLE_WORDS]
        words += [struct.unpack("<i", struct.pack("<f", p))[0] for p in self.penalties()]
        words += list(self.breakers) + [-1] * (MAX_BREAKERS - len(self.breakers))
        assert len(words) == TABLE_WORDS
        return torch.tensor(words, dtype=torch.int32).to(device)

    @classmethod
    def parse(cls, text: str) -> "Dry":
        """``"mult=0.8,base=1.75,allow=2,last=0,break=13+198"`` (``mult`` required, the others optional, any order)."""
        form = f"{DRY_ENV}={text!r}: expected mult=<float>[,base=<float>][,allow=<int>][,last=<int>][,break=<int>+<int>...]"
        names = {"mult": ("multiplier", float), "base": ("base", float), "allow": ("allowed_length", int), "last": ("last_n", int),
                 "break": ("breakers", None)}
        kw = {}
        for part in text.split(","):
            key, sep, val = part.strip().partition("=")
            key = key.strip()
            if not sep or key not in names or names[key][0] in kw:
                raise ValueError(form)
            name, conv = names[key]
            try:
                kw[name] = conv(val) if conv is not None else tuple(int(v) for v in val.split("+"))
            except ValueError:
                raise ValueError(f"{form}; {val!r} does not read as the value of {key}") from None
        if "multiplier" not in kw:
            raise ValueError(form)
        return cls(**kw)


def env_dry():
    """The process-wide default (LONGSPEC_DRY), or None."""
    text = os.environ.get(DRY_ENV, "")
    return Dry.parse(text) if text else None


def resolve(dry, temperature, use_env: bool):
    """The ``Dry`` a loop runs with: the argument; else, where `use_env` and no temperature is given, the default."""
    return resolve_keyword(dry, Dry, "dry", env_dry,
                           "is not available with temperature > 0, the reference's own T > 0 path; sampled decoding "
                           "with the DRY penalty is sampling= with dry=",
                           temperature, use_env)
