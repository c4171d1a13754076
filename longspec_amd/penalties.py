"""Token penalties and logit bias (``penalties=`` of the generate loops and the ``begin_*_decode`` entry points).

With ``penalties`` set, every row of TARGET logits a loop takes an arg-max or a draw of is first rewritten by
``ops.penalize_rows`` from that row's own history: the prompt, the text generated so far and -- in a verification pass -- the
draft tokens the row follows.  The draft passes are not penalised: a draft only decides how far a round gets.  Per element v
with 16-bit logit x, in fp32, with c = times v occurs in the generated part of the row's history:

  1. c > 0 or v occurs in the prompt:  x = x / repetition when x > 0, else x = x * repetition
  2. c > 0:                            x = x - frequency * c, then x = x - presence
  3. bias given:                       x = x + bias[v]
  4. x is rounded to nearest-even back into the logits' type

(repetition acts on prompt and generated tokens, presence and frequency on generated tokens only: the vLLM / OpenAI convention.)
"""
from __future__ import annotations

import math
import os

from .keyword import resolve_keyword

PENALTIES_ENV = "LONGSPEC_PENALTIES"     # "rep=1.1,pres=0.5,freq=0.2": the process-wide default of the begin_*_decode functions


class Penalties:
    """``Penalties(repetition=1.0, presence=0.0, frequency=0.0, bias=None)``: repetition finite and > 0; presence and frequency
    finite; bias a ``{token id: float}`` mapping with finite or ``-inf`` values (``-inf`` bans the token)."""

    __slots__ = ("repetition", "presence", "frequency", "bias")

    def __init__(self, repetition=1.0, presence=0.0, frequency=0.0, bias=None):
        r, p, f = float(repetition), float(presence), float(frequency)
        if not (math.isfinite(r) and r > 0):
            raise ValueError(f"Penalties: repetition must be a finite number > 0, got {repetition!r}")
        if not math.isfinite(p):
            raise ValueError(f"Penalties: presence must be finite, got {presence!r}")
        if not math.isfinite(f):
            raise ValueError(f"Penalties: frequency must be finite, got {frequency!r}")
        items = []
        if bias is not None:
            if not hasattr(bias, "items"):
                raise TypeError(f"Penalties: bias must be a {{token id: float}} mapping or None, got {type(bias).__name__}")
            for tok, val in bias.items():
                if isinstance(tok, bool) or int(tok) != tok or int(tok) < 0:
                    raise ValueError(f"Penalties: bias key {tok!r} is not a token id")
                v = float(val)
                if math.isnan(v) or v == math.inf:
                    raise ValueError(f"Penalties: bias[{tok!r}] must be finite or -inf, got {val!r}")
                items.append((int(tok), v))
        self.repetition, self.presence, self.frequency = r, p, f
        self.bias = tuple(sorted(items))

    def __repr__(self):
        return (f"Penalties(repetition={self.repetition}, presence={self.presence}, frequency={self.frequency}, "
                f"bias={dict(self.bias) if self.bias else None})")

    def __eq__(self, other):
        return isinstance(other, Penalties) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def _key(self):
        return (self.repetition, self.presence, self.frequency, self.bias)

    @property
    def changes_nothing(self) -> bool:
        return self.repetition == 1.0 and self.presence == 0.0 and self.frequency == 0.0 and not any(v != 0.0 for _, v in self.bias)

    def bias_table(self, vocab: int, device):
        """A new dense fp32 [vocab] table of ``bias`` on `device` (None without a bias).  The object keeps no tensor: a decode
        state holds the table of its generation (``st.bias_table``)."""
        if not self.bias:
            return None
        import torch
        if self.bias[-1][0] >= vocab:
            raise ValueError(f"Penalties: bias names token {self.bias[-1][0]}, the vocabulary has {vocab}")
        host = torch.zeros((vocab,), dtype=torch.float32)
        host[torch.tensor([k for k, _ in self.bias], dtype=torch.int64)] = torch.tensor([v for _, v in self.bias], dtype=torch.float32)
        return host.to(device)

    @classmethod
    def parse(cls, text: str) -> "Penalties":
        """``"rep=1.1,pres=0.5,freq=0.2"`` (each optional, any order)."""
        names = {"rep": "repetition", "pres": "presence", "freq": "frequency"}
        kw = {}
        for part in text.split(","):
            key, sep, val = part.strip().partition("=")
            if not sep or key not in names or names[key] in kw:
                raise ValueError(f"{PENALTIES_ENV}={text!r}: expected [rep=<float>][,pres=<float>][,freq=<float>]")
            try:
                kw[names[key]] = float(val)
            except ValueError:
                raise ValueError(f"{PENALTIES_ENV}={text!r}: {key}={val!r} is not a number") from None
        return cls(**kw)


def env_penalties():
    """The process-wide default (LONGSPEC_PENALTIES), or None."""
    text = os.environ.get(PENALTIES_ENV, "")
    return Penalties.parse(text) if text else None


def resolve(penalties, temperature, use_env: bool):
    """The ``Penalties`` a loop runs with, or None when nothing would change: the argument; else, where `use_env` and no
    temperature is given, the default."""
    p = resolve_keyword(penalties, Penalties, "penalties", env_penalties,
                        "is not available with temperature > 0: that is the reference's own T > 0 path, kept "
                        "token for token; penalised sampling is sampling= with penalties=",
                        temperature, use_env)
    return None if p is None or p.changes_nothing else p
