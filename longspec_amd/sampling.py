"""Parameters of sampled decoding (``sampling=`` of the generate loops and the ``begin_*_decode`` entry points).

With ``sampling`` set, every arg-max of TARGET logits in a loop becomes one draw from the tempered, top-k / top-p / min_p /
typical_p filtered distribution of that row (``ops.sample_rows``), keyed by (seed, batch row, absolute position); acceptance stays the greedy
one, on the drawn tokens.  ``temperature=`` of the loops is something else: the reference's own T > 0 paths, kept as they are.
"""
from __future__ import annotations

import math
import os

from .keyword import resolve_keyword

SAMPLING_ENV = "LONGSPEC_SAMPLING"       # "t=0.6,k=40,p=0.95,m=0.05,typ=0.9,seed=1": the process-wide default of the begin_*_decode functions


class Sampling:
    """``Sampling(temperature, top_k=0, top_p=1.0, seed=0, min_p=0.0, typical_p=1.0)``: temperature > 0; top_k >= 0 (0 = off);
    0 < top_p <= 1 (1 = off); seed an unsigned 64-bit integer; 0 <= min_p <= 1 (0 = off): drop the tokens whose probability is
    below min_p times the most likely one's; 0 < typical_p <= 1 (1 = off): locally typical sampling, keep the tokens whose
    surprise is closest to the entropy until they hold typical_p of the mass (the most likely token may be dropped).  The
    filters run in the order top_k, top_p, min_p, typical_p, each on what the former kept."""

    __slots__ = ("temperature", "top_k", "top_p", "seed", "min_p", "typical_p")

    def __init__(self, temperature, top_k: int = 0, top_p: float = 1.0, seed: int = 0, min_p: float = 0.0,
                 typical_p: float = 1.0):
        t = float(temperature)
        if not (t > 0 and math.isfinite(t)):
            raise ValueError(f"Sampling: temperature must be a finite number > 0, got {temperature!r}")
        if isinstance(top_k, bool) or int(top_k) != top_k or int(top_k) < 0 or int(top_k) >= 1 << 31:
            raise ValueError(f"Sampling: top_k must be an integer >= 0 (0 = off), got {top_k!r}")
        p = float(top_p)
        if not (0 < p <= 1):
            raise ValueError(f"Sampling: top_p must lie in (0, 1] (1 = off), got {top_p!r}")
        if isinstance(seed, bool) or int(seed) != seed or not (0 <= int(seed) < 1 << 64):
            raise ValueError(f"Sampling: seed must be an integer in [0, 2^64), got {seed!r}")
        mp = float(min_p)
        if not (0 <= mp <= 1):
            raise ValueError(f"Sampling: min_p must lie in [0, 1] (0 = off), got {min_p!r}")
        tp = float(typical_p)
        if not (0 < tp <= 1):
            raise ValueError(f"Sampling: typical_p must lie in (0, 1] (1 = off), got {typical_p!r}")
        self.temperature, self.top_k, self.top_p, self.seed = t, int(top_k), p, int(seed)
        self.min_p, self.typical_p = mp, tp

    def __repr__(self):
        return (f"Sampling(temperature={self.temperature}, top_k={self.top_k}, top_p={self.top_p}, seed={self.seed}, "
                f"min_p={self.min_p}, typical_p={self.typical_p})")

    def __eq__(self, other):
        return isinstance(other, Sampling) and all(getattr(self, n) == getattr(other, n) for n in self.__slots__)

    def __hash__(self):
        return hash(tuple(getattr(self, n) for n in self.__slots__))

    @classmethod
    def parse(cls, text: str) -> "Sampling":
        """``"t=0.6,k=40,p=0.95,m=0.05,typ=0.9,seed=1"`` (``t`` is required, the rest optional, any order)."""
        names = {"t": "temperature", "k": "top_k", "p": "top_p", "seed": "seed", "m": "min_p", "typ": "typical_p"}
        kw = {}
        for part in text.split(","):
            key, sep, val = part.strip().partition("=")
            if not sep or key not in names or names[key] in kw:
                raise ValueError(f"{SAMPLING_ENV}={text!r}: expected t=<float>[,k=<int>][,p=<float>][,m=<float>]"
                                 "[,typ=<float>][,seed=<int>]")
            try:
                kw[names[key]] = int(val) if key in ("k", "seed") else float(val)
            except ValueError:
                raise ValueError(f"{SAMPLING_ENV}={text!r}: {key}={val!r} is not a number") from None
        if "temperature" not in kw:
            raise ValueError(f"{SAMPLING_ENV}={text!r}: t=<temperature> is required")
        return cls(**kw)


def env_sampling():
    """The process-wide default (LONGSPEC_SAMPLING), or None."""
    text = os.environ.get(SAMPLING_ENV, "")
    return Sampling.parse(text) if text else None


def resolve(sampling, temperature, use_env: bool):
    """The ``Sampling`` a loop runs with: the argument; else, where `use_env` and no temperature is given, the default."""
    return resolve_keyword(sampling, Sampling, "sampling", env_sampling,
                           "and temperature > 0 are two different decoders: sampling= draws every token from the "
                           "target's distribution, temperature= is the reference's own T > 0 path; give one of them",
                           temperature, use_env)
