"""Two truncation samplers on the target's draw (``cut=`` of the generate loops and the ``begin_*_decode`` entry points), next to
``sampling=``, which they need: ``top_n_sigma`` and XTC ("exclude top choices").  Both run inside ``ops.sample_rows``
(``ls_sample_rows_cut``, ``csrc/sample_cut.hip``); ``logprobs=`` is untouched, it is defined over the full ruled vocabulary.

A row is the 16-bit target logits ``x`` behind all rules (``TargetRules.apply``), ``T`` the sampler's temperature, ``m`` the row
maximum.  Filter order, each on what the former kept: top_n_sigma -> top_k -> top_p -> min_p -> typical_p -> xtc.

``top_n_sigma = n`` (finite, >= 0; 0 = off).  Over the ``N`` finite entries of the row (``-inf`` takes no part)
``sigma = sqrt(sum (x - mean)^2 / N)``, the population deviation of the raw 16-bit values -- not divided by ``T``, so the kept
set does not change with the temperature.  Keep ``x_j >= m - n sigma``.  A threshold set that holds the maximum: it intersects
with top_k in either order, and top_p's mass is taken over what both kept.  ``sigma = 0`` (one finite logit, or all equal) keeps
the maxima; a row without a finite logit is left alone.  The kernel sums ``y = x - m`` in double precision in a fixed order.

``xtc = (probability P, threshold theta)``, ``0 <= P <= 1`` (0 = off), ``0 < theta <= 1``.  The row's coin is Philox4x32-10
with the seed's two halves as key and counter ``(0xFFFFFFFF, position lo, position hi, stream)``; word 0 gives
``u = ((w >> 9) + 0.5) 2^-23`` and the cut happens iff ``u < P``, compared in fp32.  (Token noise has counter word 0 =
``column >> 2 < 2^22``: the streams cannot meet.)  When the coin fires, with ``S`` the set kept so far,
``F(v) = floor(2^40 exp((v - m) / T))`` as top_p forms it and ``Z_S`` the integer sum of ``F`` over ``S``: ``v*`` is the
smallest value occurring in ``S`` with ``F(v*) >= ceil(theta Z_S)``, and every token of ``S`` above ``v*`` is dropped.  ALL
tokens tied at ``v*`` stay (llama.cpp keeps one of them; the rule mirrors top_k's ties here).  If only the largest value of
``S`` qualifies, or nothing does, the row is unchanged: ``theta > 0.5`` is a no-op without a tie at the top.  So is a row
with ``Z_S = 0`` (typical_p has moved ``S`` so far below ``m`` that every ``F`` is 0).  XTC never empties a row.
"""
from __future__ import annotations

import math
import os

from .keyword import resolve_keyword

CUT_ENV = "LONGSPEC_CUT"       # "sigma=1.0,xtcp=0.5,xtct=0.1": the process-wide default of the begin_*_decode functions


class Cut:
    """``Cut(top_n_sigma=0.0, xtc_probability=0.0, xtc_threshold=0.1)``: top_n_sigma finite and >= 0 (0 = off);
    0 <= xtc_probability <= 1 (0 = off); 0 < xtc_threshold <= 1.  The module has the definitions."""

    __slots__ = ("top_n_sigma", "xtc_probability", "xtc_threshold")

    def __init__(self, top_n_sigma: float = 0.0, xtc_probability: float = 0.0, xtc_threshold: float = 0.1):
        for name, v in (("top_n_sigma", top_n_sigma), ("xtc_probability", xtc_probability), ("xtc_threshold", xtc_threshold)):
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise TypeError(f"Cut: {name} must be a number, got {v!r}")
        n, p, t = float(top_n_sigma), float(xtc_probability), float(xtc_threshold)
        if not (n >= 0 and math.isfinite(n)):
            raise ValueError(f"Cut: top_n_sigma must be a finite number >= 0 (0 = off), got {top_n_sigma!r}")
        if not (0 <= p <= 1):
            raise ValueError(f"Cut: xtc_probability must lie in [0, 1] (0 = off), got {xtc_probability!r}")
        if not (0 < t <= 1):
            raise ValueError(f"Cut: xtc_threshold must lie in (0, 1], got {xtc_threshold!r}")
        self.top_n_sigma, self.xtc_probability, self.xtc_threshold = n, p, t

    @property
    def on(self) -> bool:
        """Whether either filter does anything."""
        return self.top_n_sigma > 0.0 or self.xtc_probability > 0.0

    def __repr__(self):
        return (f"Cut(top_n_sigma={self.top_n_sigma}, xtc_probability={self.xtc_probability}, "
                f"xtc_threshold={self.xtc_threshold})")

    def __eq__(self, other):
        return isinstance(other, Cut) and all(getattr(self, n) == getattr(other, n) for n in self.__slots__)

    def __hash__(self):
        return hash(tuple(getattr(self, n) for n in self.__slots__))

    @classmethod
    def parse(cls, text: str) -> "Cut":
        """``"sigma=1.0,xtcp=0.5,xtct=0.1"`` (all optional, any order)."""
        form = f"{CUT_ENV}={text!r}: expected [sigma=<float>][,xtcp=<float>][,xtct=<float>]"
        names = {"sigma": "top_n_sigma", "xtcp": "xtc_probability", "xtct": "xtc_threshold"}
        kw = {}
        for part in text.split(","):
            key, sep, val = part.strip().partition("=")
            key = key.strip()
            if not sep or key not in names or names[key] in kw:
                raise ValueError(form)
            try:
                kw[names[key]] = float(val)
            except ValueError:
                raise ValueError(f"{form}; {key}={val!r} is not a number") from None
        return cls(**kw)


def env_cut():
    """The process-wide default (LONGSPEC_CUT), or None."""
    text = os.environ.get(CUT_ENV, "")
    return Cut.parse(text) if text else None


def resolve(cut, temperature, use_env: bool, sampling=None):
    """The ``Cut`` a loop runs with: the argument; else, where `use_env` and no temperature is given, the default; None where
    both of its filters are off.  ``sampling``: the ``Sampling`` in force -- a cut without one is refused, whether it was
    passed or comes from the environment."""
    cut = resolve_keyword(cut, Cut, "cut", env_cut,
                          "is not available with temperature > 0, the reference's own T > 0 path; the cuts act on the draw "
                          "of sampling=",
                          temperature, use_env)
    if cut is None or not cut.on:
        return None
    if sampling is None:
        raise ValueError("cut= needs sampling=: top_n_sigma and xtc cut the set a sampled draw is taken from, and no "
                         "sampling= (or LONGSPEC_SAMPLING) is in force")
    return cut
