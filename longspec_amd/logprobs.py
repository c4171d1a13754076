"""Log-probabilities of the emitted tokens (``logprobs=`` of the generate loops and the ``begin_*_decode`` entry points).

With ``logprobs`` set, a loop keeps, column for column with ``output_ids``, the log-probability of every emitted token under
the distribution it was taken from, and the ``top_n`` most likely alternatives (``ops.token_logprobs``).  For a row of 16-bit
target logits ``x`` as the token was picked from them -- behind the penalties when ``penalties=`` is on -- and
``T = sampling.temperature`` (1 for greedy decoding), in fp32:

    lp_j = (x_j - m) / T - ln sum_i exp((x_i - m) / T),   m = max_i x_i

The distribution is over the FULL vocabulary: a sampled token that survived a top-k / top-p / min_p / typical_p cut is reported
under the tempered, penalised soft-max, not under the renormalised kept set ("processed logits, not truncated") -- the one definition that is the
same for greedy and sampled rows.  The alternatives are the ``top_n`` columns with the largest logits, ordered by (logit
descending, column ascending): the order of the arg-max, so under greedy decoding the first alternative IS the emitted token.

The loops publish the result as ``model.last_logprobs``, a namespace of
    token   [bsz, W] fp32          log-prob of ``output_ids[:, c]``; NaN where nothing was emitted
    top_ids [bsz, W, top_n] int64  columns of the alternatives; -1 where nothing was emitted
    top     [bsz, W, top_n] fp32   their log-probs; -inf where nothing was emitted
Their return tuples stay as they are.
"""
from __future__ import annotations

import os
from types import SimpleNamespace

import torch

from .keyword import resolve_keyword

LOGPROBS_ENV = "LONGSPEC_LOGPROBS"       # "n=5": the process-wide default of the loops and the begin_*_decode functions
MAX_TOP_N = 20


class Logprobs:
    """``Logprobs(top_n=0)``: keep the log-prob of every emitted token and its ``top_n`` (0..20) most likely alternatives."""

    __slots__ = ("top_n",)

    def __init__(self, top_n: int = 0):
        if isinstance(top_n, bool) or not isinstance(top_n, int) or not (0 <= top_n <= MAX_TOP_N):
            raise ValueError(f"Logprobs: top_n must be an integer in 0..{MAX_TOP_N}, got {top_n!r}")
        self.top_n = top_n

    def __repr__(self):
        return f"Logprobs(top_n={self.top_n})"

    def __eq__(self, other):
        return isinstance(other, Logprobs) and self.top_n == other.top_n

    def __hash__(self):
        return hash(("Logprobs", self.top_n))

    @classmethod
    def parse(cls, text: str) -> "Logprobs":
        """``"n=5"`` (``n`` = top_n, required)."""
        key, sep, val = text.strip().partition("=")
        if not sep or key.strip() != "n":
            raise ValueError(f"{LOGPROBS_ENV}={text!r}: expected n=<int>")
        try:
            n = int(val)
        except ValueError:
            raise ValueError(f"{LOGPROBS_ENV}={text!r}: n={val!r} is not an integer") from None
        return cls(n)


def env_logprobs():
    """The process-wide default (LONGSPEC_LOGPROBS), or None."""
    text = os.environ.get(LOGPROBS_ENV, "")
    return Logprobs.parse(text) if text else None


def resolve(logprobs, temperature, use_env: bool):
    """The ``Logprobs`` a loop runs with: the argument; else, where `use_env` and no temperature is given, the default."""
    return resolve_keyword(logprobs, Logprobs, "logprobs", env_logprobs,
                           "is not available with temperature > 0, the reference's own T > 0 path; sampled "
                           "decoding with log-probs is sampling= with logprobs=",
                           temperature, use_env)


def new_buffers(bsz: int, width: int, top_n: int, device) -> SimpleNamespace:
    """The three output buffers, aligned with an ``output_ids`` of ``width`` columns, holding their fill values."""
    return SimpleNamespace(token=torch.full((bsz, width), float("nan"), dtype=torch.float32, device=device),
                           top_ids=torch.full((bsz, width, top_n), -1, dtype=torch.int64, device=device),
                           top=torch.full((bsz, width, top_n), float("-inf"), dtype=torch.float32, device=device))
