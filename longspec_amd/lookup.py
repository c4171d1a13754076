"""Prompt-lookup (n-gram) speculation: the definition of the drafter, its limits and the check of its parameters.

The drafter of ``lookup_generate`` is the text itself.  For batch row z the text is

    T = prompt_ids[z, :input_len[z]] ++ output_ids[z, :w],   w = cache_lens[z] - input_len[z] + 1,   L = len(T) = cache_lens[z] + 1

(``w`` columns are written so far, the last round's bonus token included; prompt padding and the output columns at or behind
``w`` are not text).  For every end ``e`` in ``1 .. L-1`` -- the exclusive end of an earlier occurrence, ``T[e]`` exists --
``m(e)`` is the largest ``k <= min(max_ngram, e)`` with ``T[e-k:e] == T[L-k:L]``; ids are compared as 64-bit integers and an
occurrence may overlap the suffix.  An end is a candidate when ``m(e) >= min_ngram``; the winner has the largest ``m``, then
the largest ``e``: the longest context first, then the most recent.  The draft is

    d[i] = T[e + (i mod (L - e))],   i = 0 .. gamma-1

the continuation, extended periodically where it runs into the end of the text -- what one gets by reading on into the draft
itself, so a loop of period p is drafted to full depth.  Without a candidate ``n = 0``, ``e = -1`` and ``d[i] = T[L-1]``: any
valid id will do, a wrong draft is simply rejected.  ``ops.ngram_draft`` (``ls_ngram_draft``, csrc/lookup.hip) computes it on
the device; tests/lookup_oracle.py is the same definition in plain Python."""
from __future__ import annotations

MAX_GAMMA = 15       # draft tokens of a round (one lane each; the verification pass has gamma + 1 rows)
MAX_NGRAM = 8        # tokens of context compared at most


def check(gamma, max_ngram, min_ngram):
    """The three parameters as ints, or ValueError."""
    for name, v in (("gamma", gamma), ("max_ngram", max_ngram), ("min_ngram", min_ngram)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"lookup: {name}={v!r} must be an int")
    if not 1 <= gamma <= MAX_GAMMA:
        raise ValueError(f"lookup: gamma={gamma} outside 1..{MAX_GAMMA}")
    if not 1 <= max_ngram <= MAX_NGRAM:
        raise ValueError(f"lookup: max_ngram={max_ngram} outside 1..{MAX_NGRAM}")
    if not 1 <= min_ngram <= max_ngram:
        raise ValueError(f"lookup: min_ngram={min_ngram} outside 1..max_ngram={max_ngram}")
    return gamma, max_ngram, min_ngram
