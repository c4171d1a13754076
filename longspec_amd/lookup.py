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
the device; tests/lookup_oracle.py is the same definition in plain Python.

The tree drafter (``lookup_generate(branches=B)``, ``2 <= B <= 8``) offers several continuations to ONE verification pass.
The text, ``m(e)`` and the candidates are those above, with one difference: the number of written output columns is a tensor
of its own, ``w = written[z]`` (int32, clamped to the buffer; the tree round's ``emitted_dev``), so ``L = input_len[z] + w`` --
in the tree round ``cache_lens`` lags the text by the tokens the next pass feeds again.

* The candidates are ordered by the key ``(m, e)``, descending, and the first ``NGRAM_TOP = 8`` are taken.
* The continuation of ``e`` is ``c_e[i] = T[e + (i mod (L - e))]``, ``i = 0 .. gamma-1``: the periodic extension above.
* The 8 are walked in that order; one is kept when its ``gamma``-tuple differs from every kept one; the walk stops at ``B``
  kept.  ``nb`` (0..B) is the number kept.
* Slot ``j < nb`` holds kept candidate ``j``; a slot ``j >= nb`` holds a copy of slot 0.  With ``nb = 0`` every slot is
  ``T[L-1]`` repeated and its ``(n, e)`` is ``(0, -1)``.  Slot 0 is therefore always what ``ngram_draft`` drafts from the text.

The tree has ``F = 1 + B * gamma`` nodes, the root (the last emitted token) first, in a static, LEVEL-MAJOR order: the node of
branch ``j`` at depth ``d`` (1..gamma) is ``1 + (d-1) * B + j``; ``all_spec[node] = slot_j[d-1]``; ``tree_mask[node, :]`` is
1 at column 0 and at the nodes of branch ``j`` at depths ``<= d`` (itself included), else 0.  Level-major is what makes copies
harmless: ``tree_collapse`` accepts the path of the highest-indexed node whose whole path verifies, and with the levels in
index order that node is one of the deepest.  Two branches that share a verified prefix verify alike along it and name the
same tokens, so whichever of them the index order prefers, the accepted text is the same.
``ops.ngram_tree_draft`` (``ls_ngram_tree_draft``, csrc/lookup_tree.hip) computes all of it on the device;
tests/lookup_tree_oracle.py is the same definition in plain Python."""
from __future__ import annotations

MAX_GAMMA = 15       # draft tokens of a round (one lane each; the verification pass has gamma + 1 rows)
MAX_NGRAM = 8        # tokens of context compared at most
NGRAM_TOP = 8        # candidates the tree drafter walks, and so the most branches of a tree
MAX_ROWS = 80        # rows of a verification pass (ops.LINEAR_MAX_ROWS)


def tree_rows(gamma: int, branches: int) -> int:
    """Rows of the tree round's verification pass: up to gamma + 1 accepted tokens fed again, and the branches * gamma nodes."""
    return branches * gamma + gamma + 1


def check(gamma, max_ngram, min_ngram, branches=1):
    """The three parameters as ints, or ValueError.  ``branches`` is checked with them: 1 is the chain, 2..8 a tree whose
    verification pass (``tree_rows``) must fit ``MAX_ROWS``."""
    for name, v in (("gamma", gamma), ("max_ngram", max_ngram), ("min_ngram", min_ngram), ("branches", branches)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"lookup: {name}={v!r} must be an int")
    if not 1 <= gamma <= MAX_GAMMA:
        raise ValueError(f"lookup: gamma={gamma} outside 1..{MAX_GAMMA}")
    if not 1 <= max_ngram <= MAX_NGRAM:
        raise ValueError(f"lookup: max_ngram={max_ngram} outside 1..{MAX_NGRAM}")
    if not 1 <= min_ngram <= max_ngram:
        raise ValueError(f"lookup: min_ngram={min_ngram} outside 1..max_ngram={max_ngram}")
    if not 1 <= branches <= NGRAM_TOP:
        raise ValueError(f"lookup: branches={branches} outside 1..{NGRAM_TOP}")
    if branches > 1 and tree_rows(gamma, branches) > MAX_ROWS:
        raise ValueError(f"lookup: branches={branches} x gamma={gamma} needs a verification pass of {tree_rows(gamma, branches)} "
                         f"rows, above {MAX_ROWS}")
    return gamma, max_ngram, min_ngram
