"""Oracle of ``ops.ban_rows`` (``ls_ban_rows``): the definition of ``longspec_amd/ban.py`` in plain Python, and an operator
namespace layered on ``lookup_tree_oracle.ops`` that lets every host loop run with ``ban=`` on the CPU.  The operator reads the
``Ban`` back out of its int32 table, so the table's layout is part of what it checks.  Lives under tests/: the product never
imports it."""
import math
from types import SimpleNamespace

import lookup_tree_oracle
from longspec_amd import Ban
from longspec_amd import ban as ban_mod


def ban_of_table(table, raw=False):
    """The ``Ban`` an int32 table was built from; ``raw``: a namespace of its two fields as the table has them, unvalidated (a
    hand-made table may hold -1)."""
    t = table.cpu().tolist()
    assert len(t) == ban_mod.TABLE_WORDS == t[3]
    offs = t[ban_mod.OFFS_OFF:ban_mod.OFFS_OFF + t[0] + 1]
    seqs = tuple(tuple(t[ban_mod.TOKS_OFF + offs[q]:ban_mod.TOKS_OFF + offs[q + 1]]) for q in range(t[0]))
    return SimpleNamespace(sequences=seqs, no_repeat_ngram=t[1]) if raw else Ban(seqs, t[1])


def spec_of(ban):
    """The text ``Ban.parse`` reads ``ban`` back from."""
    parts = []
    if ban.sequences:
        parts.append("seq=" + "|".join("+".join(str(v) for v in s) for s in ban.sequences))
    if ban.no_repeat_ngram:
        parts.append(f"ngram={ban.no_repeat_ngram}")
    return ",".join(parts)


def forbidden(text, ban):
    """The ids a row with the text ``text`` (a list of ints) may not emit next, as a set: the definition, literally."""
    t, m, out = list(text), len(text), set()
    for s in ban.sequences:
        L = len(s)
        if L - 1 <= m and t[m - L + 1:m] == list(s[:L - 1]):
            out.add(s[L - 1])
    n = ban.no_repeat_ngram
    if n >= 1 and m >= n - 1:
        tail = t[m - n + 1:m]
        for j in range(n - 1, m):
            if t[j - n + 1:j] == tail:
                out.add(t[j])
    return out


def repeats(text, n):
    """The first column of ``text`` that completes an n-gram the text already holds, or None."""
    seen = set()
    for c in range(n - 1, len(text)):
        g = tuple(text[c - n + 1:c + 1])
        if g in seen:
            return c
        seen.add(g)
    return None


def row_texts(b, rows, output_ids, base=None, base_sub=None, base_add=0, extra_ids=None, extra_mask=None):
    """[z][r] -> the text of row r of batch z, as ``ban_rows`` defines it."""
    out = []
    for z in range(b):
        W = output_ids.shape[1] if output_ids is not None else 0
        w = (int(base[z]) if base is not None else 0) - (int(base_sub[z]) if base_sub is not None else 0) + base_add
        w = max(0, min(w, W))
        head = output_ids[z, :w].tolist() if w else []
        per_row = []
        for r in range(rows):
            path = []
            if extra_ids is not None and extra_ids.shape[-1] > 0:
                mask = extra_mask[z, r] if extra_mask.dim() == 3 else extra_mask[r]
                path = [int(extra_ids[z, c]) for c in range(extra_ids.shape[-1]) if int(mask[c]) != 0]
            per_row.append(head + path)
        out.append(per_row)
    return out


def ban_rows(logits, table, output_ids, base=None, base_sub=None, base_add=0, extra_ids=None, extra_mask=None):
    """``longspec_amd.ops.ban_rows`` on CPU tensors (in place, exact)."""
    ban = ban_of_table(table, raw=True)
    x = logits if logits.dim() == 3 else logits.unsqueeze(1)
    b, R, V = x.shape
    texts = row_texts(b, R, output_ids, base, base_sub, base_add, extra_ids, extra_mask)
    for z in range(b):
        for r in range(R):
            for t in forbidden(texts[z][r], ban):
                if 0 <= t < V:
                    x[z, r, t] = -math.inf
    return logits


class Ops:
    """``lookup_tree_oracle.ops`` plus ``ban_rows``: the operator namespace of the ``ban=`` host-logic tests."""

    def __getattr__(self, name):
        return getattr(lookup_tree_oracle.ops, name)

    ban_rows = staticmethod(ban_rows)


ops = Ops()
