"""Oracle of ``ops.dry_rows`` (``ls_dry_rows``): the definition of ``longspec_amd/dry.py`` in plain Python, and an operator
namespace layered on ``guide_oracle.ops`` that lets every host loop run with ``dry=`` on the CPU.  The operator reads the
parameters back out of its int32 table, so the table's layout is part of what it checks; the arithmetic is
``(x.float() - pen).to(dtype)`` of CPU torch.  Lives under tests/: the product never imports it."""
import struct
from types import SimpleNamespace

import torch

import guide_oracle
from ban_oracle import row_texts
from longspec_amd import dry as dry_mod

MAX_MATCH = dry_mod.MAX_MATCH


def params_of_table(table):
    """A namespace of what an int32 table holds: ``allowed_length``, ``last_n``, ``breakers`` (a set), ``pen`` (33 floats that
    are exact fp32 values)."""
    t = table.cpu().tolist()
    assert len(t) == dry_mod.TABLE_WORDS == t[3]
    pen = [struct.unpack("<f", struct.pack("<i", v))[0] for v in t[dry_mod.PEN_OFF:dry_mod.PEN_OFF + MAX_MATCH + 1]]
    brk = t[dry_mod.BREAK_OFF:dry_mod.BREAK_OFF + t[0]]
    assert all(v == -1 for v in t[dry_mod.BREAK_OFF + t[0]:])
    return SimpleNamespace(allowed_length=t[1], last_n=t[2], breakers=set(brk), pen=pen)


def spec_of(dry):
    """The text ``Dry.parse`` reads ``dry`` back from."""
    parts = [f"mult={dry.multiplier!r}", f"base={dry.base!r}", f"allow={dry.allowed_length}", f"last={dry.last_n}"]
    if dry.breakers:
        parts.append("break=" + "+".join(str(v) for v in dry.breakers))
    return ",".join(parts)


def matches(text, last_n=0, breakers=()):
    """Every (j, L(j)) of a row with the text ``text`` (a list of ints): the definition, literally."""
    t, m = list(text), len(text)
    lo = max(0, m - last_n) if last_n > 0 else 0
    if m - lo < 2 or t[m - 1] in breakers:
        return
    for j in range(lo, m - 1):
        if t[j] != t[m - 1]:
            continue
        L = 0
        while L < MAX_MATCH and j - L >= lo and t[j - L] == t[m - 1 - L] and t[j - L] not in breakers:
            L += 1
        yield j, L


def match_lengths(text, allowed_length=1, last_n=0, breakers=()):
    """{v: len[v]} of a row with the text ``text``, for the v with ``len[v] >= allowed_length``."""
    out = {}
    for j, L in matches(text, last_n, breakers):
        v = text[j + 1]
        out[v] = max(out.get(v, 0), L)
    return {v: L for v, L in out.items() if L >= allowed_length}


def loops(text, n=8):
    """The first column of ``text`` that ends a verbatim repeat of the ``n`` tokens in front of it at some earlier place --
    column c with text[c-n+1 .. c] == text[j-n+1 .. j] for a j < c --, or None."""
    seen = set()
    for c in range(n - 1, len(text)):
        g = tuple(text[c - n + 1:c + 1])
        if g in seen:
            return c
        seen.add(g)
    return None


def dry_rows(logits, table, output_ids, scratch=None, base=None, base_sub=None, base_add=0, extra_ids=None, extra_mask=None):
    """``longspec_amd.ops.dry_rows`` on CPU tensors (in place, exact).  ``scratch`` is not touched: it stays all zero."""
    p = params_of_table(table)
    x = logits if logits.dim() == 3 else logits.unsqueeze(1)
    b, R, V = x.shape
    texts = row_texts(b, R, output_ids, base, base_sub, base_add, extra_ids, extra_mask)
    for z in range(b):
        for r in range(R):
            for v, L in match_lengths(texts[z][r], p.allowed_length, p.last_n, p.breakers).items():
                if 0 <= v < V and not torch.isnan(x[z, r, v]):
                    x[z, r, v] = (x[z, r, v].float() - torch.tensor(p.pen[L], dtype=torch.float32)).to(x.dtype)
    return logits


class Ops:
    """``guide_oracle.ops`` plus ``dry_rows``: the operator namespace of the ``dry=`` host-logic tests."""

    def __getattr__(self, name):
        return getattr(guide_oracle.ops, name)

    dry_rows = staticmethod(dry_rows)


ops = Ops()
