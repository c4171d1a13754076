"""Oracle of ``ops.watermark_rows`` / ``ops.watermark_score`` (``ls_watermark_rows`` / ``ls_watermark_score``): the definition
of ``longspec_amd/watermark.py`` in plain Python integers, one id at a time -- written from the definition, not from that
module's vectorised restatement --, and an operator namespace layered on ``dry_oracle.ops`` that lets every host loop run with
``watermark=`` on the CPU.  The operator reads the parameters back out of its int32 table, so the table's layout is part of
what it checks; the arithmetic is ``(x.float() + delta).to(dtype)`` of CPU torch.  Lives under tests/: the product never
imports it."""
import functools
import math
import struct
from types import SimpleNamespace

import torch

import dry_oracle
from ban_oracle import row_texts

MASK = (1 << 64) - 1
M1, M2, M3 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
TABLE_WORDS = 8


def fin(z):
    z = ((z ^ (z >> 30)) * M2) & MASK
    z = ((z ^ (z >> 27)) * M3) & MASK
    return z ^ (z >> 31)


def state(key, context):
    """The state of the tokens ``context``, oldest first (Python ints; a negative id is its 64-bit two's complement)."""
    s = fin((key + M1) & MASK)
    for c in context:
        s = fin(((s ^ (c & MASK)) + M1) & MASK)
    return s


def u_of(s, v):
    return fin((s + ((v & MASK) + 1) * M1) & MASK)


def is_green(s, v, T):
    return (u_of(s, v) >> 32) < T


def green_ids(key, context, gamma, upto):
    """The green ids below ``upto`` after ``context``."""
    s, T = state(key, context), math.floor(gamma * 2 ** 32)
    return [v for v in range(upto) if is_green(s, v, T)]


@functools.lru_cache(maxsize=256)
def green_mask(s, T, V):
    """bool [V]: the ids of [0, V) that are green in the state ``s`` (kept: rows of one pass often share a context)."""
    return torch.tensor([is_green(s, v, T) for v in range(V)])


def params_of_table(table):
    """A namespace of what an int32 table holds: ``h``, ``T``, ``delta`` (an exact fp32 value), ``key``."""
    t = [v & 0xffffffff for v in table.cpu().tolist()]
    assert len(t) == TABLE_WORDS == t[3] and t[6] == 0 and t[7] == 0
    return SimpleNamespace(h=t[0], T=t[1], delta=struct.unpack("<f", struct.pack("<I", t[2]))[0], key=t[4] | (t[5] << 32))


def spec_of(wm):
    """The text ``Watermark.parse`` reads ``wm`` back from."""
    return f"key={wm.key},gamma={wm.gamma!r},delta={wm.delta!r},ctx={wm.context}"


def watermark_rows(logits, table, output_ids, base=None, base_sub=None, base_add=0, extra_ids=None, extra_mask=None):
    """``longspec_amd.ops.watermark_rows`` on CPU tensors (in place, exact; NOT idempotent: every call adds delta)."""
    p = params_of_table(table)
    x = logits if logits.dim() == 3 else logits.unsqueeze(1)
    b, R, V = x.shape
    texts = row_texts(b, R, output_ids, base, base_sub, base_add, extra_ids, extra_mask)
    delta = torch.tensor(p.delta, dtype=torch.float32)
    for z in range(b):
        for r in range(R):
            t = texts[z][r]
            if len(t) < p.h:
                continue
            s = state(p.key, t[len(t) - p.h:])
            row = x[z, r]
            sel = green_mask(s, p.T, V) & ~torch.isnan(row)
            row[sel] = (row[sel].float() + delta).to(x.dtype)
    return logits


def score(ids, key, gamma, h, length=None, unique=False):
    """(scored, green, z, flags) of the list ``ids``: the detector, one position at a time."""
    n = len(ids) if length is None else max(0, min(length, len(ids)))
    T = math.floor(gamma * 2 ** 32)
    p = T / 2 ** 32
    flags, seen, N, G = [-1] * len(ids), set(), 0, 0
    for c in range(h, n):
        u = u_of(state(key, ids[c - h:c]), ids[c])
        g = (u >> 32) < T
        flags[c] = int(g)
        if unique and u in seen:
            continue
        seen.add(u)
        N += 1
        G += int(g)
    z = (G - p * N) / math.sqrt(p * (1 - p) * N) if N else math.nan
    return N, G, z, flags


class Ops:
    """``dry_oracle.ops`` plus ``watermark_rows``: the operator namespace of the ``watermark=`` host-logic tests."""

    def __getattr__(self, name):
        return getattr(dry_oracle.ops, name)

    watermark_rows = staticmethod(watermark_rows)


ops = Ops()
