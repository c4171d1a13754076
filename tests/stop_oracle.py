"""Oracle of ``ops.stop_scan`` / ``ops.stop_ban_rows`` (``ls_stop_scan`` / ``ls_stop_ban_rows``): the definition of
``longspec_amd/stop.py`` in plain Python -- scan, cut, ban -- and an operator namespace layered on ``logprob_oracle.ops`` that
lets the host loops run with ``stop=`` on the CPU.  The operators read the ``Stop`` back out of its int32 table, so the table's
layout is part of what they check.  Lives under tests/: the product never imports it."""
import math

import logprob_oracle
from longspec_amd import Stop
from longspec_amd import stop as stop_mod


def matches_at(text, c, stop):
    """Listing-order numbers of the stops that match ``text`` (a list of ints) at column ``c``."""
    if c < stop.min_tokens:
        return []
    hits = [i for i, t in enumerate(stop.token_ids) if text[c] == t]
    for q, s in enumerate(stop.sequences):
        L = len(s)
        if L <= c + 1 and list(text[c - L + 1:c + 1]) == list(s):
            hits.append(len(stop.token_ids) + q)
    return hits


def scan(text, stop, first=0):
    """(length, which, match_start) of the first match at a column >= ``first`` of ``text``, or (-1, -1, -1)."""
    for c in range(first, len(text)):
        hits = matches_at(text, c, stop)
        if hits:
            return c + 1, hits[0], c - stop.stop_len(hits[0]) + 1
    return -1, -1, -1


def cut(row, n, stop, fill):
    """``oracle_cut``: ``row`` (a list, ``n`` text columns, the rest whatever the loop left) as a loop with ``stop=`` must
    return it -- the text up to ``length``, ``fill`` over the rest of the TEXT columns; with the triple."""
    length, which, start = scan(row[:n], stop)
    if length < 0:
        return list(row), (length, which, start)
    return list(row[:length]) + [fill] * (n - length) + list(row[n:]), (length, which, start)


def stop_of_table(table):
    """The ``Stop`` an int32 table was built from."""
    t = table.cpu().tolist()
    assert len(t) == stop_mod.TABLE_WORDS == t[3]
    ids = tuple(t[stop_mod.IDS_OFF:stop_mod.IDS_OFF + t[0]])
    offs = t[stop_mod.OFFS_OFF:stop_mod.OFFS_OFF + t[1] + 1]
    seqs = tuple(tuple(t[stop_mod.TOKS_OFF + offs[q]:stop_mod.TOKS_OFF + offs[q + 1]]) for q in range(t[1]))
    return Stop(ids, seqs, t[2])


def stop_scan(output_ids, table, stop_state, written, written_sub=None, written_add=0, num=None, num_const=1, fill=0, state=None,
              spec_mask=None, logprobs=None):
    """``longspec_amd.ops.stop_scan`` on CPU tensors (in place, exact)."""
    stop = stop_of_table(table)
    b, W = output_ids.shape
    for z in range(b):
        w = int(written[z]) - (int(written_sub[z]) if written_sub is not None else 0) + written_add
        w = max(0, min(w, W))
        length = int(stop_state[z, 0])
        if length < 0:
            n_new = max(0, min(int(num[z]) if num is not None else num_const, w))
            length, which, start = scan(output_ids[z, :w].tolist(), stop, first=w - n_new)
            if length < 0:
                continue
            stop_state[z, 0], stop_state[z, 1], stop_state[z, 2] = length, which, start
        if state is not None:
            state[z, 1] |= 2
        if w > length:
            output_ids[z, length:w] = fill
            if spec_mask is not None:
                spec_mask[z, length:w] = 0
            if logprobs is not None:
                logprobs.token[z, length:w] = float("nan")
                logprobs.top[z, length:w] = float("-inf")
                logprobs.top_ids[z, length:w] = -1


def stop_ban_rows(logits, table, base=None, base_sub=None, base_add=0, depth=None, tree_mask=None):
    """``longspec_amd.ops.stop_ban_rows`` on CPU tensors (in place, exact)."""
    stop = stop_of_table(table)
    x = logits if logits.dim() == 3 else logits.unsqueeze(1)
    b, R, V = x.shape
    for z in range(b):
        col0 = (int(base[z]) if base is not None else 0) - (int(base_sub[z]) if base_sub is not None else 0) + base_add
        for r in range(R):
            d = 0 if depth is None else r if depth == "row" else int((tree_mask[z, r, 1:] != 0).sum())
            if col0 + d < stop.min_tokens:
                for t in stop.token_ids:
                    if t < V:
                        x[z, r, t] = -math.inf
    return logits


class Ops:
    """``logprob_oracle.ops`` plus the two stop operators: the operator namespace of the ``stop=`` host-logic tests."""

    def __getattr__(self, name):
        return getattr(logprob_oracle.ops, name)

    stop_scan = staticmethod(stop_scan)
    stop_ban_rows = staticmethod(stop_ban_rows)


ops = Ops()
