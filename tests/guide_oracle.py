"""Oracle of ``ops.guide_rows`` / ``ops.guide_advance`` (``ls_guide_rows`` / ``ls_guide_advance``): the definition of
``longspec_amd/guide.py`` in plain Python, and an operator namespace layered on ``ban_oracle.ops`` that lets every host loop run
with ``guide=`` on the CPU.  The operators read the automaton back out of the int32 table, so the table's layout is part of what
they check.  Lives under tests/: the product never imports it."""
from types import SimpleNamespace

import numpy as np
import torch

import ban_oracle
from longspec_amd import guide as guide_mod

NINF = {torch.float16: 0xfc00, torch.bfloat16: 0xff80}


def parse(table):
    """The fields of an int32 guide table, unvalidated: S, C, start, vocab, cls (int [vocab], -1 = forbidden), next [S, C]."""
    t = table.cpu().numpy()
    S, C, start, vocab, words = (int(v) for v in t[:5])
    assert words == t.size and not t[5:8].any()
    K = guide_mod.class_words(vocab)
    assert K % 4 == 0 and guide_mod.HEADER_WORDS + K + S * C == words
    area = t[guide_mod.HEADER_WORDS:guide_mod.HEADER_WORDS + K].astype("<i4").view("<u2").astype(np.int64)
    assert (area[vocab:] == guide_mod.NO_CLASS).all()
    cls = np.where((area[:vocab] == guide_mod.NO_CLASS) | (area[:vocab] >= C), -1, area[:vocab])
    nxt = t[guide_mod.HEADER_WORDS + K:].reshape(S, C).astype(np.int64)
    nxt = np.where((nxt < 0) | (nxt >= S), -1, nxt)
    return SimpleNamespace(S=S, C=C, start=start, vocab=vocab, cls=cls, next=nxt)


def step(g, s, token, vocab=None):
    vocab = g.vocab if vocab is None else min(vocab, g.vocab)
    if s < 0 or s >= g.S or token < 0 or token >= vocab or g.cls[token] < 0:
        return -1
    return int(g.next[s, g.cls[token]])


def walk(g, s, tokens, vocab=None):
    """``s`` walked along ``tokens`` through the parsed table ``g``; -1 once dead."""
    s = int(s)
    if s < -1 or s >= g.S:
        s = -1
    for t in tokens:
        s = step(g, s, int(t), vocab)
    return s


def paths(b, rows, extra_ids=None, extra_mask=None):
    """[z][r] -> the ordered path of row r of batch z."""
    out = []
    for z in range(b):
        per_row = []
        for r in range(rows):
            path = []
            if extra_ids is not None and extra_ids.shape[-1] > 0:
                mask = extra_mask[z, r] if extra_mask.dim() == 3 else extra_mask[r]
                path = [int(extra_ids[z, c]) for c in range(extra_ids.shape[-1]) if int(mask[c]) != 0]
            per_row.append(path)
        out.append(per_row)
    return out


def row_states(g, V, state, rows, extra_ids=None, extra_mask=None):
    """[z][r] -> the state of row r of batch z: ``state[z]`` walked along the row's path."""
    b = state.shape[0]
    return [[walk(g, int(state[z]), p, V) for p in per_row] for z, per_row in enumerate(paths(b, rows, extra_ids, extra_mask))]


def allowed(g, s, V):
    """bool [V]: the ids a live state ``s`` allows."""
    ok = np.zeros(V, dtype=bool)
    n = min(V, g.vocab)
    live = g.cls[:n] >= 0
    ok[:n][live] = g.next[s, g.cls[:n][live]] >= 0
    return ok


def guide_rows(logits, table, state, extra_ids=None, extra_mask=None):
    """``longspec_amd.ops.guide_rows`` on CPU tensors, bit level: returns a NEW tensor of the shape of ``logits``."""
    g = parse(table)
    out = logits.clone()
    x = out if out.dim() == 3 else out.unsqueeze(1)
    b, R, V = x.shape
    states = row_states(g, V, state.cpu(), R, None if extra_ids is None else extra_ids.cpu(),
                        None if extra_mask is None else extra_mask.cpu())
    if logits.dtype in NINF:
        bits, ninf = x.view(torch.int16), NINF[logits.dtype] - 65536
    else:                                                                     # (a host loop on fp32 logits)
        bits, ninf = x, float("-inf")
    for z in range(b):
        for r in range(R):
            if states[z][r] < 0:
                continue
            bad = torch.from_numpy(~allowed(g, states[z][r], V))
            bits[z, r][bad] = ninf
    return out


def guide_advance(state, table, ids, num=None):
    """``longspec_amd.ops.guide_advance`` on CPU tensors (in place)."""
    g = parse(table)
    b = state.shape[0]
    ids = ids.view(b, -1)
    for z in range(b):
        n = ids.shape[1] if num is None else max(0, min(int(num[z]), ids.shape[1]))
        state[z] = walk(g, int(state[z]), ids[z, :n].tolist())


def _rows_in_place(logits, table, state, extra_ids=None, extra_mask=None):
    logits.copy_(guide_rows(logits, table, state, extra_ids, extra_mask))
    return logits


class Ops:
    """``ban_oracle.ops`` plus the two guide operators: the operator namespace of the ``guide=`` host-logic tests."""

    def __getattr__(self, name):
        return getattr(ban_oracle.ops, name)

    guide_rows = staticmethod(_rows_in_place)
    guide_advance = staticmethod(guide_advance)


ops = Ops()
