"""``ops.guide_advance`` (``ls_guide_advance``) against the oracle (tests/guide_oracle.py), exactly: ``num`` of 0 / 1 / n /
None, n of 1 and 128, strided ``ids`` and ``num``, batch 1 and 3, walks that die mid-way, a start from -1, ids outside the
vocabulary, and the state the rows operator then reads."""
import numpy as np
import pytest
import torch

import guide_oracle as go
from longspec_amd import Guide

pytestmark = pytest.mark.gpu
DEV = "cuda"
V = 1023


@pytest.fixture(scope="module")
def ops():
    from longspec_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def guides():
    rng = np.random.default_rng(1)
    nx = rng.integers(0, 7, size=(7, 33))
    nx[rng.random((7, 33)) < 0.3] = -1
    nx[:, 0] = (np.arange(7) + 1) % 7
    v = np.arange(V - 50)
    return {"parity": Guide([[1, -1], [-1, 0]], np.arange(V) % 2),
            "c33": Guide(nx, np.where(v % 11 == 5, -1, v % 33), start=3)}       # ids >= V - 50 and every 11th: forbidden


def live_walk(g, s, n, rng):
    """n ids that keep state s inside the language."""
    out = []
    tc = g._classes_of(V)
    for _ in range(n):
        ok = tc >= 0
        ok[ok] = g.next[s, tc[ok]] >= 0
        t = int(rng.choice(np.flatnonzero(ok)))
        out.append(t)
        s = g.step(s, t, vocab=V)
    return out


def both(ops, table, state, ids, num):
    """The operator on the device and the oracle on copies; returns the new state (asserted equal)."""
    want = state.clone()
    go.guide_advance(want, table, ids, num)
    got = state.to(DEV)
    ops.guide_advance(got, table.to(DEV), ids.to(DEV) if ids.is_contiguous() else as_strided_on_device(ids),
                      None if num is None else (num.to(DEV) if num.is_contiguous() else as_strided_on_device(num)))
    torch.cuda.synchronize()
    assert got.cpu().tolist() == want.tolist(), (state.tolist(), num)
    return want


def as_strided_on_device(t):
    """The same view of a device copy of the tensor's whole storage: strides and offset survive the copy."""
    base = torch.empty(0, dtype=t.dtype).set_(t.untyped_storage()).to(DEV)
    return base.as_strided(t.shape, t.stride(), t.storage_offset())


@pytest.mark.parametrize("name", ["parity", "c33"])
@pytest.mark.parametrize("n", [1, 17, 128])
@pytest.mark.parametrize("b", [1, 3])
def test_the_walk_is_the_oracles(ops, name, n, b):
    g = guides()[name]
    table = g.table(V, "cpu")
    rng = np.random.default_rng(n + b)
    starts = [g.start, (g.start + 1) % g.states, -1][:b]
    ids = torch.tensor([live_walk(g, s, n, rng) if s >= 0 else rng.integers(0, V, n).tolist() for s in starts])
    state = torch.tensor(starts, dtype=torch.int32)
    # all n (None and num = n): every live row stays live
    after = both(ops, table, state, ids, None)
    assert all((a >= 0) == (s >= 0) for a, s in zip(after.tolist(), starts))
    assert both(ops, table, state, ids, torch.full((b,), n, dtype=torch.int64)).tolist() == after.tolist()
    # num = 0: nothing moves; num = 1; a different num per row, beyond n and negative clamped
    assert both(ops, table, state, ids, torch.zeros(b, dtype=torch.int64)).tolist() == starts
    both(ops, table, state, ids, torch.ones(b, dtype=torch.int64))
    both(ops, table, state, ids, torch.tensor([n // 2, n + 5, -3][:b]))
    # a walk that dies mid-way: a forbidden id, an id >= V, a negative id at position n // 2
    for bad in (V - 1 if name == "c33" else None, V, V + 1000, -1, -2 ** 40, 2 ** 40):
        broken = ids.clone()
        if bad is None:                   # parity: the id of the wrong parity
            broken[:, n // 2] = ids[:, n // 2] ^ 1
        else:
            broken[:, n // 2] = bad
        after = both(ops, table, state, broken, None)
        assert after.tolist() == [-1] * b
        short = both(ops, table, state, broken, torch.full((b,), n // 2, dtype=torch.int64))     # ... and not when num stops in front of it
        assert all((a >= 0) == (s >= 0) for a, s in zip(short.tolist(), starts))
    # strided ids (rows of a wider buffer) and a strided num (a column of the round's state)
    wide = torch.full((b, n + 9), -5, dtype=torch.int64)
    wide[:, 3:3 + n] = ids
    round_state = torch.tensor([[n, 0], [max(n - 1, 0), 1], [1, 1]][:b])
    both(ops, table, state, wide[:, 3:3 + n], round_state[:, 0])


def test_the_rows_operator_reads_the_advanced_state(ops):
    g = guides()["parity"]
    table = g.table(V, DEV)
    state = torch.tensor([0, 0], dtype=torch.int32, device=DEV)
    ops.guide_advance(state, table, torch.tensor([[4, 7, 10], [4, 7, 11]], device=DEV))
    assert state.tolist() == [1, -1]
    x = torch.zeros((2, V), dtype=torch.float16, device=DEV)
    ops.guide_rows(x, table, state)
    bad = torch.isinf(x)
    assert bad[0, 0::2].all() and not bad[0, 1::2].any() and not bad[1].any()          # odd ids next; the dead row keeps its bits


def test_argument_checks(ops):
    from longspec_amd import _C
    g = guides()["parity"]
    table = g.table(V, DEV)
    state = torch.zeros((2,), dtype=torch.int32, device=DEV)
    ids = torch.tensor([[2, 3], [2, 3]], device=DEV)
    num = torch.tensor([2, 1], device=DEV)
    good = dict(state=state, table=table, ids=ids, num=num)
    ops.guide_advance(**good)
    assert state.tolist() == [0, 1]
    for bad in (dict(state=state.long()), dict(state=state.view(2, 1)), dict(state=state.cpu()), dict(table=table[:7]), dict(table=table[1:]),
                dict(table=table.long()), dict(ids=ids.int()), dict(ids=ids[:1]), dict(num=num.int()), dict(num=num[:1]),
                dict(ids=torch.zeros((2, ops.GUIDE_MAX_EXTRA + 1), dtype=torch.int64, device=DEV)),
                dict(ids=torch.zeros((2, 0), dtype=torch.int64, device=DEV))):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises((TypeError, ValueError, RuntimeError)):
            ops.guide_advance(**kw)
    lib = _C.load()
    args = lambda **o: [o.get("state", state.data_ptr()), o.get("b", 2), o.get("table", table.data_ptr()), o.get("words", table.numel()),
                        o.get("ids", ids.data_ptr()), o.get("n", 2), o.get("ids_stride", 2), num.data_ptr(), o.get("num_stride", 1), None]
    for o in (dict(state=None), dict(table=None), dict(ids=None), dict(b=0), dict(n=0), dict(n=129), dict(words=7), dict(ids_stride=-1),
              dict(num_stride=-1), dict(table=table.data_ptr() + 8)):
        assert lib.ls_guide_advance(*args(**o)) == _C.LS_ERR_INVALID_ARG, o
    torch.cuda.synchronize()
    assert state.tolist() == [0, 1]
    # a header that does not fit its words: every state becomes -1
    broken = table.clone()
    broken[0] = 3
    ops.guide_advance(state, broken, ids)
    assert state.tolist() == [-1, -1]
