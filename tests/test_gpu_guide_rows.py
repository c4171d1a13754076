"""``ops.guide_rows`` (``ls_guide_rows``) against the oracle (tests/guide_oracle.py), the whole buffer bit for bit -- the gaps
between the rows and the guards around it included (the ``guarded_logits`` construction of test_gpu_ban_rows.py): V = 1023 (a
ragged tail, rows that are only 2-byte aligned), 1024 and 128 256, 1 / 5 / 69 rows with padded row and batch strides, batch 1 and
3, fp16 and bf16, the mask as [R, C] and [b, R, C], the level-major 4-branch tree and the chain, 0 and 128 extra columns.  The
paths are planted so that rows stay live, die at depth 1, die at the last depth, die of an id >= V and of a negative id, and
start from a committed state of -1; the guides so that groups of eight ids are wholly forbidden, wholly allowed and mixed --
each kind asserted to occur."""
import numpy as np
import pytest
import torch

import guide_oracle as go
from longspec_amd import Guide
from test_gpu_ban_rows import DEV, GUARD, guarded_logits

pytestmark = pytest.mark.gpu
NAMES = ["all", "one", "parity", "c33", "minus1", "short", "c16384"]
_guides, _tables = {}, {}


@pytest.fixture(scope="module")
def ops():
    from longspec_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def guide_of(name, V):
    """The guides of the module's docstring, for a vocabulary of V ids; built once."""
    if (name, V) in _guides:
        return _guides[name, V]
    rng = np.random.default_rng(len(name) * 1000 + V % 1000)
    v = np.arange(V)
    if name == "all":                     # S = 1, C = 1, everything allowed: nothing is written
        g = Guide([[0]], np.zeros(V, dtype=np.int64))
    elif name == "one":                   # everything but one id forbidden
        tc = np.full(V, -1)
        tc[V // 2] = 0
        g = Guide([[0]], tc)
    elif name == "parity":                # even and odd ids alternate: every group of eight is mixed
        g = Guide([[1, -1], [-1, 0]], v % 2)
    elif name == "short":                 # token_class shorter than V: the tail is forbidden in every state
        g = Guide([[1, -1], [-1, 0]], v[:V - 100] % 2, start=1)
    elif name in ("c33", "minus1"):       # C = 33: the allow bits are no multiple of 32; groups of one class, then mixed ones
        nx = rng.integers(0, 5, size=(5, 33))
        nx[rng.random((5, 33)) < 0.45] = -1
        nx[:, 0] = (np.arange(5) + 1) % 5
        tc = np.where(v < V // 2, (v // 8) % 33, v % 33)
        if name == "minus1":              # a class area with -1 entries
            tc = np.where(v % 7 == 3, -1, tc)
        g = Guide(nx, tc, start=2)
    else:                                 # C = 16384, S = 1024: a 64 MB transition area
        if "nx" not in _guides:           # (one transition area for every V)
            rng = np.random.default_rng(16384)
            nx = rng.integers(0, 1024, size=(1024, 16384), dtype=np.int32)
            nx[rng.integers(0, 2, size=nx.shape, dtype=np.int8) == 0] = -1
            nx[:, 0] = (np.arange(1024) + 1) % 1024
            _guides["nx"] = nx
        g = Guide(_guides["nx"], v % 16384, start=7)
    _guides[name, V] = g
    return g


def tables_of(name, V):
    if (name, V) not in _tables:
        t = guide_of(name, V).table(V, "cpu")
        _tables[name, V] = (t, t.to(DEV))
    return _tables[name, V]


def ok_mask(g, s, V):
    tc = g._classes_of(V)
    ok = tc >= 0
    ok[ok] = g.next[s, tc[ok]] >= 0
    return ok


def plant(g, V, state, R, b, rng, shift):
    """(extra_ids [b, C], extra_mask [b, R, C]) of the level-major tree of test_gpu_ban_rows.tree -- 69 rows: 4 branches of
    depth 17; 5 and 129 rows: the chain -- with branch j of batch row z planted by its variant (z + j + shift) % 4: 0 stays in the
    language, 1 leaves it at depth 1, 2 at the last depth, 3 holds an id outside [0, V) at depth 2 (z even: >= V; odd: negative)."""
    if R == 1:
        return None, None, 0
    B = 4 if R == 69 else 1
    gamma, C = (R - 1) // B, R - 1
    ids = torch.zeros((b, C), dtype=torch.int64)
    mask = torch.zeros((b, R, C), dtype=torch.int64)
    for j in range(B):
        for d in range(1, gamma + 1):
            for dd in range(1, d + 1):
                mask[:, 1 + (d - 1) * B + j, (dd - 1) * B + j] = 1 + dd        # (any non-zero value selects)
    cache = {}
    for z in range(b):
        for j in range(B):
            variant, s = (z + j + shift) % 4, int(state[z])
            for d in range(1, gamma + 1):
                if s >= 0 and s not in cache:
                    cache[s] = ok_mask(g, s, V)
                if variant == 3 and d == min(2, gamma):
                    t = V + 3 + z if z % 2 == 0 else -1 - z
                elif s < 0:
                    t = int(rng.integers(0, V))
                else:
                    kill = (variant == 1 and d == 1) or (variant == 2 and d == gamma)
                    pool = np.flatnonzero(~cache[s] if kill else cache[s])
                    t = int(rng.choice(pool)) if pool.size else V             # (a guide that forbids nothing: only an id >= V kills)
                ids[z, (d - 1) * B + j] = t
                s = g.step(s, t, vocab=V)
    return ids, mask, gamma


def kinds_of(g, V, state, R, ids, mask, gamma):
    """Which kinds of row and of group a case holds."""
    seen = set()
    for z, rows in enumerate(go.paths(state.shape[0], R, ids, mask)):
        for path in rows:
            s = int(state[z])
            if s < 0:
                seen.add("committed -1")
                continue
            for k, t in enumerate(path):
                s = g.step(s, t, vocab=V)
                if s < 0:
                    seen.add("killed at depth 1" if k == 0 else "killed at the last depth" if k == gamma - 1 else "killed inside")
                    if t >= V:
                        seen.add("killed by an id >= V")
                    if t < 0:
                        seen.add("killed by a negative id")
                    break
            else:
                seen.add("live")
                bad = np.zeros((V + 7) // 8 * 8, dtype=bool)
                bad[:V] = ~ok_mask(g, s, V)
                per = bad[:V // 8 * 8].reshape(-1, 8).sum(axis=1)
                seen |= {"wholly forbidden"} if (per == 8).any() else set()
                seen |= {"wholly allowed"} if (per == 0).any() else set()
                seen |= {"mixed"} if ((per > 0) & (per < 8)).any() else set()
    return seen


def check(ops, b, R, V, dtype, name, state, ids, mask, tables=None):
    """One call on the device and in the oracle; the whole guarded buffer must agree.  Returns the elements changed."""
    flat, shape, strides = guarded_logits(b, R, V, dtype)
    flat_c = flat.clone()
    before = flat_c.clone()
    flat_d = flat_c.to(DEV)
    x_c, x_d = flat_c.as_strided(shape, strides, GUARD), flat_d.as_strided(shape, strides, GUARD)
    if R == 1 and ids is None:
        x_c, x_d = x_c[:, 0], x_d[:, 0]                                   # the two-dimensional form
    t_c, t_d = tables or tables_of(name, V)
    dv = lambda t: None if t is None else t.to(DEV)
    state_d = state.to(DEV)
    go.ops.guide_rows(x_c, t_c, state, ids, mask)
    got = ops.guide_rows(x_d, t_d, state_d, extra_ids=dv(ids), extra_mask=dv(mask))
    assert got is x_d
    torch.cuda.synchronize()
    assert torch.equal(state_d.cpu(), state)                              # the committed state is read only
    assert torch.equal(flat_c.view(torch.int16), flat_d.cpu().view(torch.int16))
    changed = flat_c.view(torch.int16) != before.view(torch.int16)
    ninf = -0x0400 if dtype == torch.float16 else -0x0080
    assert (flat_c.view(torch.int16)[changed] == ninf).all()
    return int(changed.sum())


def states_for(g, b, k, rng):
    """Committed states: batch 1 the start state; batch 3 three different ones, the last -1 in every second case."""
    if b == 1:
        return torch.tensor([g.start], dtype=torch.int32)
    others = [s for s in range(min(g.states, 64)) if s != g.start] or [g.start]
    s1 = others[int(rng.integers(0, len(others)))]
    return torch.tensor([g.start, s1, -1 if (k // 2) % 2 else others[-1]], dtype=torch.int32)


LIVE = {"live", "wholly forbidden", "wholly allowed", "mixed"}
KILLS = {"killed at depth 1", "killed at the last depth", "killed by an id >= V", "killed by a negative id", "committed -1"}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("V", [1023, 1024])
def test_the_whole_buffer_is_the_oracles_bit_for_bit(ops, V, dtype):
    rng = np.random.default_rng(V)
    seen, k = set(), 0
    for name in NAMES[:-1]:
        g = guide_of(name, V)
        for R in (1, 5, 69):
            for b in (1, 3):
                state = states_for(g, b, k, rng)
                ids, mask, gamma = plant(g, V, state, R, b, rng, shift=k)
                n = check(ops, b, R, V, dtype, name, state, ids, mask if mask is None or k % 3 else mask[0])
                seen |= kinds_of(g, V, state, R, ids, mask, gamma)
                assert name != "all" or n == 0                             # everything allowed: nothing is written
                k += 1
    print(f"V={V}: kinds seen: {sorted(seen)}")
    assert LIVE | KILLS <= seen, sorted((LIVE | KILLS) - seen)


PLAN = [(69, 3, "parity"), (69, 1, "c16384"), (5, 1, "c33"), (1, 3, "short"), (69, 1, "one"), (5, 3, "all"), (5, 3, "minus1")]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("R,b,name", PLAN, ids=[f"{n}-{R}x{b}" for R, b, n in PLAN])
def test_the_real_vocabulary(ops, R, b, name, dtype):
    V = 128256
    k = PLAN.index((R, b, name)) + (dtype == torch.bfloat16)
    rng = np.random.default_rng(k)
    g = guide_of(name, V)
    state = states_for(g, b, k, rng)
    ids, mask, gamma = plant(g, V, state, R, b, rng, shift=k)
    n = check(ops, b, R, V, dtype, name, state, ids, mask if mask is None or k % 3 else mask[0])
    seen = kinds_of(g, V, state, R, ids, mask, gamma)
    print(f"{name} R={R} b={b}: {n} elements written; kinds seen: {sorted(seen)}")
    assert "live" in seen and (n == 0) == (name == "all")
    if R == 69:
        assert {"killed at depth 1", "killed at the last depth"} <= seen
    if name == "c16384":
        assert tables_of(name, V)[0].numel() * 4 > 64 * 2 ** 20 and {"wholly allowed", "mixed"} <= seen
    if name in ("one", "short"):
        assert "wholly forbidden" in seen


def test_the_largest_guide_at_a_ragged_vocabulary(ops):
    V, name = 1023, "c16384"
    rng = np.random.default_rng(5)
    g = guide_of(name, V)
    state = torch.tensor([7, 1023, 500], dtype=torch.int32)
    ids, mask, gamma = plant(g, V, state, 5, 3, rng, shift=0)
    assert check(ops, 3, 5, V, torch.float16, name, state, ids, mask) > 0
    assert "live" in kinds_of(g, V, state, 5, ids, mask, gamma)


@pytest.mark.parametrize("name", ["parity", "minus1"])
def test_the_longest_path_of_128_columns(ops, name):
    """n_extra = LS_GUIDE_MAX_EXTRA: the path is assembled over two full steps of 64 mask columns, the chain through the table is
    128 long."""
    V, R = 1023, 129
    assert R - 1 == ops.GUIDE_MAX_EXTRA
    rng = np.random.default_rng(11)
    g = guide_of(name, V)
    seen = set()
    for shift, dtype in ((0, torch.float16), (1, torch.bfloat16), (2, torch.float16)):
        state = states_for(g, 3, 0, rng)
        ids, mask, gamma = plant(g, V, state, R, 3, rng, shift=shift)
        assert gamma == 128
        assert check(ops, 3, R, V, dtype, name, state, ids, mask[0] if shift else mask) > 0
        seen |= kinds_of(g, V, state, R, ids, mask, gamma)
    assert {"live", "killed at depth 1", "killed at the last depth", "killed by an id >= V", "killed by a negative id"} <= seen


def test_hand_made_tables_index_nothing_out_of_range(ops):
    """A class >= C, a state outside [-1, S) in the transition area and in ``state``, and a header that does not fit its words:
    counted as forbidden / -1 / every row dead, as the oracle counts them."""
    V, R = 1023, 5
    g = guide_of("c33", V)
    t = g.table(V, "cpu")
    K = (V + 1) // 2
    K = (K + 3) // 4 * 4
    rng = np.random.default_rng(2)
    state = torch.tensor([2, 0, 4], dtype=torch.int32)
    ids, mask, gamma = plant(g, V, state, R, 3, rng, shift=0)
    bad = t.clone()
    area = bad[8:8 + K].numpy().view("<u2")
    area[5], area[64], area[700] = 33, 40000, 0xFFFE                       # classes the table does not have
    nxt = bad[8 + K:].view(5, 33)
    nxt[2, 0], nxt[0, 1], nxt[4, 2], nxt[1, 3] = 5, 2 ** 31 - 1, -7, -2 ** 31   # states outside [-1, S)
    p = go.parse(bad)
    assert p.cls[5] == -1 and p.cls[64] == -1 and p.next[2, 0] == -1 and p.next[4, 2] == -1
    for st in (state, torch.tensor([5, -2, 2 ** 31 - 1], dtype=torch.int32)):     # the second: every committed state is out of range
        n = check(ops, 3, R, V, torch.float16, None, st, ids, mask, tables=(bad, bad.to(DEV)))
        assert (n > 0) == (st is state)
    # a header whose areas do not fit: S, C, vocab, each in turn -- nothing is written
    for word, value in ((0, 6), (0, 0), (1, 34), (1, 0), (1, 16385), (3, V + 9), (3, 0), (0, 2 ** 31 - 1), (1, -1)):
        broken = t.clone()
        broken[word] = value
        flat, shape, strides = guarded_logits(3, R, V, torch.float16)
        flat_d = flat.to(DEV)
        ops.guide_rows(flat_d.as_strided(shape, strides, GUARD), broken.to(DEV), state.to(DEV), extra_ids=ids.to(DEV),
                       extra_mask=mask.to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(flat_d.cpu().view(torch.int16), flat.view(torch.int16)), (word, value)


def test_argument_checks(ops):
    from longspec_amd import _C
    V = 64
    table = Guide([[1, -1], [-1, 0]], np.arange(V) % 2).table(V, DEV)
    x = torch.zeros((2, 3, V), dtype=torch.float16, device=DEV)
    state = torch.zeros((2,), dtype=torch.int32, device=DEV)
    ids = torch.tensor([[3, 4], [5, 6]], device=DEV)
    mask = torch.ones((2, 3, 2), dtype=torch.int64, device=DEV)
    good = dict(logits=x, table=table, state=state, extra_ids=ids, extra_mask=mask)
    assert ops.guide_rows(**good) is x
    for bad in (dict(logits=x.float()), dict(logits=x.transpose(1, 2)), dict(logits=x.cpu()), dict(logits=x.view(-1).as_strided((2, 3, V), (8, 8, 1))),
                dict(table=table[:7]), dict(table=table.long()), dict(table=table[1:]), dict(table=table.cpu()),
                dict(state=state.long()), dict(state=state[:1]), dict(state=state.view(2, 1)),
                dict(extra_mask=None), dict(extra_ids=None), dict(extra_ids=ids.int()), dict(extra_ids=ids[:1]),
                dict(extra_mask=mask.int()), dict(extra_mask=mask[:, :2]), dict(extra_mask=mask[:1]), dict(extra_mask=mask[:, :, :1]),
                dict(extra_ids=torch.zeros((2, ops.GUIDE_MAX_EXTRA + 1), dtype=torch.int64, device=DEV),
                     extra_mask=torch.zeros((3, ops.GUIDE_MAX_EXTRA + 1), dtype=torch.int64, device=DEV))):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises((TypeError, ValueError, RuntimeError)):
            ops.guide_rows(**kw)
    # the C entry point refuses before any launch
    lib = _C.load()
    args = lambda **o: [o.get("logits", x.data_ptr()), o.get("b", 2), o.get("rows", 3), o.get("vocab", V), o.get("dtype", _C.LS_F16), 3 * V,
                        o.get("stride_r", V), o.get("table", table.data_ptr()), o.get("words", table.numel()), o.get("state", state.data_ptr()),
                        ids.data_ptr(), 2, o.get("mask", mask.data_ptr()), 6, 2, o.get("n_extra", 2), None]
    before = x.clone()
    for o in (dict(words=7), dict(logits=None), dict(table=None), dict(state=None), dict(dtype=99), dict(b=0), dict(rows=0), dict(rows=65536),
              dict(vocab=0), dict(stride_r=V - 1), dict(n_extra=-1), dict(n_extra=129), dict(mask=None), dict(table=table.data_ptr() + 4),
              dict(logits=x.data_ptr() + 1)):
        assert lib.ls_guide_rows(*args(**o)) == _C.LS_ERR_INVALID_ARG, o
    assert lib.ls_guide_rows(*args()) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, before)                                         # (the same call again: -inf stays -inf)
