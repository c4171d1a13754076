"""The watermark's definition on the CPU: the known answers of the contract against the plain-Python oracle
(tests/watermark_oracle.py), ``Watermark.detect`` on CPU tensors -- the vectorised restatement in longspec_amd/watermark.py --
against that oracle (flags, counts, ``unique`` on texts with planted repeats, ``lengths``), the oracle's row operator on a
hand-made row, the argument refusals, ``parse`` round trips and the table's layout."""
import math
import struct

import pytest
import torch

import watermark_oracle as wo
from longspec_amd import Watermark
from longspec_amd import watermark as wm_mod

KEY = 0x0123456789ABCDEF


def test_known_answers():
    assert wo.fin((KEY + wo.M1) & wo.MASK) == 0x157a3807a48faa9d == wo.state(KEY, [])
    assert wo.state(KEY, [42]) == 0xc9dc5224ee052e4e
    assert wo.state(KEY, [7, 42]) == 0x7b27bfd5b546ca6f
    assert wo.state(KEY, [-1]) == 0x8128563c99490a49
    assert wo.green_ids(KEY, [42], 0.25, 64) == [0, 4, 11, 13, 15, 21, 22, 25, 29, 31, 33, 35, 53, 54, 58]
    assert wo.green_ids(KEY, [7, 42], 0.25, 64) == [0, 2, 3, 4, 5, 6, 9, 28, 33, 41, 45, 51, 60, 62]


def test_detect_on_the_cpu_gives_the_known_green_lists():
    for ctx, want in (([42], [0, 4, 11, 13, 15, 21, 22, 25, 29, 31, 33, 35, 53, 54, 58]),
                      ([7, 42], [0, 2, 3, 4, 5, 6, 9, 28, 33, 41, 45, 51, 60, 62])):
        wm = Watermark(KEY, 0.25, 2.0, context=len(ctx))
        ids = torch.tensor([ctx + [v] for v in range(64)])
        got = wm.detect(ids)
        assert got.flags[:, :len(ctx)].eq(-1).all() and got.scored.tolist() == [1] * 64
        assert [v for v in range(64) if int(got.flags[v, -1]) == 1] == want == [v for v in range(64) if int(got.green[v])]
    got = Watermark(KEY, 0.25, context=1).detect(torch.tensor([-1, 3]))             # an id outside every vocabulary
    assert int(got.flags[0, 1]) == int(wo.is_green(0x8128563c99490a49, 3, 2 ** 30))


def texts(n, vocab, seed, repeats):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, vocab, (n,), generator=g)
    if repeats and n >= 40:
        x[n - 12:n] = x[5:17]                                             # a planted repeat of 12 tokens ...
        x[20:26] = x[5:11]                                                # ... and one of 6
    return x


@pytest.mark.parametrize("h", [1, 2, 3, 8])
@pytest.mark.parametrize("gamma", [0.25, 0.5, 0.9])
def test_detect_on_the_cpu_is_the_oracle(h, gamma):
    wm = Watermark(KEY + h, gamma, 2.0, context=h)
    for n, vocab, repeats in ((0, 50, False), (h, 50, False), (h + 1, 50, False), (97, 50000, True), (300, 7, True), (1025, 128256, True)):
        rows = torch.stack([texts(n, vocab, 10 * n + z, repeats) for z in range(3)]) if n else torch.zeros((3, 0), dtype=torch.int64)
        if n > 2:
            rows[1, 1] = -5                                               # ids outside the vocabulary take part as they are
            rows[2, n - 1] = 2 ** 40
        lengths = [n, max(n - 3, 0), n + 7]
        for unique in (False, True):
            for lens in (None, lengths):
                got = wm.detect(rows, lengths=lens, unique=unique)
                assert got.scored.dtype == torch.int32 and got.green.dtype == torch.int32 and got.z.dtype == torch.float64
                assert got.flags.dtype == torch.int8 and tuple(got.flags.shape) == (3, n)
                for z in range(3):
                    N, G, zz, flags = wo.score(rows[z].tolist(), wm.key, gamma, h, None if lens is None else lens[z], unique)
                    assert (int(got.scored[z]), int(got.green[z])) == (N, G), (n, z, unique, lens)
                    assert got.flags[z].tolist() == flags
                    assert (math.isnan(zz) and math.isnan(float(got.z[z]))) or abs(zz - float(got.z[z])) < 1e-12
            if repeats and h <= 3:
                a, b = wm.detect(rows, unique=False), wm.detect(rows, unique=True)
                assert (b.scored < a.scored).all(), "the planted repeats must count once"
    one = wm.detect(texts(97, 50, 3, True))                               # [n]: one row
    assert tuple(one.flags.shape) == (1, 97) and tuple(one.scored.shape) == (1,)


def test_a_loop_cannot_inflate_z():
    wm = Watermark(KEY, 0.25, 2.0, context=2)
    s = wo.state(KEY, [5, 6])
    v = next(v for v in range(100) if wo.is_green(s, v, wm.threshold) and wo.is_green(wo.state(KEY, [6, v]), 5, wm.threshold)
             and wo.is_green(wo.state(KEY, [v, 5]), 6, wm.threshold))
    loop = torch.tensor([5, 6, v] * 40)                                   # three green positions, said forty times
    plain, once = wm.detect(loop), wm.detect(loop, unique=True)
    assert int(plain.green[0]) == int(plain.scored[0]) == 118 and float(plain.z[0]) > 18
    assert int(once.green[0]) == int(once.scored[0]) == 3 and float(once.z[0]) == pytest.approx(3.0)


def test_the_oracles_row_operator():
    V = 64
    wm = Watermark(KEY, 0.25, 1000.0, context=1)
    table = wm.table(V, "cpu")
    row = torch.zeros((1, V), dtype=torch.float16)
    row[0, 0], row[0, 4], row[0, 11], row[0, 13] = 65000.0, float("nan"), -math.inf, -0.0
    before = row.clone()
    out = torch.tensor([[9, 42, 3]])
    i32 = lambda v: torch.tensor([v], dtype=torch.int32)
    assert torch.equal(wo.watermark_rows(row.clone(), table, out, base=i32(0)).view(torch.int16), before.view(torch.int16))     # m < h
    got = wo.watermark_rows(row.clone(), table, out, base=i32(2))
    green = [0, 4, 11, 13, 15, 21, 22, 25, 29, 31, 33, 35, 53, 54, 58]
    assert got[0, 0] == math.inf and math.isnan(float(got[0, 4])) and got[0, 11] == -math.inf and float(got[0, 13]) == 1000.0
    assert [v for v in range(V) if float(got[0, v]) == 1000.0] == green[3:] and not got[0, [v for v in range(V) if v not in green]].any()
    # the path takes over from the columns, and a second call adds delta again
    ids, mask = torch.tensor([[7, 42]]), torch.tensor([[0, 0], [1, 0], [1, 1]])
    rows = torch.zeros((1, 3, V), dtype=torch.bfloat16)
    two = Watermark(KEY, 0.25, 2.0, context=2)
    wo.watermark_rows(rows, two.table(V, "cpu"), out, base=i32(1), extra_ids=ids, extra_mask=mask)
    assert not rows[0, 0].any()                                           # one token, h = 2
    assert rows[0, 1].nonzero().flatten().tolist() == wo.green_ids(KEY, [9, 7], 0.25, V)       # the seam: a column, then the path
    assert rows[0, 2].nonzero().flatten().tolist() == [0, 2, 3, 4, 5, 6, 9, 28, 33, 41, 45, 51, 60, 62]
    wo.watermark_rows(rows, two.table(V, "cpu"), out, base=i32(1), extra_ids=ids, extra_mask=mask)
    assert set(rows[0, 2].tolist()) == {0.0, 4.0}


def test_argument_refusals():
    for bad in (dict(key=1.0), dict(key="1"), dict(key=True), dict(key=1, gamma="0.25"), dict(key=1, delta=None), dict(key=1, context=1.0),
                dict(key=1, context=True), dict(key=1, gamma=True)):
        with pytest.raises(TypeError):
            Watermark(**bad)
    for bad in (dict(key=-1), dict(key=2 ** 64), dict(key=1, gamma=0.0), dict(key=1, gamma=1.0), dict(key=1, gamma=2.0 ** -33),
                dict(key=1, gamma=-0.5), dict(key=1, gamma=math.nan), dict(key=1, delta=0.0), dict(key=1, delta=-1.0),
                dict(key=1, delta=math.inf), dict(key=1, delta=math.nan), dict(key=1, delta=1e39), dict(key=1, context=0),
                dict(key=1, context=9)):
        with pytest.raises(ValueError):
            Watermark(**bad)
    assert Watermark(0, 2.0 ** -32).threshold == 1 and Watermark(2 ** 64 - 1, 1.0 - 2.0 ** -32).threshold == 2 ** 32 - 1
    with pytest.raises(TypeError):
        Watermark(1).detect(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError):
        Watermark(1).detect([1, 2, 3])
    with pytest.raises(TypeError):
        Watermark(1).detect(torch.zeros((2, 4), dtype=torch.int64), lengths=[1, 2, 3])


def test_object_protocol_and_parse_round_trips(monkeypatch):
    a, b = Watermark(KEY, 0.25, 2.0, 1), Watermark(KEY)
    assert a == b and hash(a) == hash(b) and a != Watermark(KEY, context=2) and a != Watermark(KEY + 1) and a != "x"
    assert "0x123456789abcdef" in repr(a) and "gamma=0.25" in repr(a) and "context=1" in repr(a)
    for wm in (a, Watermark(0), Watermark(2 ** 64 - 1, 0.1, 0.3, 8), Watermark(5, 1 / 3, 1e-3, 4)):
        assert Watermark.parse(wo.spec_of(wm)) == wm
    assert Watermark.parse("key=0x10") == Watermark(16) and Watermark.parse(" ctx=3 , key=7 ") == Watermark(7, context=3)
    for bad in ("", "gamma=0.25", "key=1,key=2", "key=1,what=2", "key=x", "key=1,gamma=", "key", "key=1,ctx=1.5", "key=1;gamma=0.5"):
        with pytest.raises(ValueError, match=wm_mod.WATERMARK_ENV):
            Watermark.parse(bad)
    with pytest.raises(ValueError):
        Watermark.parse("key=1,ctx=9")
    monkeypatch.delenv(wm_mod.WATERMARK_ENV, raising=False)
    assert wm_mod.env_watermark() is None and wm_mod.resolve(None, None, True) is None
    monkeypatch.setenv(wm_mod.WATERMARK_ENV, "key=1,gamma=0.25,delta=2")
    assert wm_mod.env_watermark() == Watermark(1) == wm_mod.resolve(None, None, True)
    assert wm_mod.resolve(None, 0.5, True) is None and wm_mod.resolve(None, None, False) is None
    assert wm_mod.resolve(a, None, True) is a
    with pytest.raises(ValueError, match="temperature"):
        wm_mod.resolve(a, 0.5, True)
    with pytest.raises(TypeError, match="longspec_amd.Watermark"):
        wm_mod.resolve("key=1", None, True)


def test_table_layout():
    wm = Watermark(0xFEDCBA9876543210, 0.75, 2.5, context=5)
    t = wm.table(1000, "cpu")
    assert t.dtype == torch.int32 and tuple(t.shape) == (8,) == (wm_mod.TABLE_WORDS,)
    w = [v & 0xffffffff for v in t.tolist()]
    assert w[0] == 5 and w[1] == math.floor(0.75 * 2 ** 32) == 0xC0000000 and w[3] == 8 and w[6] == w[7] == 0
    assert struct.unpack("<f", struct.pack("<I", w[2]))[0] == 2.5
    assert w[4] == 0x76543210 and w[5] == 0xFEDCBA98
    p = wo.params_of_table(t)
    assert (p.h, p.T, p.delta, p.key) == (5, wm.threshold, 2.5, wm.key) and wm.rate == 0.75
    assert wo.params_of_table(Watermark(KEY, 0.1).table(5, "cpu")).T == math.floor(0.1 * 2 ** 32)
