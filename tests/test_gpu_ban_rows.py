"""``ops.ban_rows`` (``ls_ban_rows``) against the oracle (tests/ban_oracle.py), the whole buffer bit for bit -- the gaps between
the rows and the guards around it included: V = 1023 and 128 256, 1 / 5 / 69 rows with padded row and batch strides, batch 1
and 3, fp16 and bf16, the mask as [R, C] and [b, R, C], text widths around n and around the scan's chunk edges, n = 1 / 2 / 4 /
16, 0 / 1 / 64 sequences of 1 / 2 / 16 tokens, ids outside the vocabulary in text and table, NaN payloads and -0.0 in the
logits.  Texts are drawn from 8 ids and end in a period-3 stretch that one branch of the tree continues, so that matches lie
wholly in the text, across a chunk edge, wholly in a path, and across the text / path boundary -- each asserted to occur."""
import pytest
import torch

import ban_oracle as bo
from longspec_amd import Ban
from longspec_amd import ban as ban_mod

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 16
NS = [1, 2, 4, 16]


@pytest.fixture(scope="module")
def ops():
    from longspec_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


_base = {}


def guarded_logits(b, R, V, dtype):
    """(flat buffer, shape, strides): rows 24 elements apart from each other, batch rows a further 40; NaNs with payloads, both
    infinities and -0.0 sprinkled over rows and gaps.  Built once per shape, cloned per call."""
    key = (b, R, V, dtype)
    if key not in _base:
        sr_, sb = V + 24, R * (V + 24) + 40
        g = torch.Generator().manual_seed(V + R)
        flat = (torch.randn(GUARD + b * sb + GUARD, generator=g) * 4).to(dtype)
        bits = flat.view(torch.int16)
        spots = torch.randint(0, flat.numel(), (flat.numel() // 7,), generator=g)
        nan = 0x7e01 if dtype == torch.float16 else 0x7fc1
        for k, pattern in enumerate((nan, nan + 0x21, -0x8000, 0x7c00 if dtype == torch.float16 else 0x7f80, -(0x8000 - nan))):
            bits[spots[k::5]] = pattern                                   # (the last: a NaN with the sign bit set)
        _base[key] = (flat, (b, R, V), (sb, sr_, 1))
    return _base[key]


def alphabet(V):
    return [0, 1, 5, 17, V // 2, V - 1, V, -1]                            # two of the eight are outside the vocabulary


def tree(R, b, V, g):
    """(extra_ids [b, C], extra_mask [b, R, C]) of a level-major tree of B branches (node = 1 + (d - 1) * B + j): 69 rows = 4
    branches of depth 17, 5 rows = the chain of depth 4, 1 row = no extras."""
    if R == 1:
        return None, None, 1, 0
    B = 4 if R == 69 else 1                                               # (129 rows: the chain of depth 128, the longest path)
    gamma = (R - 1) // B
    C = R - 1
    al = torch.tensor(alphabet(V))
    ids = al[torch.randint(0, 8, (b, C), generator=g)]
    mask = torch.zeros((b, R, C), dtype=torch.int64)
    for j in range(B):
        for d in range(1, gamma + 1):
            for dd in range(1, d + 1):
                mask[:, 1 + (d - 1) * B + j, (dd - 1) * B + j] = 1 + dd     # (any non-zero value selects)
    return ids, mask, B, gamma


def make_case(b, R, V, n, ws, seed):
    """Texts and trees with planted matches: every text ends in a period-3 stretch of ids inside the vocabulary, branch 0 goes
    on with it, branch 1 is one id repeated, the others are random over the alphabet."""
    g = torch.Generator().manual_seed(seed)
    W = 2 * bo_chunk() + 8
    al = torch.tensor(alphabet(V))
    out = al[torch.randint(0, 8, (b, W), generator=g)]
    pat = [5, V - 1, 0]
    ids, mask, B, gamma = tree(R, b, V, g)
    for z, w in enumerate(ws):
        for i in range(max(0, w - 40), w):
            out[z, i] = pat[i % 3]
        out[z, w:] = 17                                                   # behind w: never read (a constant would match if it were)
        if ids is not None:
            for d in range(1, gamma + 1):
                ids[z, (d - 1) * B] = pat[(w + d - 1) % 3]
                if B > 1:
                    ids[z, (d - 1) * B + 1] = 1
    return out, ids, mask


def bo_chunk():
    from longspec_amd import ops as _ops
    return _ops.BAN_CHUNK


def categories(texts, ws, n, V):
    """Which kinds of no-repeat match the rows of a case hold (with an id inside the vocabulary, so that a store happens)."""
    CH, seen = bo_chunk(), set()
    for z, rows in enumerate(texts):
        w = ws[z]
        for t in rows:
            m = len(t)
            if n < 2 or m < n:
                continue
            tail = t[m - n + 1:]
            for j in range(n - 1, m):
                if t[j - 1] != tail[-1] or t[j - n + 1:j] != tail or not (0 <= t[j] < V):
                    continue
                lo = j - n + 1
                if j < w:
                    seen.add("text")
                    if lo // CH != j // CH:
                        seen.add("chunk-edge")
                    if 0 < m - w < n - 1:
                        seen.add("tail-straddles")
                elif lo >= w:
                    seen.add("path")
                else:
                    seen.add("text/path")
    return seen


def check(ops, b, R, V, dtype, table, out, base, base_sub, base_add, ids, mask):
    flat, shape, strides = guarded_logits(b, R, V, dtype)
    flat_c = flat.clone()
    before = flat_c.clone()
    flat_d = flat_c.to(DEV)
    x_c, x_d = flat_c.as_strided(shape, strides, GUARD), flat_d.as_strided(shape, strides, GUARD)
    if R == 1 and ids is None:
        x_c, x_d = x_c[:, 0], x_d[:, 0]                                   # the two-dimensional form
    i32 = lambda t, dv: None if t is None else torch.tensor(t, dtype=torch.int32, device=dv)
    dv = lambda t: None if t is None else t.to(DEV)
    bo.ban_rows(x_c, table, out, base=i32(base, "cpu"), base_sub=i32(base_sub, "cpu"), base_add=base_add, extra_ids=ids, extra_mask=mask)
    got = ops.ban_rows(x_d, table.to(DEV), dv(out), base=i32(base, DEV), base_sub=i32(base_sub, DEV), base_add=base_add,
                       extra_ids=dv(ids), extra_mask=dv(mask))
    assert got is x_d
    torch.cuda.synchronize()
    assert torch.equal(flat_c.view(torch.int16), flat_d.cpu().view(torch.int16))
    changed = flat_c.view(torch.int16) != before.view(torch.int16)
    ninf = -0x0400 if dtype == torch.float16 else -0x0080
    assert (flat_c.view(torch.int16)[changed] == ninf).all()
    return int(changed.sum())


def sequences_for(k, texts, V):
    """0, 1 or 64 sequences of 1, 2 and 16 tokens; those of 2 and 16 are the ends of rows' texts plus one id, so they match."""
    if k == 0:
        return []
    flat = [t for rows in texts for t in rows]
    ok = lambda t, L: len(t) >= L - 1 and all(0 <= v < 2 ** 31 for v in t[len(t) - L + 1:])
    seqs = []
    for L, quota in ((16, 20), (2, 24), (1, 20)):
        fit = [(i, t) for i, t in enumerate(flat) if ok(t, L)]
        for i, t in fit[::max(len(fit) // quota, 1)][:quota]:             # spread over the rows
            seqs.append(t[len(t) - L + 1:] + [(7 * i + L) % V if i % 5 else V + i])
    while len(seqs) < 64:
        seqs.append([len(seqs) % V])
    return seqs[:1] if k == 1 else seqs[:64]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("V", [1023, 128256])
@pytest.mark.parametrize("R", [1, 5, 69])
def test_the_whole_buffer_is_the_oracles_bit_for_bit(ops, R, V, dtype):
    CH = ops.BAN_CHUNK
    seen, stores = set(), 0
    for k, n in enumerate(NS):
        widths = sorted({0, 1, max(n - 2, 0), max(n - 1, 0), n, CH - 1, CH, CH + 1, 2 * CH + 3})
        groups = [widths[i:i + 3] for i in range(0, len(widths), 3)]
        groups[-1] = (groups[-1] + widths)[:3]
        for gi, ws in enumerate(groups):                                  # batch 3: three widths a call
            out, ids, mask = make_case(3, R, V, n, ws, seed=100 * k + gi)
            texts = bo.row_texts(3, R, out, base=torch.tensor(ws), extra_ids=ids, extra_mask=mask)
            seqs = sequences_for((0, 1, 64)[(k + gi) % 3], texts, V)
            table = Ban(seqs, n).table(V, "cpu")
            # base / base_sub / base_add as the loops pass them: w = base - base_sub + base_add
            stores += check(ops, 3, R, V, dtype, table, out, [w + 1000 for w in ws], [1001] * 3, 1, ids,
                            mask if mask is None or gi % 2 else mask[0])  # the tree is one for the batch: [R, C] or [b, R, C]
            seen |= categories(texts, ws, n, V)
        # batch 1, the width just past a chunk edge, sequences only half of the time
        out, ids, mask = make_case(1, R, V, n, [CH + 1], seed=7 * k)
        stores += check(ops, 1, R, V, dtype, Ban([[5, V - 1, 0]] if k % 2 else [], n).table(V, "cpu"), out, [CH + 1], None, 0, ids, mask)
    want = {"text", "chunk-edge"} | ({"path", "text/path", "tail-straddles"} if R > 1 else set())
    print(f"R={R} V={V}: {stores} stores; matches seen: {sorted(seen)}")
    assert want <= seen, sorted(want - seen)
    assert stores > 100 * R


def test_the_longest_path_of_128_columns(ops):
    """C = LS_BAN_MAX_EXTRA: the path is assembled, counted and placed over two full steps of 64 mask columns."""
    V, R = 1023, 129
    assert R - 1 == ops.BAN_MAX_EXTRA
    CH, seen, stores = ops.BAN_CHUNK, set(), 0
    for n, ws in ((16, [0, 7, 2 * CH + 3]), (2, [1, CH, CH + 1]), (4, [3, 100, CH - 1])):
        out, ids, mask = make_case(3, R, V, n, ws, seed=n)
        texts = bo.row_texts(3, R, out, base=torch.tensor(ws), extra_ids=ids, extra_mask=mask)
        assert max(len(t) - w for rows, w in zip(texts, ws) for t in rows) == 128
        table = Ban(sequences_for(64, texts, V), n).table(V, "cpu")
        stores += check(ops, 3, R, V, torch.bfloat16 if n == 2 else torch.float16, table, out, ws, None, 0, ids, mask if n == 4 else mask[0])
        seen |= categories(texts, ws, n, V)
    assert {"text", "chunk-edge", "path", "text/path", "tail-straddles"} <= seen and stores > 100 * R


def test_sequences_alone_and_a_hand_made_table_with_minus_one(ops):
    V, R = 1023, 5
    out, ids, mask = make_case(3, R, V, 0, [0, 3, 40], seed=3)
    out[1, :3] = torch.tensor([-1, V, 5])
    out[2, 30:40] = torch.tensor([-1, 7, -1, 7, -1, 7, -1, 7, -1, 7])
    ids[2, :] = torch.tensor([-1, 7, -1, V + 3])
    table = Ban([[7, 2], [V, 5, 9], [7, 7, 11], [3], [2 ** 31 - 1], [7, 7, 7, V + 3, 12]], 0).table(V, "cpu")
    # by hand: sequence 0 becomes (-1, 2) -- a -1 in the table matches a -1 of the text --, sequence 2 ends in -1: never written
    t = table.clone()
    assert t[ban_mod.TOKS_OFF:ban_mod.TOKS_OFF + 2].tolist() == [7, 2] and int(t[ban_mod.TOKS_OFF + 7]) == 11
    t[ban_mod.TOKS_OFF], t[ban_mod.TOKS_OFF + 7] = -1, -1
    for dtype in (torch.float16, torch.bfloat16):
        for tab in (table, t):
            n = check(ops, 3, R, V, dtype, tab, out, [0, 3, 40], None, 0, ids, mask)
            assert n >= 3 * R                                            # the one-token sequence in every row, at the least
    x = torch.zeros((1, R, V), dtype=torch.float16)
    bo.ban_rows(x, t, out[2:], base=torch.tensor([40], dtype=torch.int32), extra_ids=ids[2:], extra_mask=mask[2:])
    assert torch.isinf(x[0, :, 2]).tolist() == [False, True, False, True, False]    # rows whose text ends in -1


def test_nothing_is_read_behind_the_written_columns_or_in_front_of_column_0(ops):
    """The same text in a wider buffer whose other columns would match gives the same rows; base clamps to the width."""
    V, n = 1023, 4
    table = Ban(no_repeat_ngram=n).table(V, DEV)
    text = torch.tensor([[5, 6, 7, 5, 6, 7, 5, 6]], device=DEV)
    wide = torch.cat([text, torch.tensor([[7, 5, 6, 7, 9]], device=DEV)], 1)
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)
    a = ops.ban_rows(torch.zeros((1, V), dtype=torch.float16, device=DEV), table, text, base=i32(8))
    b = ops.ban_rows(torch.zeros((1, V), dtype=torch.float16, device=DEV), table, wide, base=i32(8))
    c = ops.ban_rows(torch.zeros((1, V), dtype=torch.float16, device=DEV), table, text, base=i32(500))        # clamped to 8
    d = ops.ban_rows(torch.zeros((1, V), dtype=torch.float16, device=DEV), table, text, base=i32(-3))         # clamped to 0
    e = ops.ban_rows(torch.zeros((1, V), dtype=torch.float16, device=DEV), table, None)
    assert torch.isinf(a).nonzero().tolist() == [[0, 7]] and torch.equal(a, b) and torch.equal(a, c)
    assert not torch.isinf(d).any() and not torch.isinf(e).any()


def test_argument_checks(ops):
    V = 64
    table = Ban(no_repeat_ngram=2).table(V, DEV)
    x = torch.zeros((2, 3, V), dtype=torch.float16, device=DEV)
    out = torch.zeros((2, 8), dtype=torch.int64, device=DEV)
    base = torch.zeros((2,), dtype=torch.int32, device=DEV)
    ids = torch.tensor([[3, 4], [5, 6]], device=DEV)
    mask = torch.ones((2, 3, 2), dtype=torch.int64, device=DEV)
    good = dict(logits=x, table=table, output_ids=out, base=base, extra_ids=ids, extra_mask=mask)
    assert ops.ban_rows(**good) is x
    for bad in (dict(logits=x.float()), dict(logits=x.transpose(1, 2)), dict(logits=x.cpu()), dict(logits=x.view(-1).as_strided((2, 3, V), (8, 8, 1))),
                dict(table=table[:-1]), dict(table=table.long()), dict(table=torch.zeros(341, dtype=torch.int32, device=DEV)),
                dict(output_ids=out.int()), dict(output_ids=out[:1]), dict(output_ids=out.t()), dict(output_ids=out[:1].expand(2, 8)),
                dict(base=base.long()), dict(base=base[:1]), dict(base_sub=base.long()),
                dict(extra_mask=None), dict(extra_ids=None), dict(extra_ids=ids.int()), dict(extra_ids=ids[:1]),
                dict(extra_mask=mask.int()), dict(extra_mask=mask[:, :2]), dict(extra_mask=mask[:1]), dict(extra_mask=mask[:, :, :1]),
                dict(extra_ids=torch.zeros((2, ops.BAN_MAX_EXTRA + 1), dtype=torch.int64, device=DEV),
                     extra_mask=torch.zeros((3, ops.BAN_MAX_EXTRA + 1), dtype=torch.int64, device=DEV))):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises((TypeError, ValueError, RuntimeError)):
            ops.ban_rows(**kw)
    assert not torch.isinf(x).any()                                       # (no text and paths without a repeat: nothing was banned)
    assert ops.BAN_TABLE_WORDS == ban_mod.TABLE_WORDS and ops.BAN_CHUNK >= 64
