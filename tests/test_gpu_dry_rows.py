"""``ops.dry_rows`` (``ls_dry_rows``) against the oracle (tests/dry_oracle.py), the whole buffer bit for bit -- the gaps between
strided rows and the guards around the buffer included: fp16 and bf16, 1 / 5 / 33 / 69 rows, V = 1 000 and 70 001, text widths
around MAX_MATCH and around the scan's chunk edges with repeats planted across each edge, alphabets of 2-3 ids so that many
positions compete for one cell of the scratch, random tree masks of 79 columns and chain masks of 100, breakers, ``last_n``,
ids outside the vocabulary, -inf / NaN / -0.0 in the rows.  Behind every call the scratch is all zero, a second call on it
returns the same bits, and the two launches replay from a graph."""
import pytest
import torch

import dry_oracle as do
from ban_oracle import row_texts
from longspec_amd import Dry

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 16
CH = 1024                                                                # LS_BAN_CHUNK (asserted below)


@pytest.fixture(scope="module")
def ops():
    from longspec_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert _ops.BAN_CHUNK == CH and _ops.DRY_MAX_MATCH == 32
    return _ops


_base = {}


def base_logits(b, R, V, dtype, strided):
    """(flat buffer, shape, strides): contiguous, or rows 24 elements apart and batch rows a further 40; both infinities, NaNs
    with payloads and -0.0 sprinkled over rows and gaps.  Built once per shape, cloned per call."""
    key = (b, R, V, dtype, strided)
    if key not in _base:
        sr_ = V + 24 if strided else V
        sb = R * sr_ + (40 if strided else 0)
        g = torch.Generator().manual_seed(V + R)
        flat = (torch.randn(GUARD + b * sb + GUARD, generator=g) * 6).to(dtype)
        bits = flat.view(torch.int16)
        spots = torch.randint(0, flat.numel(), (flat.numel() // 5,), generator=g)
        nan = 0x7e01 if dtype == torch.float16 else 0x7fc1
        ninf = -0x0400 if dtype == torch.float16 else -0x0080
        for k, pattern in enumerate((ninf, nan, -0x8000, 0x7c00 if dtype == torch.float16 else 0x7f80, ninf, 0x0001)):
            bits[spots[k::6]] = pattern                                   # (0x0001: the smallest subnormal)
        _base[key] = (flat, (b, R, V), (sb, sr_, 1))
    return _base[key]


def masks(kind, b, R, g):
    """(C, extra_mask [b, R, C]): ``tree``: 79 columns, every row a random increasing subset of up to 24 of them (row 0: none);
    ``chain``: 100 columns, row r follows the first r * 100 // (R - 1) -- the last row all 100, two ballot rounds."""
    if kind is None or R == 1:
        return 0, None
    C = 79 if kind == "tree" else 100
    mask = torch.zeros((b, R, C), dtype=torch.int64)
    for z in range(b):
        for r in range(1, R):
            if kind == "tree":
                n = int(torch.randint(1, 25, (1,), generator=g))
                mask[z, r, torch.randperm(C, generator=g)[:n]] = 1 + r     # (any non-zero value selects)
            else:
                mask[z, r, :r * C // (R - 1)] = -1
    return C, mask


def make_case(b, R, V, ws, alphabet, kind, seed):
    """Texts over ``alphabet`` with a 40-token stretch -- the end of the text -- planted across every chunk edge the text has,
    so that positions on both sides of an edge match to depth 32 through it; extras over the same alphabet."""
    g = torch.Generator().manual_seed(seed)
    al = torch.tensor(alphabet)
    W = max(max(ws), 1) + 3
    out = al[torch.randint(0, len(alphabet), (b, W), generator=g)]
    for z, w in enumerate(ws):
        out[z, w:] = alphabet[0]                                          # behind w: never read (it would match if it were)
        for edge in (CH, 2 * CH):
            if w >= edge + 20 + 41:
                out[z, edge - 20:edge + 20] = out[z, w - 40:w]
    C, mask = masks(kind, b, R, g)
    ids = al[torch.randint(0, len(alphabet), (b, C), generator=g)] if C else None
    d1 = C // (R - 1) if kind == "chain" else 0                           # the depth of a chain's row 1
    for z, w in enumerate(ws):
        if d1 >= 3 and w >= 3:
            ids[z, d1 - 3:d1] = out[z, w - 3:w]                           # its path ends as the text does: the seam j = w - 1 matches
    return out, ids, mask


def categories(texts, ws, p, V):
    """Which kinds of penalised match the rows of a case hold (every fourth row and the last one are looked at)."""
    seen = set()
    for z, rows in enumerate(texts):
        w = ws[z]
        for t in (rows[::4] + rows[-1:] if len(rows) > 8 else rows):
            lo = max(0, len(t) - p.last_n) if p.last_n else 0
            for j, L in do.matches(t, p.last_n, p.breakers):
                if L < p.allowed_length or not (0 <= t[j + 1] < V):
                    continue
                seen.add("text" if j < w - 1 else "seam" if j == w - 1 else "path")
                if j < w - 1 and (j - L + 1) // CH != j // CH:
                    seen.add("chunk-edge")
                if L == 32:
                    seen.add("saturated")
                if j - L + 1 == lo and lo > 0:
                    seen.add("cut-by-last_n")
    return seen


def check(ops, b, R, V, dtype, dry, out, ws, ids, mask, strided=False, base=None, base_sub=None, base_add=0, graph=False):
    """One call against the oracle; returns (changed elements, the texts)."""
    flat, shape, strides = base_logits(b, R, V, dtype, strided)
    flat_c = flat.clone()
    before = flat_c.clone()
    flat_d = flat.to(DEV)
    x_c, x_d = flat_c.as_strided(shape, strides, GUARD), flat_d.as_strided(shape, strides, GUARD)
    if R == 1 and ids is None:
        x_c, x_d = x_c[:, 0], x_d[:, 0]                                   # the two-dimensional form
    if base is None:
        base = ws
    i32 = lambda t, dv: None if t is None else torch.tensor(t, dtype=torch.int32, device=dv)
    dv = lambda t: None if t is None else t.to(DEV)
    table = dry.table(V, "cpu")
    do.dry_rows(x_c, table, out, base=i32(base, "cpu"), base_sub=i32(base_sub, "cpu"), base_add=base_add, extra_ids=ids, extra_mask=mask)
    scratch = torch.zeros((b * R * V,), dtype=torch.int32, device=DEV)
    args = (table.to(DEV), dv(out), scratch)
    kw = dict(base=i32(base, DEV), base_sub=i32(base_sub, DEV), base_add=base_add, extra_ids=dv(ids), extra_mask=dv(mask))
    got = ops.dry_rows(x_d, *args, **kw)
    assert got is x_d
    torch.cuda.synchronize()
    want_bits = flat_c.view(torch.int16)
    assert torch.equal(want_bits, flat_d.cpu().view(torch.int16))
    assert int(scratch.count_nonzero()) == 0                              # the scratch cleans itself
    # a second call on the same scratch, on fresh rows: the same bits
    flat_d.copy_(flat.to(DEV))
    ops.dry_rows(x_d, *args, **kw)
    assert torch.equal(want_bits, flat_d.cpu().view(torch.int16)) and int(scratch.count_nonzero()) == 0
    if graph:
        fresh = flat.to(DEV)
        flat_d.copy_(fresh)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.dry_rows(x_d, *args, **kw)                                # (warm-up on the capture stream)
        torch.cuda.current_stream().wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            ops.dry_rows(x_d, *args, **kw)
        for _ in range(2):
            flat_d.copy_(fresh)
            gr.replay()
            torch.cuda.synchronize()
            assert torch.equal(want_bits, flat_d.cpu().view(torch.int16)) and int(scratch.count_nonzero()) == 0
    changed = want_bits != before.view(torch.int16)
    texts = row_texts(b, R, out, base=torch.tensor(ws), extra_ids=ids, extra_mask=mask)
    return int(changed.sum()), texts


WIDTHS = [(0, 1), (31, 33), (CH - 1, CH + 1), (2 * CH + 1, 2), (2 * CH + 90, CH)]       # batch 2, a different w per batch row


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("R,V,kind", [(1, 1000, None), (5, 70001, "chain"), (33, 1000, "tree"), (69, 70001, "tree"), (69, 1000, "chain")])
def test_the_whole_buffer_is_the_oracles_bit_for_bit(ops, R, V, kind, dtype):
    seen, stores = set(), 0
    for k, ws in enumerate(WIDTHS):
        alphabet = [3, V - 1] if k % 2 else [3, 7, V - 1]
        dry = Dry(0.8, 1.75, 2) if k < 2 else Dry(0.37, 1.3, 3)
        out, ids, mask = make_case(2, R, V, ws, alphabet, kind, seed=10 * R + k)
        n, texts = check(ops, 2, R, V, dtype, dry, out, list(ws), ids, mask if mask is None or k % 2 else mask[0],
                         strided=(k == 1), graph=(k == 2 and V == 1000))
        stores += n
        seen |= categories(texts, ws, do.params_of_table(dry.table(V, "cpu")), V)
    want = {"text", "chunk-edge", "saturated"} | ({"path", "seam"} if R > 1 else set())
    print(f"R={R} V={V} {kind}: {stores} penalised elements; matches seen: {sorted(seen)}")
    assert want <= seen, sorted(want - seen)
    assert stores >= 2 * R


def test_one_repeated_token_every_position_at_depth_32(ops):
    """The worst case for the maximum: every position of the text matches to the full depth and has the same candidate."""
    V, R = 1000, 5
    for dtype, w in ((torch.float16, 2 * CH + 1), (torch.bfloat16, CH)):
        out = torch.full((1, w + 2), 5, dtype=torch.int64)
        ids = torch.tensor([[5, 5, 6, 5]])
        mask = torch.ones((R, 4), dtype=torch.int64).tril(-1)
        n, texts = check(ops, 1, R, V, dtype, Dry(0.01, 1.2), out, [w], ids, mask, graph=(w == CH))
        cells = [(r, v) for r, t in enumerate(texts[0]) for v in do.match_lengths(t, 2)]
        assert cells == [(0, 5), (1, 5), (2, 5)] and 1 <= n <= 3          # row 3 ends in 6, row 4 in "6 5": depth 1 at the most


def test_breakers_last_n_and_ids_outside_the_vocabulary(ops):
    V = 1000
    al = [3, 7, V - 1, V, -1]                                              # two of the five are outside the vocabulary
    for k, (R, kind, ws, dry) in enumerate((
            (5, "chain", (CH + 1, 40), Dry(0.8, 1.75, 1, breakers=[7])),                      # a breaker in text and path
            (33, "tree", (CH + 500, 33), Dry(0.8, 1.75, 2, breakers=[7, V, 2 ** 31 - 1], last_n=500)),       # lo inside the text
            (5, "chain", (70, 2), Dry(0.8, 1.75, 1, last_n=3)),                               # lo inside the path (depth up to 100)
            (69, "chain", (CH + 70, CH - 5), Dry(0.8, 4.0, 2, last_n=CH + 30)),               # lo in chunk 0, the text in chunk 1
            (1, None, (2 * CH + 1, 7), Dry(0.5, 1.0, 32)))):                                  # only a saturated match counts
        out, ids, mask = make_case(2, R, V, ws, al if k < 2 else al[:3], kind, seed=50 + k)
        n, texts = check(ops, 2, R, V, torch.float16 if k % 2 else torch.bfloat16, dry, out, list(ws), ids, mask)
        p = do.params_of_table(dry.table(V, "cpu"))
        seen = categories(texts, ws, p, V)
        print(f"case {k}: {n} penalised elements; {sorted(seen)}")
        assert seen and (n > 0 or k == 4)                                 # (case 4 has one cell, which may hold an infinity)
        assert k != 4 or seen == {"text", "chunk-edge", "saturated"}
        if k in (2, 3):
            assert "cut-by-last_n" in seen
        if k == 0:
            # the breaker changes the result: without it the oracle penalises other elements
            x, y = torch.zeros((2, R, V), dtype=torch.float16), torch.zeros((2, R, V), dtype=torch.float16)
            kw = dict(base=torch.tensor(ws, dtype=torch.int32), extra_ids=ids, extra_mask=mask)
            do.dry_rows(x, dry.table(V, "cpu"), out, **kw)
            do.dry_rows(y, Dry(0.8, 1.75, 1).table(V, "cpu"), out, **kw)
            assert not torch.equal(x, y)


def test_nothing_is_read_behind_the_written_columns_and_base_clamps(ops):
    V = 1000
    table = Dry(1.0, 2.0).table(V, DEV)
    text = torch.tensor([[5, 6, 7, 5, 6, 7, 5, 6]], device=DEV)
    wide = torch.cat([text, torch.tensor([[7, 5, 6, 7, 9]], device=DEV)], 1)
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)
    scratch = torch.zeros((V,), dtype=torch.int32, device=DEV)
    row = lambda: torch.zeros((1, V), dtype=torch.float16, device=DEV)
    a = ops.dry_rows(row(), table, text, scratch, base=i32(8))
    b = ops.dry_rows(row(), table, wide, scratch, base=i32(8))
    c = ops.dry_rows(row(), table, text, scratch, base=i32(500))          # clamped to 8
    d = ops.dry_rows(row(), table, text, scratch, base=i32(-3))           # clamped to 0
    e = ops.dry_rows(row(), table, None, scratch)
    f = ops.dry_rows(row(), table, wide, scratch, base=i32(1008), base_sub=i32(1001), base_add=1)
    assert a.nonzero().tolist() == [[0, 7]] and float(a[0, 7]) == -8.0    # j = 4 matches "5 6 7 5 6" to depth 5: 2^(5 - 2)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, f)
    assert not d.any() and not e.any() and int(scratch.count_nonzero()) == 0


def test_argument_checks(ops):
    V = 64
    table = Dry(0.8).table(V, DEV)
    x = torch.zeros((2, 3, V), dtype=torch.float16, device=DEV)
    out = torch.zeros((2, 8), dtype=torch.int64, device=DEV)
    base = torch.zeros((2,), dtype=torch.int32, device=DEV)
    ids = torch.tensor([[3, 4], [5, 6]], device=DEV)
    mask = torch.ones((2, 3, 2), dtype=torch.int64, device=DEV)
    scratch = torch.zeros((2, 3, V), dtype=torch.int32, device=DEV)
    good = dict(logits=x, table=table, output_ids=out, scratch=scratch, base=base, extra_ids=ids, extra_mask=mask)
    assert ops.dry_rows(**good) is x
    for bad in (dict(logits=x.float()), dict(logits=x.transpose(1, 2)), dict(logits=x.cpu()),
                dict(table=table[:-1]), dict(table=table.long()), dict(table=torch.zeros(1093, dtype=torch.int32, device=DEV)),
                dict(scratch=scratch[:, :2]), dict(scratch=scratch.long()), dict(scratch=scratch.cpu()), dict(scratch=scratch[:, :, ::2]),
                dict(output_ids=out.int()), dict(output_ids=out[:1]), dict(output_ids=out.t()),
                dict(base=base.long()), dict(base=base[:1]), dict(base_sub=base.long()),
                dict(extra_mask=None), dict(extra_ids=None), dict(extra_ids=ids.int()), dict(extra_mask=mask[:, :2]),
                dict(extra_ids=torch.zeros((2, ops.BAN_MAX_EXTRA + 1), dtype=torch.int64, device=DEV),
                     extra_mask=torch.zeros((3, ops.BAN_MAX_EXTRA + 1), dtype=torch.int64, device=DEV))):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises((TypeError, ValueError, RuntimeError)):
            ops.dry_rows(**kw)
    assert not x.any() and int(scratch.count_nonzero()) == 0
