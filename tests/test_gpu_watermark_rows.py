"""``ops.watermark_rows`` (``ls_watermark_rows``) against the oracle (tests/watermark_oracle.py), the whole buffer bit for bit --
the gaps between strided rows and the guards around the buffer included: fp16 and bf16, 1 / 5 / 33 / 69 rows, V = 1 000 and
70 001 (odd, and with the row stride V + 24 every row starts at another offset from a 16-byte boundary: the element-wise head and
tail), batch 1 and 3, contexts of 1 / 2 / 4 / 8 tokens, text widths 0 / h-1 / h / h+1 and one beyond 1024, random tree masks
of 79 columns and chain masks of 100, paths shorter than, as long as and longer than the context, ids outside the vocabulary,
both infinities / NaNs / -0.0 / a subnormal in the rows.  A second call adds delta again, and one launch replays from a graph."""
import math

import pytest
import torch

import test_gpu_dry_rows as gd
import watermark_oracle as wo
from ban_oracle import row_texts
from longspec_amd import Watermark

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = gd.GUARD
KEY = 0x0123456789ABCDEF
base_logits, masks = gd.base_logits, gd.masks                            # the buffer and mask recipes of the dry test


@pytest.fixture(scope="module")
def ops():
    from longspec_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert _ops.WATERMARK_MAX_CONTEXT == 8
    return _ops


def make_case(b, R, V, ws, kind, seed):
    """Texts and extras over five ids, two of them outside the vocabulary: few distinct contexts, so that the oracle's green
    lists are shared between rows."""
    g = torch.Generator().manual_seed(seed)
    al = torch.tensor([3, 7, V - 1, V, -1])
    W = max(max(ws), 1) + 3
    out = al[torch.randint(0, 5, (b, W), generator=g)]
    C, mask = masks(kind, b, R, g)
    ids = al[torch.randint(0, 5, (b, C), generator=g)] if C else None
    return out, ids, mask


def check(ops, b, R, V, dtype, wm, out, ws, ids, mask, strided=False, twice=False, graph=False):
    """One call against the oracle; returns (changed elements, the texts)."""
    flat, shape, strides = base_logits(b, R, V, dtype, strided)
    flat_c = flat.clone()
    flat_d = flat.to(DEV)
    x_c, x_d = flat_c.as_strided(shape, strides, GUARD), flat_d.as_strided(shape, strides, GUARD)
    if R == 1 and ids is None:
        x_c, x_d = x_c[:, 0], x_d[:, 0]                                   # the two-dimensional form
    i32 = lambda t, dv: torch.tensor(t, dtype=torch.int32, device=dv)
    dv = lambda t: None if t is None else t.to(DEV)
    table = wm.table(V, "cpu")
    wo.watermark_rows(x_c, table, out, base=i32(ws, "cpu"), extra_ids=ids, extra_mask=mask)
    args = (table.to(DEV), dv(out))
    kw = dict(base=i32(ws, DEV), extra_ids=dv(ids), extra_mask=dv(mask))
    got = ops.watermark_rows(x_d, *args, **kw)
    assert got is x_d
    torch.cuda.synchronize()
    want_bits = flat_c.view(torch.int16).clone()
    assert torch.equal(want_bits, flat_d.cpu().view(torch.int16))
    changed = int((want_bits != flat.view(torch.int16)).sum())
    if twice:                                                             # not idempotent: delta is added again
        wo.watermark_rows(x_c, table, out, base=i32(ws, "cpu"), extra_ids=ids, extra_mask=mask)
        ops.watermark_rows(x_d, *args, **kw)
        assert torch.equal(flat_c.view(torch.int16), flat_d.cpu().view(torch.int16))
        assert changed == 0 or not torch.equal(flat_c.view(torch.int16), want_bits)
    if graph:
        fresh = flat.to(DEV)
        flat_d.copy_(fresh)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.watermark_rows(x_d, *args, **kw)                          # (warm-up on the capture stream)
        torch.cuda.current_stream().wait_stream(side)
        flat_d.copy_(fresh)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            ops.watermark_rows(x_d, *args, **kw)
        for _ in range(2):
            flat_d.copy_(fresh)
            gr.replay()
            torch.cuda.synchronize()
            assert torch.equal(want_bits, flat_d.cpu().view(torch.int16))
    texts = row_texts(b, R, out, base=torch.tensor(ws), extra_ids=ids, extra_mask=mask)
    return changed, texts


def kinds_of(texts, ws, h):
    """Where the contexts of a case's rows come from."""
    seen = set()
    for z, rows in enumerate(texts):
        for t in rows:
            d = len(t) - ws[z]
            seen.add("unmarked" if len(t) < h else "text" if d == 0 else "seam" if d < h else "path" if d == h else "deep-path")
    return seen


# (b, h, the widths of the batch rows, strided, gamma, delta)
CASES = [(3, 1, (0, 1, 2), False, 0.25, 2.0), (3, 2, (1, 2, 3), True, 0.5, 0.37), (1, 4, (1030,), True, 0.25, 2.0),
         (3, 4, (3, 4, 5), False, 0.1, 5.5), (3, 8, (7, 8, 9), True, 0.25, 2.0), (1, 8, (0,), False, 0.9, 1.0)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("R,V,kind", [(1, 1000, None), (1, 70001, None), (5, 70001, "chain"), (33, 1000, "tree"), (69, 70001, "tree"),
                                      (69, 1000, "chain")])
def test_the_whole_buffer_is_the_oracles_bit_for_bit(ops, R, V, kind, dtype):
    seen, stores = set(), 0
    for k, (b, h, ws, strided, gamma, delta) in enumerate(CASES):
        if V > 1000 and R > 5 and h > 2:
            continue                                                      # (many rows with a context each: minutes of oracle)
        wm = Watermark(KEY + k, gamma, delta, context=h)
        out, ids, mask = make_case(b, R, V, ws, kind, seed=10 * R + k)
        n, texts = check(ops, b, R, V, dtype, wm, out, list(ws), ids, mask if mask is None or k % 2 else mask[0],
                         strided=strided, twice=(V == 1000), graph=(k == 2 and V == 1000))
        stores += n
        seen |= {(h, s) for s in kinds_of(texts, ws, h)}
    print(f"R={R} V={V} {kind}: {stores} marked elements; contexts seen: {sorted(seen)}")
    where = {s for _, s in seen}
    assert {"unmarked", "text"} <= where and stores >= V // 8
    if R > 1:
        assert "deep-path" in where
    if R >= 33:
        assert {"seam", "path"} <= where and {(2, "seam"), (2, "path"), (2, "deep-path")} <= seen
    if V == 1000 and R >= 33:
        assert {(8, "seam"), (8, "deep-path"), (8, "unmarked")} <= seen


def test_known_green_lists_overflow_to_infinity_and_special_values(ops):
    V = 64
    green = [0, 4, 11, 13, 15, 21, 22, 25, 29, 31, 33, 35, 53, 54, 58]     # after [42], gamma 0.25 (the contract's known answer)
    table = Watermark(KEY, 0.25, 1000.0).table(V, DEV)
    row = torch.zeros((1, V), dtype=torch.float16)
    row[0, 0], row[0, 4], row[0, 11], row[0, 13], row[0, 1] = 65000.0, float("nan"), -math.inf, -0.0, 65000.0
    out = torch.tensor([[9, 42, 3]], device=DEV)
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)
    same = ops.watermark_rows(row.to(DEV), table, out, base=i32(0)).cpu()                    # no token: fewer than h
    assert torch.equal(same.view(torch.int16), row.view(torch.int16))
    got = ops.watermark_rows(row.to(DEV), table, out, base=i32(2)).cpu()
    assert got[0, 0] == math.inf and got[0, 1] == row[0, 1]               # 65 000 + 1 000 rounds to +inf; a red id keeps its bits
    assert int(got.view(torch.int16)[0, 4]) == int(row.view(torch.int16)[0, 4]) and got[0, 11] == -math.inf and float(got[0, 13]) == 1000.0
    assert [v for v in range(V) if float(got[0, v]) == 1000.0] == green[3:]
    want = wo.watermark_rows(row.clone(), table.cpu(), out.cpu(), base=i32(2).cpu())
    assert torch.equal(want.view(torch.int16), got.view(torch.int16))
    two = Watermark(KEY, 0.25, 2.0, context=2).table(V, DEV)               # after [7, 42]: from the path alone, then across the seam
    ids, mask = torch.tensor([[7, 42]], device=DEV), torch.tensor([[0, 0], [1, 0], [1, 1]], device=DEV)
    rows = ops.watermark_rows(torch.zeros((1, 3, V), dtype=torch.bfloat16, device=DEV), two, out, base=i32(1), extra_ids=ids, extra_mask=mask).cpu()
    assert not rows[0, 0].any() and rows[0, 1].nonzero().flatten().tolist() == wo.green_ids(KEY, [9, 7], 0.25, V)
    assert rows[0, 2].nonzero().flatten().tolist() == [0, 2, 3, 4, 5, 6, 9, 28, 33, 41, 45, 51, 60, 62]


def test_base_clamps_and_nothing_is_read_behind_the_written_columns(ops):
    V = 1000
    table = Watermark(7, 0.25, 2.0, context=2).table(V, DEV)
    text = torch.tensor([[5, 6, 7, 5, 6, 7, 5, 6]], device=DEV)
    wide = torch.cat([text, torch.tensor([[7, 5, 6, 7, 9]], device=DEV)], 1)
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)
    row = lambda: torch.zeros((1, V), dtype=torch.float16, device=DEV)
    a = ops.watermark_rows(row(), table, text, base=i32(8))
    b = ops.watermark_rows(row(), table, wide, base=i32(8))
    c = ops.watermark_rows(row(), table, text, base=i32(500))             # clamped to 8
    d = ops.watermark_rows(row(), table, text, base=i32(-3))              # clamped to 0
    e = ops.watermark_rows(row(), table, None)
    f = ops.watermark_rows(row(), table, wide, base=i32(1008), base_sub=i32(1001), base_add=1)
    assert a.nonzero()[:, 1].tolist() == [v for v in range(V) if wo.is_green(wo.state(7, [5, 6]), v, 2 ** 30)]
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, f) and not d.any() and not e.any()


def test_argument_checks(ops):
    V = 64
    table = Watermark(1).table(V, DEV)
    x = torch.zeros((2, 3, V), dtype=torch.float16, device=DEV)
    out = torch.zeros((2, 8), dtype=torch.int64, device=DEV)
    base = torch.zeros((2,), dtype=torch.int32, device=DEV)
    ids = torch.tensor([[3, 4], [5, 6]], device=DEV)
    mask = torch.ones((2, 3, 2), dtype=torch.int64, device=DEV)
    good = dict(logits=x, table=table, output_ids=out, base=base, extra_ids=ids, extra_mask=mask)
    assert ops.watermark_rows(**good) is x
    x.zero_()
    for bad in (dict(logits=x.float()), dict(logits=x.transpose(1, 2)), dict(logits=x.cpu()),
                dict(table=table[:-1]), dict(table=table.long()), dict(table=torch.zeros(101, dtype=torch.int32, device=DEV)),
                dict(output_ids=out.int()), dict(output_ids=out[:1]), dict(output_ids=out.t()),
                dict(base=base.long()), dict(base=base[:1]), dict(base_sub=base.long()),
                dict(extra_mask=None), dict(extra_ids=None), dict(extra_ids=ids.int()), dict(extra_mask=mask[:, :2]),
                dict(extra_ids=torch.zeros((2, ops.BAN_MAX_EXTRA + 1), dtype=torch.int64, device=DEV),
                     extra_mask=torch.zeros((3, ops.BAN_MAX_EXTRA + 1), dtype=torch.int64, device=DEV))):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises((TypeError, ValueError, RuntimeError)):
            ops.watermark_rows(**kw)
    assert not x.any()
