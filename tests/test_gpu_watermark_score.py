"""``ops.watermark_score`` (``ls_watermark_score``) and ``Watermark.detect`` on the device against the CPU path of
longspec_amd/watermark.py (which tests/test_watermark_oracle.py holds to the plain-Python oracle): n = 0, h, h + 1, 1 023 /
1 024 / 1 025 and 131 072, batch 1 and 3 with a row stride, ``lengths`` below and above n, planted repeated n-grams with
``unique``, ids outside the vocabulary, counts that held garbage, and a replay from a graph."""
import math

import pytest
import torch

import watermark_oracle as wo
from longspec_amd import Watermark

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEY = 0x0123456789ABCDEF


@pytest.fixture(scope="module")
def ops():
    from longspec_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def texts(b, n, vocab, seed, stride):
    """int64 [b, n] with rows ``n + stride`` apart: random ids, repeated n-grams planted, two ids outside the vocabulary."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randint(0, vocab, (b, n + stride), generator=g)
    if n >= 64:
        buf[:, n - 24:n] = buf[:, 8:32]
        buf[:, 40:52] = buf[:, 8:20]
        buf[0, 3], buf[b - 1, 33] = -7, 2 ** 45
    return buf[:, :n]


def dev(x):
    """``x`` on the device with the strides it has here."""
    d = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=DEV)
    d.copy_(x)
    return d


def same(got, want):
    assert got.scored.tolist() == want.scored.tolist() and got.green.tolist() == want.green.tolist()
    assert torch.equal(got.flags.cpu(), want.flags)
    for a, b in zip(got.z.tolist(), want.z.tolist()):                    # from equal integers: a few float64 roundings apart
        assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 8 * 2.0 ** -52 * max(1.0, abs(b))
    assert got.scored.is_cuda and got.z.dtype == torch.float64 and got.flags.dtype == torch.int8 and got.scored.dtype == torch.int32


@pytest.mark.parametrize("h", [1, 3, 8])
def test_detect_on_the_device_is_detect_on_the_cpu(ops, h):
    wm = Watermark(KEY + h, 0.25, 2.0, context=h)
    for n in (0, h, h + 1, 1023, 1024, 1025):
        for b, stride in ((1, 0), (3, 5)):
            x = texts(b, n, 50000, 100 * n + b, stride)
            assert b == 1 or n == 0 or not x.is_contiguous()
            lens = [max(n - 9, 0), n + 4, n // 2][:b]
            for lengths in (None, lens):
                for unique in (False, True):
                    same(wm.detect(dev(x), lengths=lengths, unique=unique), wm.detect(x, lengths=lengths, unique=unique))
            if n >= 1023 and h <= 3:
                assert (wm.detect(dev(x), unique=True).scored < wm.detect(dev(x)).scored).all()


def test_the_operator_overwrites_its_counts_and_returns_the_hashes(ops, monkeypatch):
    wm = Watermark(KEY, 0.5, 2.0, context=2)
    x = texts(3, 1025, 128256, 5, 7)
    real = torch.empty

    def garbage(*a, **kw):                                                # the operator's outputs start as garbage
        t = real(*a, **kw)
        t.view(torch.uint8).fill_(0x5a)
        return t

    monkeypatch.setattr(torch, "empty", garbage)
    lens = torch.tensor([1025, 1000, 0], dtype=torch.int32, device=DEV)
    got = ops.watermark_score(dev(x), wm.table(0, DEV), lens, want_flags=True, want_hashes=True)
    bare = ops.watermark_score(dev(x), wm.table(0, DEV), lens, want_flags=False)
    monkeypatch.undo()
    assert bare.flags is None and bare.hashes is None and torch.equal(bare.counts, got.counts)
    want = wm.detect(x, lengths=lens.cpu())
    assert got.counts.dtype == torch.int32 and got.counts.cpu().tolist() == [[int(s), int(g)] for s, g in zip(want.scored, want.green)]
    assert got.counts[2].tolist() == [0, 0] and torch.equal(got.flags.cpu(), want.flags)
    hashes = got.hashes.cpu().view(torch.int64)
    for z in range(3):
        row = x[z].tolist()
        for c in (0, 1, 2, 3, 33, 500, 999, 1000, 1024):
            u = wo.u_of(wo.state(wm.key, row[c - 2:c]), row[c]) if 2 <= c < int(lens[z]) else 0
            assert int(hashes[z, c]) & wo.MASK == u, (z, c)


def test_a_document_of_131072_tokens_is_one_launch(ops):
    wm = Watermark(KEY, 0.25, 2.0, context=4)
    n = 131072
    x = texts(1, n, 128256, 9, 0)
    marked = x.clone()                                                    # every 97th token replaced by a green one
    for c in range(4, n, 97):
        s = wo.state(wm.key, marked[0, c - 4:c].tolist())
        marked[0, c] = next(v for v in range(1000) if wo.is_green(s, v, wm.threshold))
    for ids in (x, marked):
        d = ids.to(DEV)
        same(wm.detect(d), wm.detect(ids))
        same(wm.detect(d, unique=True), wm.detect(ids, unique=True))
    z_plain, z_marked = float(wm.detect(x.to(DEV)).z[0]), float(wm.detect(marked.to(DEV)).z[0])
    print(f"z of the random document {z_plain:.2f}, with 1 351 green tokens planted {z_marked:.2f}")
    assert abs(z_plain) < 5 and z_marked > z_plain + 3
    # replayed from a graph: the counts are cleared inside the capture, never accumulated
    table, d = wm.table(0, DEV), x.to(DEV)
    want = wm.detect(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.watermark_score(d, table)
    torch.cuda.current_stream().wait_stream(side)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=side):
        got = ops.watermark_score(d, table)
    for _ in range(3):
        gr.replay()
        torch.cuda.synchronize()
        assert got.counts.cpu().tolist() == [[int(want.scored[0]), int(want.green[0])]]


def test_argument_checks(ops):
    table = Watermark(1).table(0, DEV)
    x = torch.zeros((2, 16), dtype=torch.int64, device=DEV)
    lens = torch.zeros((2,), dtype=torch.int32, device=DEV)
    assert ops.watermark_score(x, table, lens).counts.tolist() == [[0, 0], [0, 0]]
    for bad in (dict(ids=x.int()), dict(ids=x.cpu()), dict(ids=x.t()), dict(ids=x[None]), dict(table=table[:-1]), dict(table=table.long()),
                dict(lengths=lens.long()), dict(lengths=lens[:1]), dict(lengths=lens.cpu())):
        kw = dict(ids=x, table=table, lengths=lens)
        kw.update(bad)
        with pytest.raises((TypeError, ValueError, RuntimeError)):
            ops.watermark_score(**kw)
