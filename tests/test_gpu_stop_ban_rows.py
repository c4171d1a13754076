"""``ops.stop_ban_rows`` (``ls_stop_ban_rows``) against the oracle (tests/stop_oracle.py), exact: V = 1023 and 128 256, 1 / 5 / 69
rows with a non-contiguous row stride, fp16 and bf16, the depth of a row from a tree mask grown by the tree operators (shape
4/16/16/16/16), from the row index (chain) and none (the single row).  Every banned element is -inf, every other element of the
buffer -- the gaps between the rows and the guards around it included -- keeps its bits, and rows at or past ``min_tokens`` are
untouched."""
import pytest
import torch

import stop_oracle as so
from longspec_amd import Stop
from test_gpu_tree import grow_both

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 16


@pytest.fixture(scope="module")
def ops():
    from longspec_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def guarded_logits(b, R, V, dtype, seed):
    """(flat buffer, the [b, R, V] view into it): rows 24 elements apart from each other, batch rows a further 40."""
    sr_, sb = V + 24, R * (V + 24) + 40
    g = torch.Generator().manual_seed(seed)
    flat = (torch.randn(GUARD + b * sb + GUARD, generator=g) * 4).to(dtype)
    return flat, flat.as_strided((b, R, V), (sb, sr_, 1), GUARD)


def check(ops, b, R, V, dtype, stop, seed, depth=None, tree_mask=None, base=None, base_sub=None, base_add=0):
    flat_c, x_c = guarded_logits(b, R, V, dtype, seed)
    flat_d = flat_c.to(DEV)
    x_d = flat_d.as_strided(x_c.shape, x_c.stride(), GUARD)
    before = flat_c.clone()
    i32 = lambda t, dv: None if t is None else torch.tensor(t, dtype=torch.int32, device=dv)
    so.stop_ban_rows(x_c, stop.table(V, "cpu"), base=i32(base, "cpu"), base_sub=i32(base_sub, "cpu"), base_add=base_add, depth=depth,
                     tree_mask=tree_mask)
    got = ops.stop_ban_rows(x_d, stop.table(V, DEV), base=i32(base, DEV), base_sub=i32(base_sub, DEV), base_add=base_add, depth=depth,
                            tree_mask=None if tree_mask is None else tree_mask.to(DEV))
    assert got is x_d
    assert torch.equal(flat_c.view(torch.int16), flat_d.cpu().view(torch.int16))
    changed = flat_c.view(torch.int16) != before.view(torch.int16)
    assert torch.isinf(flat_c[changed].float()).all() and (flat_c[changed].float() < 0).all()
    return x_c, int(changed.sum())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("V", [1023, 128256])
def test_depth_from_a_grown_tree_mask(ops, V, dtype):
    (tree_mask, _, _), _, acc_n = grow_both(ops, [4, 16, 16, 16, 16], 2, min(V, 5000), seed=5)
    Fn = acc_n[-1]
    assert Fn == 69
    depth = tree_mask[:, :, 1:].sum(-1)
    assert depth[:, 0].tolist() == [0, 0] and int(depth.max()) == 5
    ids = [0, V - 1, 17, V // 2] + list(range(100, 160))
    stop = Stop(token_ids=ids, sequences=[[1, 2]], min_tokens=9)
    base = [6, 3]                                                  # row j predicts column base + depth(j); banned while < 9
    x, n = check(ops, 2, Fn, V, dtype, stop, seed=V % 97, depth="tree", tree_mask=tree_mask, base=base)
    want = (torch.tensor(base)[:, None] + depth) < 9
    assert want.any() and not want.all()
    for z in range(2):
        for r in range(Fn):
            assert bool(torch.isinf(x[z, r, ids].float()).all()) == bool(want[z, r]), (z, r)
    assert n == int(want.sum()) * len(ids)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("V", [1023, 128256])
@pytest.mark.parametrize("R", [1, 5, 69])
def test_depth_from_the_row_index_and_none(ops, R, V, dtype):
    stop = Stop(token_ids=[V - 1, 0, 5], min_tokens=4)
    # the chain form: row i predicts column cache_lens - input_len + 1 + i
    x, n = check(ops, 3, R, V, dtype, stop, seed=R, depth="row", base=[1001, 1002, 1007], base_sub=[1000, 1000, 1000], base_add=1)
    for z, first in enumerate([2, 3, 8]):
        for r in range(R):
            assert bool(torch.isinf(x[z, r, [V - 1, 0, 5]].float()).all()) == (first + r < 4), (z, r)
    # the single-row forms: the vanilla step's row predicts column cache_lens - input_len + 1, the first token's column 0
    x, n = check(ops, 3, R, V, dtype, stop, seed=R + 1, base=[1002, 1003, 1000], base_sub=[1000, 1000, 1000], base_add=1)
    assert [bool(torch.isinf(x[z, :, 0].float()).all()) for z in range(3)] == [True, False, True]
    assert not torch.isinf(x[1].float()).any() and n == 2 * R * 3
    x, n = check(ops, 3, R, V, dtype, stop, seed=R + 2)
    assert torch.isinf(x[:, :, [V - 1, 0, 5]].float()).all()


def test_nothing_changes_without_min_tokens_or_past_it(ops):
    for stop, base in ((Stop(token_ids=[3, 4]), [0]), (Stop(token_ids=[3, 4], min_tokens=5), [5]),
                       (Stop(sequences=[[3, 4]], min_tokens=5), [0])):
        x, n = check(ops, 1, 5, 1023, torch.float16, stop, seed=3, depth="row", base=base)
        assert n == 0


def test_two_dimensional_logits_and_argument_checks(ops):
    stop = Stop(token_ids=[3], min_tokens=1)
    x = torch.zeros((2, 64), dtype=torch.float16, device=DEV)
    assert ops.stop_ban_rows(x, stop.table(64, DEV)) is x
    assert x[:, 3].tolist() == [float("-inf")] * 2 and int(torch.isinf(x).sum()) == 2
    table = stop.table(64, DEV)
    base = torch.zeros((2,), dtype=torch.int32, device=DEV)
    for bad in (dict(logits=x.float()), dict(logits=x.t()), dict(table=table[:-1]), dict(base=base.long()), dict(depth="tree"),
                dict(depth="rows"), dict(logits=x.cpu()),
                dict(depth="tree", tree_mask=torch.zeros((2, 2, 3), dtype=torch.int64, device=DEV))):
        kw = dict(logits=x, table=table)
        kw.update(bad)
        with pytest.raises((TypeError, ValueError, RuntimeError)):
            ops.stop_ban_rows(**kw)
