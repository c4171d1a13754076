"""tests/topk_oracle.py on the CPU: the checker accepts a correct answer and rejects each way a selection kernel goes subtly
wrong; the exact-order oracle refuses inputs on which the order is not unique."""
import pytest
import torch

from topk_oracle import check_topk, expected_topk

R, V, K = 4, 8200, 16
GRID = torch.tensor([-3.0, -1.5, -0.25, 0.5, 1.0, 2.0, 2.5, 3.0])


def _model(logits, history, k):
    """torch fp32 plus the explicit tie rule: value descending, equal values by flat index ascending."""
    lp = logits.float().log_softmax(dim=-1)
    if history is not None:
        lp = lp + history[:, None]
    flat = lp.reshape(-1)
    idx = torch.sort(flat, descending=True, stable=True).indices[:k]
    return flat[idx].clone(), idx.clone()


def _values(logits, history, idx):
    lp = logits.float().log_softmax(dim=-1) + history[:, None]
    return lp.reshape(-1)[idx].clone()


@pytest.fixture(scope="module")
def tied():
    """Row 1 wins everything: 10 columns at 6.0, then 40 columns at 5.0 of which the 6 with the smallest column belong to the
    top 16; the other rows and columns are far below."""
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(R, V, generator=g) * 0.5).half()
    hist = torch.tensor([-2.0, 0.0, -1.0, -3.0])
    big = torch.randperm(V, generator=g)[:50].sort().values
    logits[1, big[0::5]] = 6.0                 # 10 of them
    logits[1, big[torch.arange(50) % 5 != 0]] = 5.0
    vals, idx = _model(logits, hist, K)
    assert (idx // V == 1).all() and (logits[1, idx[:10] % V] == 6).all() and (logits[1, idx[10:] % V] == 5).all()
    return logits, hist, vals, idx


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("r,v,k", [(1, 512, 4), (4, 8200, 16), (16, 32000, 16), (10, 8200, 64)])
def test_check_topk_accepts_the_model_answer(r, v, k, dtype):
    g = torch.Generator().manual_seed(r + v + k)
    logits = (torch.randn(r, v, generator=g) * 2.5).to(dtype)
    hist = None if r == 1 else -torch.rand(r, generator=g) * 3
    vals, idx = _model(logits, hist, k)
    assert check_topk(vals, idx, logits, hist, k) <= 1e-5


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_check_topk_accepts_the_model_answer_on_duplicate_heavy_rows(dtype):
    g = torch.Generator().manual_seed(5)
    logits = GRID[torch.randint(0, 8, (R, V), generator=g)].to(dtype)
    hist = -torch.rand(R, generator=g) * 3
    vals, idx = _model(logits, hist, K)
    check_topk(vals, idx, logits, hist, K)
    assert torch.equal(idx, expected_topk(logits, hist, K))


def test_the_tied_fixture_is_accepted_and_exact(tied):
    logits, hist, vals, idx = tied
    check_topk(vals, idx, logits, hist, K)
    assert torch.equal(idx, expected_topk(logits, hist, K))


def _mutants(logits, hist, vals, idx):
    fives = torch.nonzero(logits[1] == 5.0).flatten() + V          # flat indices of the tied boundary value, ascending
    out = {}
    i = idx.clone()
    i[[11, 12]] = i[[12, 11]]
    out["two tied columns swapped"] = (vals.clone(), i)
    i = idx.clone()
    i[-1] = fives[6]                                                # the 7th tied column instead of the 6th
    out["a larger tied column chosen at the boundary"] = (vals.clone(), i)
    i = idx.clone()
    i[-1] = fives[-1]
    out["the largest tied column chosen at the boundary"] = (vals.clone(), i)
    nxt = torch.sort(_values(logits, hist, torch.arange(R * V)), descending=True, stable=True).indices[K]
    i = torch.cat([idx[:3], idx[4:], nxt[None]])                    # rank 3 (a 6.0) dropped, rank k + 1 appended
    out["one candidate dropped and replaced by rank k+1"] = (_values(logits, hist, i), i)
    i = idx.clone()
    i[2] += 1
    out["an index off by one column (values kept)"] = (vals.clone(), i)
    assert logits[1, (idx[2] + 1) % V] < 5
    i = torch.cat([idx[:2], idx[3:], idx[2:3] + 1])                 # ... consistently: its own value, sorted to the end
    out["an index off by one column (values of the wrong element)"] = (_values(logits, hist, i), i)
    i = idx.clone()
    i[5] += V                                                       # column right, row 2 instead of row 1
    out["the right column in the wrong row"] = (vals.clone(), i)
    v = vals.clone()
    v[[9, 10]] = v[[10, 9]]
    i = idx.clone()
    i[[9, 10]] = i[[10, 9]]
    out["values in the wrong order"] = (v, i)
    out["values ascending"] = (vals.flip(0), idx.flip(0))
    i = idx.clone()
    i[7] = i[6]
    out["a duplicate index"] = (vals.clone(), i)
    v = vals.clone()
    v[0] += 3e-5
    out["a value off by more than the bound"] = (v, idx.clone())
    return out


@pytest.mark.parametrize("name", ["two tied columns swapped", "a larger tied column chosen at the boundary",
                                  "the largest tied column chosen at the boundary", "one candidate dropped and replaced by rank k+1",
                                  "an index off by one column (values kept)", "an index off by one column (values of the wrong element)",
                                  "the right column in the wrong row", "values in the wrong order", "values ascending",
                                  "a duplicate index", "a value off by more than the bound"])
def test_check_topk_rejects(tied, name):
    logits, hist, vals, idx = tied
    mv, mi = _mutants(logits, hist, vals, idx)[name]
    assert not (torch.equal(mv, vals) and torch.equal(mi, idx))
    with pytest.raises(AssertionError):
        check_topk(mv, mi, logits, hist, K)
    if not torch.equal(mv, vals):
        return
    assert not torch.equal(mi, expected_topk(logits, hist, K))        # an index mutant: the exact-order comparison sees it too


def test_expected_topk_raises_on_a_cross_row_near_tie():
    logits = torch.full((2, 64), -4.0, dtype=torch.float16)
    logits[0, 3] = logits[1, 9] = 2.0
    logits[0, 5] = 1.0
    lse = logits.double().logsumexp(-1)
    h_eq = float(lse[1] - lse[0])                                    # history of row 1 that puts the two 2.0 level
    for h in (h_eq + 1e-5, h_eq - 1e-5, h_eq):
        with pytest.raises(AssertionError, match="near-tie"):
            expected_topk(logits, torch.tensor([0.0, h], dtype=torch.float64), 1)
    assert expected_topk(logits, torch.tensor([0.0, h_eq + 1e-3]), 2).tolist() == [64 + 9, 3]
    assert expected_topk(logits, torch.tensor([0.0, h_eq - 1e-3]), 2).tolist() == [3, 64 + 9]
    # rank k + 1 in another row: row 1's 2.0 sits 1e-5 below row 0's 1.0, the k-th value
    h_k = float((1.0 - lse[0]) - (2.0 - lse[1]))
    with pytest.raises(AssertionError, match="near-tie"):
        expected_topk(logits, torch.tensor([0.0, h_k - 1e-5], dtype=torch.float64), 2)
    assert expected_topk(logits, torch.tensor([0.0, h_k - 1e-3]), 2).tolist() == [3, 5]
    # equal values in two rows that are not identical rows
    swapped = torch.full((2, 64), -4.0, dtype=torch.float16)
    swapped[0, 3] = swapped[1, 9] = 2.0
    with pytest.raises(AssertionError, match="near-tie"):
        expected_topk(swapped, None, 1)


def test_expected_topk_orders_identical_rows_by_flat_index():
    g = torch.Generator().manual_seed(3)
    row = (torch.randn(8200, generator=g) * 2.5).half()
    row[torch.randperm(8200, generator=g)[:4]] = torch.tensor([12.0, 11.0, 10.0, 9.0], dtype=torch.float16)
    cols = torch.sort(row.float(), descending=True, stable=True).indices[:4]
    both = torch.stack([row, row])
    # distinct values: each appears in row 0, then in row 1
    assert expected_topk(both, torch.zeros(2), 8).tolist() == [int(c) + r * 8200 for c in cols for r in (0, 1)]
    # one shared value: all of row 0's columns come before row 1's
    grid = GRID[torch.randint(0, 8, (8200,), generator=g)].half()
    threes = torch.nonzero(grid == 3.0).flatten()
    n = threes.numel()
    got = expected_topk(torch.stack([grid, grid]), None, n + 3)
    assert torch.equal(got, torch.cat([threes, threes[:3] + 8200]))
    # rows that differ in history are not identical: their values merely collide
    with pytest.raises(AssertionError, match="near-tie"):
        expected_topk(both, torch.tensor([0.0, 1e-6]), 8)


def test_signed_zeros_are_equal_logits():
    logits = torch.full((1, 64), -1.0, dtype=torch.float16)
    logits[0, 5], logits[0, 40] = -0.0, 0.0
    assert expected_topk(logits, None, 2).tolist() == [5, 40]
    vals, idx = _model(logits, None, 2)
    check_topk(vals, idx, logits, None, 2)
    with pytest.raises(AssertionError):
        check_topk(vals, idx.flip(0), logits, None, 2)
    with pytest.raises(AssertionError):
        check_topk(vals[:1], torch.tensor([40]), logits, None, 1)
