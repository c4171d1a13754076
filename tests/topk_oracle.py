"""Exact oracle for ``ops.logprob_topk``: the joint top-k over all rows of ``log_softmax(row) + history[row]``.

Pure torch on the CPU.  Values are fp64, ``logit - logsumexp64(row) + history[row]``.  The kernel's documented order is
"value descending, ties to the smaller flat index ``row * V + column``"; equal logits of one row give bit-equal kernel values
(the same fp32 expression on the same operands), so inside a row the order is (logit descending, column ascending) EXACTLY.
Only across rows can two fp32 values fall in another order than their fp64 values, when those are closer than the fp32
noise of the two log-sum-exps.  Two entry points:

``expected_topk``  for inputs built so that no such cross-row near-tie touches the top k: asserts that on the fp64 values
                   (a rule on the INPUT, checked before any GPU call) and returns the one correct index list;
``check_topk``     for inputs where near-ties cannot be excluded (random data): asserts everything that still is exact.

-0.0 and +0.0 are equal logits (the contract is torch's ``argmax`` / ``topk`` on floats)."""
import torch

TOL = 1e-5          # |kernel fp32 value - fp64 value|: torch's own fp32 log_softmax is within 4.6e-6 of fp64 at V = 152064


def _rows(logits, history):
    if logits.dim() == 3:
        assert logits.shape[0] == 1, "one batch element at a time"
        logits = logits[0]
    assert logits.dim() == 2
    logits = logits.detach().cpu()
    if history is not None:
        history = history.detach().cpu().reshape(-1).double()
        assert history.numel() == logits.shape[0]
    return logits, history


def _groups(logits, lse, history):
    """group[r] = smallest row index whose logits and history are identical to row r's (deliberately identical rows)."""
    R = logits.shape[0]
    group = list(range(R))
    for r in range(1, R):
        for s in range(r):
            if group[s] != s or lse[s] != lse[r]:
                continue
            if history is not None and history[s] != history[r]:
                continue
            if torch.equal(logits[s], logits[r]):
                group[r] = s
                break
    return torch.tensor(group)


def fp64_values(logits, history):
    """[R, V] fp64 ``logit - logsumexp(row) + history[row]``; identical rows get bit-identical values."""
    logits, history = _rows(logits, history)
    x = logits.double()
    lse = torch.logsumexp(x, dim=-1)
    group = _groups(logits, lse, history)
    lse = lse[group]                                   # (a reduction need not round alike for two equal rows; make it so)
    lp = x - lse[:, None]
    if history is not None:
        lp = lp + history[:, None]
    return lp, group


def expected_topk(logits, history, k, tol=TOL):
    """The exact flat indices [k] (int64) ``logprob_topk`` must return: fp64 value descending, bit-equal values (equal logits
    of one row, or of deliberately identical rows) by flat index ascending.  Raises AssertionError unless that list is the
    only answer an fp32 evaluation within ``tol`` can give: no element with a DIFFERENT fp64 value, and no element of another
    (non-identical) row at all, lies within ``2 * tol`` of any of the k values -- which covers rank k + 1 too."""
    lp, group = fp64_values(logits, history)
    R, V = lp.shape
    assert 1 <= k <= R * V
    order = torch.sort(lp.reshape(-1), descending=True, stable=True).indices[:k]       # stable: ties by flat index ascending
    top = lp.reshape(-1)[order]
    top_group = group[order // V]
    srt = torch.sort(lp, dim=-1).values                                                # ascending, per row
    q = top[None, :].expand(R, k).contiguous()
    near = (torch.searchsorted(srt, q + 2 * tol, right=True) - torch.searchsorted(srt, q - 2 * tol, right=False))
    equal = torch.searchsorted(srt, q, right=True) - torch.searchsorted(srt, q, right=False)
    same = group[:, None] == top_group[None, :]                                        # [R, k]: row is (identical to) the value's row
    bad = torch.where(same, near - equal, near)
    if bool((bad != 0).any()):
        r, i = [int(t[0]) for t in torch.nonzero(bad, as_tuple=True)]
        raise AssertionError(f"expected_topk: the input has a near-tie: row {r} holds {int(bad[r, i])} value(s) within {2 * tol:g} of "
                             f"rank {i} (flat index {int(order[i])}, value {float(top[i]):.9f}); the expected order is not unique")
    return order.to(torch.int64)


def check_topk(got_vals, got_idx, logits, history, k, tol=TOL):
    """Everything that is exact about a ``logprob_topk`` answer on arbitrary finite input (``got_vals`` fp32 [k], ``got_idx``
    int64 [k], one batch element).  Returns the observed max |got - fp64|."""
    lp, _ = fp64_values(logits, history)
    logits, _ = _rows(logits, history)
    R, V = lp.shape
    got_vals = got_vals.detach().cpu().reshape(-1)
    got_idx = got_idx.detach().cpu().reshape(-1)
    assert got_vals.dtype == torch.float32 and got_idx.dtype == torch.int64
    assert got_vals.numel() == k and got_idx.numel() == k
    # indices unique and in range
    assert bool(((got_idx >= 0) & (got_idx < R * V)).all()), f"index out of range: {got_idx.tolist()}"
    assert got_idx.unique().numel() == k, f"duplicate index: {got_idx.tolist()}"
    # values non-increasing, bit-equal values in ascending index order
    assert bool(torch.isfinite(got_vals).all())
    dv = got_vals[:-1] - got_vals[1:]
    assert bool((dv >= 0).all()), f"values not sorted descending at {torch.nonzero(dv < 0).flatten().tolist()}"
    tied = dv == 0
    assert bool((got_idx[:-1] < got_idx[1:])[tied].all()), \
        f"equal values not in ascending index order at {torch.nonzero(tied & ~(got_idx[:-1] < got_idx[1:])).flatten().tolist()}"
    # each value within tol of the fp64 value of the element it names
    flat = lp.reshape(-1)
    err = (got_vals.double() - flat[got_idx]).abs()
    assert float(err.max()) <= tol, f"value {int(err.argmax())} is {float(err.max()):.3e} from the fp64 value of its index (bound {tol:g})"
    # the selection: everything clearly above the k-th fp64 value is in, nothing clearly below it is
    kth = torch.topk(flat, k).values[-1]
    sel = torch.zeros(R * V, dtype=torch.bool)
    sel[got_idx] = True
    must = flat > kth + 2 * tol
    assert bool(sel[must].all()), f"missing {torch.nonzero(must & ~sel).flatten().tolist()}: more than {2 * tol:g} above the k-th value"
    assert bool((flat[got_idx] >= kth - 2 * tol).all()), \
        f"selected {got_idx[flat[got_idx] < kth - 2 * tol].tolist()}: more than {2 * tol:g} below the k-th value"
    # inside a row log-soft-max is monotone in the logit and equal logits tie exactly: the selected columns of a row are a
    # prefix of its (logit descending, column ascending) order
    rows, cols = got_idx // V, got_idx % V
    for r in rows.unique().tolist():
        mine = cols[rows == r].sort().values
        want = torch.sort(logits[r].float(), descending=True, stable=True).indices[:mine.numel()].sort().values
        assert torch.equal(mine, want), f"row {r}: selected columns {mine.tolist()} are not its {mine.numel()} best {want.tolist()}"
    return float(err.max())
