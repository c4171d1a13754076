"""Oracle of ``ops.token_logprobs`` / ``ops.logprob_commit`` (``ls_token_logprobs`` / ``ls_logprob_commit``): the definition of
``longspec_amd/logprobs.py`` in numpy float64 on the CPU, an exact commit, and an operator namespace layered on
``penalty_oracle.ops`` that lets the host loops run with ``logprobs=`` on the CPU.  The temperature is the fp32 number the C
ABI receives.  Lives under tests/: the product never imports it."""
import numpy as np
import torch

import penalty_oracle


def row_logprobs64(x, temperature):
    """float64 log-soft-max of one row of logits ``x`` (any float array) at ``temperature``, over the whole row."""
    x = np.asarray(x, dtype=np.float64)
    T = float(np.float32(temperature))
    m = x.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (x - m) / T
        return z - np.log(np.exp(z).sum())


def row_order(x):
    """Columns of a row by (logit descending, column ascending); -0.0 == +0.0."""
    x = np.asarray(x, dtype=np.float64) + 0.0            # -0.0 + 0.0 = +0.0
    return np.lexsort((np.arange(x.size), -x))


def token_logprobs64(logits, ids, temperature=1.0, n=0):
    """numpy float64: (row_lp [b, R], top_val [b, R, n], top_idx [b, R, n] int64) of ``ops.token_logprobs``."""
    x = logits if logits.dim() == 3 else logits.unsqueeze(1)
    b, R, V = x.shape
    x = x.to(torch.float64).cpu().numpy()
    ids = ids.reshape(b, R).cpu().numpy()
    row_lp = np.full((b, R), np.nan)
    top_val = np.full((b, R, n), -np.inf)
    top_idx = np.full((b, R, n), -1, dtype=np.int64)
    for z in range(b):
        for r in range(R):
            lp = row_logprobs64(x[z, r], temperature)
            if 0 <= ids[z, r] < V:
                row_lp[z, r] = lp[ids[z, r]]
            order = row_order(x[z, r])[:n]
            top_idx[z, r, :order.size] = order
            top_val[z, r, :order.size] = lp[order]
    return row_lp, top_val, top_idx


def token_logprobs(logits, ids, temperature=1.0, n=0):
    """``longspec_amd.ops.token_logprobs`` on CPU tensors: the float64 values rounded once to fp32."""
    row_lp, top_val, top_idx = token_logprobs64(logits, ids, temperature, n)
    return (torch.from_numpy(row_lp.astype(np.float32)), torch.from_numpy(top_val.astype(np.float32)), torch.from_numpy(top_idx))


def logprob_commit(rows, out, base, base_add=0, num=None, index_map=None):
    """``longspec_amd.ops.logprob_commit`` on CPU tensors (in place, exact)."""
    row_lp, top_val, top_idx = rows
    b, R = row_lp.shape
    W = out.token.shape[1]
    J = index_map.shape[1] if index_map is not None else R
    for z in range(b):
        cnt = J if num is None else max(0, min(int(num[z]), J))
        for j in range(cnt):
            src = int(index_map[z, j]) if index_map is not None else j
            dst = int(base[z]) + base_add + j
            if not (0 <= src < R and 0 <= dst < W):
                continue
            out.token[z, dst] = row_lp[z, src]
            out.top[z, dst] = top_val[z, src]
            out.top_ids[z, dst] = top_idx[z, src]


class Ops:
    """``penalty_oracle.ops`` plus the two log-prob operators: the operator namespace of the ``logprobs=`` host-logic tests."""

    def __getattr__(self, name):
        return getattr(penalty_oracle.ops, name)

    token_logprobs = staticmethod(token_logprobs)
    logprob_commit = staticmethod(logprob_commit)


ops = Ops()
