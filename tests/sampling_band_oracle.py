"""Oracle of ``ls_sample_rows_ex``: tests/sampling_oracle.py plus the min_p and typical_p filters, restated in float64 from the
semantics in include/longspec_hip.h, and an operator namespace that lets the host loops run with them on the CPU.

Filters run in the order top_k -> top_p -> min_p -> typical_p, each on the set the former kept; the kept set is the band
``lo <= x <= hi`` of the row's finite values (``lo = hi = -inf``: the row has none and everything is kept).  Lives under tests/:
the product never imports it."""
import numpy as np
import torch

import oracle_ops
import sampling_oracle as so


def typical_distances(v, n, m, T):
    """Distinct values v (counts n) of the set S, row maximum m, fp32 temperature T as float: (Z, H, d(v))."""
    a = (m - v) / T
    w = np.exp(-a)
    Z = float((n * w).sum())
    s = np.log(Z) + a
    H = float((n * (w / Z) * s).sum())
    return Z, H, np.abs(s - H)


def band(x, temperature, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0):
    """(lo, hi) of one row x (float64 [V], finite or -inf)."""
    fin = x[np.isfinite(x)]
    if fin.size == 0:
        return -np.inf, -np.inf
    T = float(np.float32(temperature))
    m = float(fin.max())
    lo, hi = so.threshold(x, temperature, top_k, top_p), m
    mp, tp = float(np.float32(min_p)), float(np.float32(typical_p))
    if mp > 0.0:
        S = fin[fin >= lo]
        lo = float(S[np.exp((S - m) / T) >= mp].min())                  # the maximum always passes: w = 1 >= min_p
    if tp < 1.0:
        v, n = np.unique(fin[fin >= lo], return_counts=True)
        Z, H, d = typical_distances(v, n, m, T)
        order = np.argsort(d, kind="stable")
        ds, mass = d[order], np.cumsum((n * np.exp(-(m - v) / T))[order]) / Z
        last = np.searchsorted(ds, ds, side="right") - 1                # ties in d count together
        ok = mass[last] >= tp
        dstar = ds[np.argmax(ok)] if ok.any() else ds[-1]               # (the whole set holds mass 1 up to rounding)
        keep = v[d <= dstar]
        lo, hi = float(keep.min()), float(keep.max())
    return lo, hi


def sample_row(x, position, stream, seed, temperature, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0):
    """(idx, ((i1, i2), (key1, key2)), kept, lo, hi) of one row."""
    x = np.asarray(x, dtype=np.float64)
    lo, hi = band(x, temperature, top_k, top_p, min_p, typical_p)
    some = np.isfinite(lo)
    kept = ((x >= lo) & (x <= hi)) if some else np.ones(x.shape, dtype=bool)
    key = so.gumbel_keys(x, position, stream, seed, temperature)
    masked = np.where(kept, key, -np.inf)
    first = int(np.argmax(masked)) if some else 0                        # ties (and the all -inf row) to the smaller column
    n = int(kept.sum())
    if n < 2:
        return first, ((first, -1), (float(key[first]), -np.inf)), n, lo, hi
    kept2 = kept.copy()
    kept2[first] = False
    second = int(np.argmax(np.where(kept2, key, -np.inf))) if some else 1
    return first, ((first, second), (float(key[first]), float(key[second]))), n, lo, hi


def sample_rows(logits, positions, sampling, streams=None, return_top2=False, return_upper=False):
    """``longspec_amd.ops.sample_rows`` on CPU tensors."""
    shape = logits.shape[:-1]
    x = logits.reshape(-1, logits.shape[-1]).float().numpy().astype(np.float64)
    pos = positions.reshape(-1).to(torch.int64).numpy().copy()
    strm = streams.reshape(-1).numpy().copy() if streams is not None else np.zeros(len(pos), dtype=np.int64)
    assert len(pos) == x.shape[0] == len(strm)
    rows = [sample_row(x[r], pos[r], strm[r], sampling.seed, sampling.temperature, sampling.top_k, sampling.top_p,
                       getattr(sampling, "min_p", 0.0), getattr(sampling, "typical_p", 1.0)) for r in range(x.shape[0])]
    res = (torch.tensor([r[0] for r in rows], dtype=torch.int64).view(shape),)
    if return_top2:
        res += (torch.tensor([r[1][0] for r in rows], dtype=torch.int64).view(*shape, 2),
                torch.tensor([r[1][1] for r in rows], dtype=torch.float32).view(*shape, 2),
                torch.tensor([r[2] for r in rows], dtype=torch.int32).view(shape),
                torch.tensor([r[3] for r in rows], dtype=torch.float32).view(shape))
    if return_upper:
        res += (torch.tensor([r[4] for r in rows], dtype=torch.float32).view(shape),)
    return res if len(res) > 1 else res[0]


class Ops:
    """``tests/oracle_ops.py`` plus ``sample_rows`` with the band filters: the namespace of the host-logic tests."""

    def __getattr__(self, name):
        return getattr(oracle_ops, name)

    sample_rows = staticmethod(sample_rows)


ops = Ops()


def robust_band_gap(x, position, sampling, m):
    """Twin of ``sampled_runs.robust_gap`` for min_p and typical_p (top_k / top_p off): the key gap between the oracle's winner
    of row x and the best other token that COULD be kept, were every logit off by up to m; -inf when the winner itself could
    drop out.  With e = m / T:

    min_p     u_j = (x_j - max) / T moves by at most 2e (x_j and the maximum by e each).  Kept for sure: u_j - ln min_p >= 2e;
              kept at most: u_j - ln min_p >= -2e.
    typical_p a_j = (max - x_j) / T moves by at most 2e (delta_j); each weight exp(-a_j) by a factor within exp(+-2e), so each
              q_j = w_j / Z by a factor within exp(+-4e).  A = sum q a:  A' - A = sum q'_j delta_j + sum (q'_j - q_j)(a_j - A)
              (the second sum may be centred because sum (q' - q) = 0), hence |A' - A| <= 2e + (exp(4e) - 1) * sd with
              sd = sum q |a - A|, and every distance d_j = |a_j - A| (= |s_j - H|: ln Z cancels) moves by at most
              D = 4e + (exp(4e) - 1) * sd.  The mass of a set of tokens, relative to Z, moves by a factor within exp(+-4e).
              Token j is kept iff the mass of the tokens STRICTLY closer than j is below typical_p (d* is the smallest
              distance whose closed ball reaches it).  The perturbed set {d'_i < d'_j} lies between {d_i < d_j - 2D} and
              {d_i < d_j + 2D}.  Kept for sure: mass{d_i < d_j + 2D} * exp(4e) < typical_p.  Kept at most:
              mass{d_i < d_j - 2D} * exp(-4e) < typical_p.
    With both on, typical_p runs on the tokens min_p keeps: a token min_p may or may not keep changes S, so such rows count as
    -inf unless the sure and the possible min_p sets agree."""
    T = float(np.float32(sampling.temperature))
    e = m / T
    mp, tp = float(np.float32(sampling.min_p)), float(np.float32(sampling.typical_p))
    assert sampling.top_k == 0 and sampling.top_p == 1.0
    win = sample_row(x, position, 0, sampling.seed, sampling.temperature, 0, 1.0, mp, tp)[0]
    key = so.gumbel_keys(x, position, 0, sampling.seed, sampling.temperature)
    fin = np.isfinite(x)
    sure, may = fin.copy(), fin.copy()
    xm = x[fin].max()
    with np.errstate(invalid="ignore"):
        u = np.where(fin, (x - xm) / T, -np.inf)
    if mp > 0.0:
        sure, may = sure & (u - np.log(mp) >= 2 * e), may & (u - np.log(mp) >= -2 * e)
        if tp < 1.0 and not np.array_equal(sure, may):
            return -np.inf
    if tp < 1.0:
        S = may
        a = np.where(S, -u, 0.0)
        w = np.where(S, np.exp(-a), 0.0)
        q = w / w.sum()
        A = float((q * a).sum())
        d = np.where(S, np.abs(a - A), np.inf)
        D = 4 * e + (np.exp(4 * e) - 1.0) * float((q * np.abs(a - A)).sum())
        order = np.argsort(d, kind="stable")
        ds, cum = d[order], np.cumsum(q[order])
        below = lambda t: np.where(np.searchsorted(ds, t, side="left") > 0,
                                   cum[np.maximum(np.searchsorted(ds, t, side="left") - 1, 0)], 0.0)   # mass{d_i < t}
        f = np.exp(4 * e)
        sure, may = sure & S & (below(d + 2 * D) * f < tp), may & S & (below(d - 2 * D) / f < tp)
    if not sure[win]:
        return -np.inf
    others = may.copy()
    others[win] = False
    return float(key[win] - key[others].max()) if others.any() else np.inf


def min_robust_band_gap(record, n_tokens, prompt_len, sampling, m):
    return min(robust_band_gap(record["rows"][prompt_len - 1 + i], prompt_len - 1 + i, sampling, m) for i in range(n_tokens))
