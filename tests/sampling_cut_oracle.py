"""Oracle of ``ls_sample_rows_cut``: tests/sampling_band_oracle.py plus the top_n_sigma and xtc cuts, restated in float64 from
the semantics in include/longspec_hip.h and longspec_amd/cut.py (no reference counterpart exists), and an operator namespace
that lets the host loops run with ``cut=`` on the CPU.

Filters run in the order top_n_sigma -> top_k -> top_p -> min_p -> typical_p -> xtc, each on the set the former kept; the kept
set is the band ``lo <= x <= hi`` of the row's finite values (``lo = hi = -inf``: the row has none and everything is kept).
The coin of xtc is a Philox4x32-10 written out here on Python integers, independently of the kernel's source and of the numpy
one in sampling_oracle.py.  Lives under tests/: the product never imports it."""
import math

import numpy as np
import torch

import lookup_tree_oracle
import sampled_runs as sr
import sampling_band_oracle as sbo
import sampling_oracle as so

M32 = 0xFFFFFFFF


def philox_words(counter, key):
    """Philox4x32-10 on Python integers: counter four and key two 32-bit words -> four 32-bit words."""
    c0, c1, c2, c3 = (int(c) & M32 for c in counter)
    k0, k1 = (int(k) & M32 for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def coin(seed, position, stream=0):
    """u of the row's coin: counter (0xFFFFFFFF, position lo, position hi, stream), key = the seed's halves, word 0."""
    position, seed = int(position) & (2 ** 64 - 1), int(seed) & (2 ** 64 - 1)
    w = philox_words((M32, position & M32, position >> 32, int(stream) & M32), (seed & M32, seed >> 32))[0]
    return ((w >> 9) + 0.5) * 2.0 ** -23                  # exact in fp32, in (0, 1)


def fires(seed, position, stream, probability):
    """u < P, both fp32."""
    return bool(np.float32(coin(seed, position, stream)) < np.float32(probability))


def sigma_threshold(x, n):
    """(sigma, t = m - n sigma) of one row x (float64, finite or -inf): the population deviation of the finite entries; n is
    the fp32 value the kernel is handed.  (nan, -inf) for a row without a finite entry."""
    fin = x[np.isfinite(x)]
    if fin.size == 0:
        return math.nan, -np.inf
    sigma = float(np.sqrt(np.mean((fin - fin.mean()) ** 2)))
    return sigma, float(fin.max()) - float(np.float32(n)) * sigma


def xtc_cut(v, n, m, T, theta):
    """Distinct values v (counts n) of the set S, row maximum m: v*, the smallest value with q(v*) >= theta under the exact
    float64 masses of S, or None."""
    w = np.exp((v - m) / T)
    q = w / float((n * w).sum())
    ok = q >= float(np.float32(theta))
    return float(v[ok].min()) if ok.any() else None


def band(x, temperature, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0, cut=None, fired=False):
    """(lo, hi) of one row x (float64 [V], finite or -inf); ``fired``: the row's xtc coin."""
    n_sigma = cut.top_n_sigma if cut is not None else 0.0
    if n_sigma > 0.0 and np.isfinite(x).any():
        _, t = sigma_threshold(x, n_sigma)
        x = np.where(x >= t, x, -np.inf)                  # holds the maximum; the later filters see what it kept
    lo, hi = sbo.band(x, temperature, top_k, top_p, min_p, typical_p)
    if cut is not None and fired and cut.xtc_probability > 0.0 and np.isfinite(lo):
        S = x[np.isfinite(x) & (x >= lo) & (x <= hi)]
        v, n = np.unique(S, return_counts=True)
        vstar = xtc_cut(v, n, float(x[np.isfinite(x)].max()), float(np.float32(temperature)), cut.xtc_threshold)
        if vstar is not None:
            hi = vstar
    return lo, hi


def sample_row(x, position, stream, seed, temperature, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0, cut=None):
    """(idx, ((i1, i2), (key1, key2)), kept, lo, hi) of one row."""
    x = np.asarray(x, dtype=np.float64)
    fired = cut is not None and fires(seed, position, stream, cut.xtc_probability)
    lo, hi = band(x, temperature, top_k, top_p, min_p, typical_p, cut, fired)
    some = np.isfinite(lo)
    kept = ((x >= lo) & (x <= hi)) if some else np.ones(x.shape, dtype=bool)
    key = so.gumbel_keys(x, position, stream, seed, temperature)
    first = int(np.argmax(np.where(kept, key, -np.inf))) if some else 0
    n = int(kept.sum())
    if n < 2:
        return first, ((first, -1), (float(key[first]), -np.inf)), n, lo, hi
    kept2 = kept.copy()
    kept2[first] = False
    second = int(np.argmax(np.where(kept2, key, -np.inf))) if some else 1
    return first, ((first, second), (float(key[first]), float(key[second]))), n, lo, hi


def sample_rows(logits, positions, sampling, streams=None, return_top2=False, return_upper=False, cut=None):
    """``longspec_amd.ops.sample_rows`` on CPU tensors."""
    shape = logits.shape[:-1]
    x = logits.reshape(-1, logits.shape[-1]).float().numpy().astype(np.float64)
    pos = positions.reshape(-1).to(torch.int64).numpy().copy()
    strm = streams.reshape(-1).numpy().copy() if streams is not None else np.zeros(len(pos), dtype=np.int64)
    assert len(pos) == x.shape[0] == len(strm)
    rows = [sample_row(x[r], pos[r], strm[r], sampling.seed, sampling.temperature, sampling.top_k, sampling.top_p,
                       getattr(sampling, "min_p", 0.0), getattr(sampling, "typical_p", 1.0), cut) for r in range(x.shape[0])]
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
    """``sampling_band_oracle.ops`` with ``cut=`` on ``sample_rows``: the namespace of the host-logic tests.  What that
    namespace lacks -- the drafters of the prompt-lookup loops -- comes from ``lookup_tree_oracle.ops``."""

    def __getattr__(self, name):
        try:
            return getattr(sbo.ops, name)
        except AttributeError:
            return getattr(lookup_tree_oracle.ops, name)

    sample_rows = staticmethod(sample_rows)


ops = Ops()


class CutSpy(sr.Top2Spy):
    """``sampled_runs.Top2Spy`` whose ``sample_rows`` takes ``cut=`` and also keeps every row's band edges."""

    def __init__(self, base):
        super().__init__(base)
        self.edges = {}                  # (stream, position) -> (smallest kept value, largest kept value)

    def sample_rows(self, logits, positions, sampling, streams=None, return_top2=False, cut=None):
        idx, t2i, t2k, kept, thr, upper = self._base.sample_rows(logits, positions, sampling, streams=streams, return_top2=True,
                                                                 return_upper=True, cut=cut)
        pos = positions.reshape(-1).tolist()
        strm = streams.reshape(-1).tolist() if streams is not None else [0] * len(pos)
        ti, tk, kp = t2i.reshape(-1, 2).tolist(), t2k.reshape(-1, 2).tolist(), kept.reshape(-1).tolist()
        lo, hi = thr.reshape(-1).tolist(), upper.reshape(-1).tolist()
        x = logits.reshape(len(pos), -1).float().cpu().numpy().astype(np.float64)
        for r in range(len(pos)):
            gap = tk[r][0] - tk[r][1] if ti[r][1] >= 0 else math.inf
            self.rec[(int(strm[r]), int(pos[r]))] = (ti[r][0], ti[r][1], gap, kp[r])
            self.rows[(int(strm[r]), int(pos[r]))] = x[r]
            self.edges[(int(strm[r]), int(pos[r]))] = (lo[r], hi[r])
        return (idx, t2i, t2k, kept, thr) if return_top2 else idx


def vanilla_with_record(m, base_ops, run, sampling, cut, device=None, max_gen_len=None):
    """``sampled_runs.vanilla_with_record`` under ``cut=``; the record also has ``edges``: {position: (lo, hi)}."""
    spy = CutSpy(base_ops)
    saved, saved_graphs = m.ops, m.GRAPH_ROUNDS
    m.ops, m.GRAPH_ROUNDS = spy, False
    try:
        ids = run["prompt"].to(device) if device else run["prompt"]
        pl = torch.tensor([run["prompt_len"]], device=device)
        out, num, _ = m.vanilla_generate(ids, pl, max_gen_len=max_gen_len or run["max_gen_len"], eos_id=run["eos_id"],
                                         sampling=sampling, cut=cut)
    finally:
        m.ops, m.GRAPH_ROUNDS = saved, saved_graphs
    rec = {pos: v for (s, pos), v in spy.rec.items() if s == 0}
    rec["rows"] = {pos: v for (s, pos), v in spy.rows.items() if s == 0}
    rec["edges"] = {pos: v for (s, pos), v in spy.edges.items() if s == 0}
    return out.cpu(), rec


def robust_cut_gap(x, position, sampling, cut, tol):
    """Twin of ``sampled_runs.robust_gap`` under ``cut`` (and top_k / top_p; min_p and typical_p off): the key gap between the
    oracle's winner of row x and the best other token that COULD be kept, were every logit off by up to tol; -inf when the
    winner itself could drop out, at the lower edge or at the upper one.  Every filter takes a pair of sets -- the tokens kept
    for sure and the tokens kept at most, S_sure <= S' <= S_may for every perturbed S' -- to the next pair.  With e = tol,
    f = exp(2e / T) (a weight exp(x / T) moves by a factor within exp(+-e / T), a ratio of two by the square), w_j =
    exp((x_j - m) / T), Z_sure and Z_may the sums of w over the two sets, so that the perturbed share of a token or a set lies
    between w / (f Z_may) and f w / Z_sure:

    top_n_sigma  m moves by at most e, and so does sigma (the deviation of x + d is at most that of x plus that of d, which is
                 at most e), hence t = m - n sigma by (1 + n) e and x_j - t by (2 + n) e.  Kept for sure: x_j - t >= (2 + n) e;
                 kept at most: x_j - t >= -(2 + n) e.
    top_k        as ``sampled_runs.robust_gap``: x_j >= t_k + e for sure, x_j >= t_k - e at most.
    top_p        j is kept iff the share of the tokens above it is below p; a token within 2e may change sides.  Kept for
                 sure: f sum{w_i : i in S_may, i != j, x_i > x_j - 2e} / Z_sure < p.  Kept at most:
                 sum{w_i : i in S_sure, x_i > x_j + 2e} / (f Z_may) < p.
    xtc          Q_sure = {j in S_sure : w_j / (f Z_may) >= theta} qualify for sure, Q_may = {j in S_may : f w_j / Z_sure >=
                 theta} at most; the cut value is the smallest perturbed value of the qualifying tokens and a token is kept iff
                 it is not above it.  Kept for sure: x_j + 2e <= x_i for every other i in Q_may.  Kept at most: x_j - 2e <= x_i
                 for every other i in Q_sure."""
    assert sampling.min_p == 0.0 and sampling.typical_p == 1.0
    T = float(np.float32(sampling.temperature))
    e, f = tol, math.exp(2 * tol / T)
    win = sample_row(x, position, 0, sampling.seed, sampling.temperature, sampling.top_k, sampling.top_p, cut=cut)[0]
    key = so.gumbel_keys(x, position, 0, sampling.seed, sampling.temperature)
    fin = np.isfinite(x)
    xf = np.where(fin, x, -np.inf)
    w = np.where(fin, np.exp((np.where(fin, x, 0.0) - x[fin].max()) / T), 0.0)
    sure, may = fin.copy(), fin.copy()
    if cut.top_n_sigma > 0.0:
        _, t = sigma_threshold(x, cut.top_n_sigma)
        slack = (2.0 + float(np.float32(cut.top_n_sigma))) * e
        sure, may = sure & (xf - t >= slack), may & (xf - t >= -slack)
    if sampling.top_k > 0:
        t_k = so.threshold(x, sampling.temperature, sampling.top_k, 1.0)
        sure, may = sure & (xf >= t_k + e), may & (xf >= t_k - e)

    def mass_above(S, shift):
        """sum{w_i : i in S, x_i > x_j + shift} for every j."""
        order = np.argsort(xf, kind="stable")
        xs, ws = xf[order], np.where(S, w, 0.0)[order]
        cum = np.concatenate([[0.0], np.cumsum(ws)])
        return cum[-1] - cum[np.searchsorted(xs, xf + shift, side="right")]

    if sampling.top_p < 1.0:
        p = float(np.float32(sampling.top_p))
        z_sure, z_may = float(w[sure].sum()), float(w[may].sum())
        hi_share = (mass_above(may, -2 * e) - np.where(may, w, 0.0) * (2 * e > 0)) * f / z_sure if z_sure > 0 else np.inf
        lo_share = mass_above(sure, 2 * e) / (f * z_may)
        sure, may = sure & (hi_share < p), may & (lo_share < p)
    if cut.xtc_probability > 0.0 and fires(sampling.seed, position, 0, cut.xtc_probability):
        theta = float(np.float32(cut.xtc_threshold))
        z_sure, z_may = float(w[sure].sum()), float(w[may].sum())
        q_sure = sure & (w / (f * z_may) >= theta)
        q_may = may & (f * w / z_sure >= theta) if z_sure > 0 else may.copy()

        def floor_of_others(Q):
            """min over i in Q, i != j, of x_i, for every j (inf where there is none)."""
            idx = np.flatnonzero(Q)
            if idx.size == 0:
                return np.full(x.shape, np.inf)
            idx = idx[np.argsort(xf[idx], kind="stable")]
            out = np.full(x.shape, xf[idx[0]])
            out[idx[0]] = xf[idx[1]] if idx.size > 1 else np.inf
            return out

        sure, may = sure & (xf + 2 * e <= floor_of_others(q_may)), may & (xf - 2 * e <= floor_of_others(q_sure))
    if not sure[win]:
        return -math.inf
    others = may.copy()
    others[win] = False
    return float(key[win] - key[others].max()) if others.any() else math.inf


def min_robust_cut_gap(record, n_tokens, prompt_len, sampling, cut, tol):
    return min(robust_cut_gap(record["rows"][prompt_len - 1 + i], prompt_len - 1 + i, sampling, cut, tol) for i in range(n_tokens))
