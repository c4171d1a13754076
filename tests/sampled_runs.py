"""Shared by the sampled host-logic tests (CPU oracle) and their GPU twins: the cross-loop rule of sampled decoding.

With one seed the vanilla, chain, MagicDec and tree loops draw the same noise for a position, so they emit the same text --
up to near-ties: the loops run different kernels on the way to the logits (row counts, split counts), the 16-bit logits differ
by an ulp now and then, and where the two best keys of a position are closer than that, a loop may take the runner-up.  A spy
on ``sample_rows`` in the vanilla run records every position's winner, runner-up and key gap; a loop may leave the vanilla
text only at a position where it took the runner-up and the gap is below ``tol / T``; the comparison stops there."""
import math

import numpy as np
import torch

import sampling_oracle as so

TOL = {torch.float16: 0.02, torch.bfloat16: 0.25}       # the project's near-tie bounds on 16-bit logits (test_gpu_generate.py)


class Top2Spy:
    """An operator namespace that forwards to `base` and records, per (stream, position) of every ``sample_rows`` call,
    (winner, runner-up, key gap, kept).  One host read per call: for eager runs only."""

    def __init__(self, base):
        self._base = base
        self.rec = {}
        self.rows = {}                   # (stream, position) -> the row's logits (float64), for `robust_gap`

    def __getattr__(self, name):
        return getattr(self._base, name)

    def sample_rows(self, logits, positions, sampling, streams=None, return_top2=False):
        idx, t2i, t2k, kept, thr = self._base.sample_rows(logits, positions, sampling, streams=streams, return_top2=True)
        pos = positions.reshape(-1).tolist()
        strm = streams.reshape(-1).tolist() if streams is not None else [0] * len(pos)
        ti, tk, kp = t2i.reshape(-1, 2).tolist(), t2k.reshape(-1, 2).tolist(), kept.reshape(-1).tolist()
        x = logits.reshape(len(pos), -1).float().cpu().numpy().astype(np.float64)
        for r in range(len(pos)):
            gap = tk[r][0] - tk[r][1] if ti[r][1] >= 0 else math.inf
            self.rec[(int(strm[r]), int(pos[r]))] = (ti[r][0], ti[r][1], gap, kp[r])
            self.rows[(int(strm[r]), int(pos[r]))] = x[r]
        return (idx, t2i, t2k, kept, thr) if return_top2 else idx


def vanilla_with_record(m, base_ops, run, sampling, device=None, max_gen_len=None):
    """(output_ids [1, max_gen] on the CPU, {position: (winner, runner-up, gap, kept)}) of a spied vanilla run."""
    spy = Top2Spy(base_ops)
    saved, saved_graphs = m.ops, m.GRAPH_ROUNDS
    _set_ops(m, spy)
    m.GRAPH_ROUNDS = False
    try:
        ids = run["prompt"].to(device) if device else run["prompt"]
        pl = torch.tensor([run["prompt_len"]], device=device)
        out, num, _ = m.vanilla_generate(ids, pl, max_gen_len=max_gen_len or run["max_gen_len"], eos_id=run["eos_id"],
                                         sampling=sampling)
    finally:
        _set_ops(m, saved)
        m.GRAPH_ROUNDS = saved_graphs
    rec = {pos: v for (s, pos), v in spy.rec.items() if s == 0}
    rec["rows"] = {pos: v for (s, pos), v in spy.rows.items() if s == 0}
    return out.cpu(), rec


def _set_ops(m, ops):
    """The loops reach ``sample_rows`` through the model object's namespace (as the spies of test_host_generate.py)."""
    m.ops = ops


def with_long_prompt(run, n):
    """The run with its prompt tiled to n tokens (MagicDec's streaming cache needs a prompt of 1024 + tokens)."""
    reps = -(-n // run["prompt"].size(1))
    return {**run, "prompt": run["prompt"].repeat(1, reps)[:, :n].contiguous(), "prompt_len": n}


def min_gap(record, n_tokens, prompt_len):
    """Smallest key gap over the positions that produced tokens 0 .. n_tokens-1 (token i is drawn at position P - 1 + i)."""
    return min(record[prompt_len - 1 + i][2] for i in range(n_tokens))


def robust_gap(x, position, sampling, m):
    """The key gap between the oracle's winner of row x and the best other token that COULD be kept, were every logit off by up
    to m: -inf when the winner itself could drop out.  A filter's threshold is a step: a logit that moves by an ulp can move
    the k-th value, or the value at which the mass from the top reaches top_p, and with it a token into or out of the kept
    set, however far apart the keys are.  Kept for sure: x >= t_k + m and mass above x, times exp(2m / T), below top_p of the
    total (each mass changes by a factor within exp(+-m / T), a ratio of sums by at most the square).  Kept at most: the same
    with -m and the inverse factor."""
    T = float(np.float32(sampling.temperature))
    win = so.sample_row(x, position, 0, sampling.seed, sampling.temperature, sampling.top_k, sampling.top_p)[0]
    key = so.gumbel_keys(x, position, 0, sampling.seed, sampling.temperature)
    sure, may = np.isfinite(x), np.isfinite(x)
    t_k = so.threshold(x, sampling.temperature, sampling.top_k, 1.0)
    if sampling.top_k > 0:
        sure, may = sure & (x >= t_k + m), may & (x >= t_k - m)
    if sampling.top_p < 1.0:
        mass = np.where(x >= t_k, so.masses(x, sampling.temperature), 0.0)
        order = np.argsort(-x, kind="stable")
        xs, ms = x[order], mass[order]
        cum = np.concatenate([[0.0], np.cumsum(ms)])[:-1]                      # mass in front of each sorted position
        first = np.searchsorted(-xs, -xs, side="left")                          # ... of the first position with the same value
        above = np.empty_like(x)
        above[order] = cum[first] / ms.sum()
        f, p = math.exp(2 * m / T), float(np.float32(sampling.top_p))
        sure, may = sure & (above * f < p), may & (above / f < p)
    if not sure[win]:
        return -math.inf
    others = may.copy()
    others[win] = False
    return float(key[win] - key[others].max()) if others.any() else math.inf


def min_robust_gap(record, n_tokens, prompt_len, sampling, m):
    return min(robust_gap(record["rows"][prompt_len - 1 + i], prompt_len - 1 + i, sampling, m) for i in range(n_tokens))


def parting(out, n, v_out, record, prompt_len, temperature, tol, what):
    """None when ``out[0, :n]`` is the vanilla text; else the index of the first other token, after asserting that it is an
    explained near-tie."""
    a, b = out[0, :n].cpu(), v_out[0, :n]
    neq = (a != b).nonzero()
    if neq.numel() == 0:
        return None
    i = int(neq[0])
    win, runner, gap, _ = record[prompt_len - 1 + i]
    assert int(b[i]) == win, f"{what}: the vanilla record does not hold the vanilla token at {i}"
    assert int(a[i]) == runner and gap < tol / temperature, \
        f"{what}: parts from the vanilla text at token {i} (took {int(a[i])}, vanilla {win}, runner-up {runner}, key gap {gap})"
    return i


def stop_len(v_out, eos, n):
    """Tokens of the vanilla text that count: up to and including its first eos."""
    row = v_out[0, :n].tolist()
    return row.index(eos) + 1 if eos is not None and eos in row else n
