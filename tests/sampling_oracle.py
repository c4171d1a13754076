"""Oracle of ``ops.sample_rows`` / ``ls_sample_rows``: Philox4x32-10 in numpy and the float64 restatement of the operator
(filter by exact counts, masses and keys in float64), plus an operator namespace that lets the host loops run sampled on the
CPU.  Lives under tests/: the product never imports it."""
import numpy as np
import torch

import oracle_ops

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two uint32 scalars -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in counter])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]                   # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> _S32, p0 & _MASK, p1 >> _S32, p1 & _MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def uniforms(V, position, stream, seed):
    """u_j, j < V, of one row: float64 array (every value is exact in fp32 and lies in (0, 1))."""
    position, stream, seed = int(position) & (2 ** 64 - 1), int(stream) & 0xFFFFFFFF, int(seed)
    blocks = np.arange((V + 3) // 4, dtype=np.uint64)
    w = philox4x32_10((blocks, position & 0xFFFFFFFF, position >> 32, stream), (seed & 0xFFFFFFFF, seed >> 32))
    w = np.stack(w, axis=1).reshape(-1)[:V]
    return ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel_keys(x, position, stream, seed, temperature):
    """key_j = x_j / T - ln(-ln u_j) in float64; T is the fp32 value the kernel is handed."""
    T = float(np.float32(temperature))
    u = uniforms(x.shape[0], position, stream, seed)
    with np.errstate(divide="ignore"):
        return x / T - np.log(-np.log(u))


def masses(x, temperature):
    """exp((x - x_max) / T) in float64 (0 for -inf)."""
    T = float(np.float32(temperature))
    with np.errstate(invalid="ignore"):
        return np.where(np.isneginf(x), 0.0, np.exp((x - x.max()) / T))


def threshold(x, temperature, top_k=0, top_p=1.0):
    """The smallest kept value of one row x (float64 [V], finite or -inf): -inf only when the row has no finite entry."""
    fin = x[np.isfinite(x)]
    if fin.size == 0:
        return -np.inf
    vals, counts = np.unique(fin, return_counts=True)           # ascending distinct values with exact counts
    vals, counts = vals[::-1], counts[::-1]
    t = vals[-1]
    if top_k and top_k > 0:
        t = vals[np.searchsorted(np.cumsum(counts), min(int(top_k), fin.size))]      # first value whose count from the top >= k
    if top_p < 1.0:
        keep = vals >= t
        v, n = vals[keep], counts[keep]
        T = float(np.float32(temperature))
        cum = np.cumsum(n * np.exp((v - vals[0]) / T))
        t = v[np.argmax(cum >= float(np.float32(top_p)) * cum[-1])]                   # the largest v whose mass from the top reaches p
    return float(t)


def sample_row(x, position, stream, seed, temperature, top_k=0, top_p=1.0):
    """(idx, top2_idx [2], top2_key [2], kept, threshold) of one row."""
    x = np.asarray(x, dtype=np.float64)
    thr = threshold(x, temperature, top_k, top_p)
    kept = (x >= thr) & (np.isfinite(x) if np.isfinite(thr) else True)
    key = gumbel_keys(x, position, stream, seed, temperature)
    masked = np.where(kept, key, -np.inf)
    first = int(np.argmax(masked)) if np.isfinite(thr) else 0     # ties (and the all -inf row) to the smaller column
    n = int(kept.sum())
    if n < 2:
        return first, (first, -1), (float(key[first]), -np.inf), n, thr
    masked2 = masked.copy()
    masked2[first] = -np.inf
    kept2 = kept.copy()
    kept2[first] = False
    second = int(np.argmax(np.where(kept2, masked2, -np.inf))) if np.isfinite(thr) else 1
    return first, (first, second), (float(key[first]), float(key[second])), n, thr


def sample_rows(logits, positions, sampling, streams=None, return_top2=False):
    """``longspec_amd.ops.sample_rows`` on CPU tensors."""
    shape = logits.shape[:-1]
    x = logits.reshape(-1, logits.shape[-1]).float().numpy().astype(np.float64)
    pos = positions.reshape(-1).to(torch.int64).numpy().copy()
    strm = streams.reshape(-1).numpy().copy() if streams is not None else np.zeros(len(pos), dtype=np.int64)
    assert len(pos) == x.shape[0] == len(strm)
    rows = [sample_row(x[r], pos[r], strm[r], sampling.seed, sampling.temperature, sampling.top_k, sampling.top_p)
            for r in range(x.shape[0])]
    idx = torch.tensor([r[0] for r in rows], dtype=torch.int64).view(shape)
    if not return_top2:
        return idx
    return (idx, torch.tensor([r[1] for r in rows], dtype=torch.int64).view(*shape, 2),
            torch.tensor([r[2] for r in rows], dtype=torch.float32).view(*shape, 2),
            torch.tensor([r[3] for r in rows], dtype=torch.int32).view(shape),
            torch.tensor([r[4] for r in rows], dtype=torch.float32).view(shape))


class Ops:
    """``tests/oracle_ops.py`` plus ``sample_rows``: the operator namespace of the sampled host-logic tests."""

    def __getattr__(self, name):
        return getattr(oracle_ops, name)

    sample_rows = staticmethod(sample_rows)


ops = Ops()
