"""``ops.sample_rows`` (csrc/sample.hip) against tests/sampling_oracle.py: the draw, the kept set, the thresholds of top-k
and top-p, and the independence of a row's outputs from everything but that row."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sampling_oracle as so

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
TEMPS = (0.3, 1.0, 1.7)
FILTERS = ((0, 1.0), (1, 1.0), (50, 1.0), (0, 0.9), (50, 0.95), (0, 1e-6))          # (top_k, top_p)
# top-p: the kernel sums F(x) = floor(2^40 exp((x - x_max) / T)) (double-precision exp) as exact integers.  Per logit
# |F / 2^40 - mass| <= 2^-40 (+ 2^-52 relative from exp and the division), the kept mass is >= 1 (the maximum's), so a
# cumulative mass over <= V logits is off by <= V 2^-40 relative to the total, and the target ceil(p * total) adds 2^-40:
# below 2^-22 for V <= 2^18.  DESIGN.md "Sampled decoding" has the derivation; 2^-20 leaves room for the oracle's own sums.
EPS_P = 2.0 ** -20
SHAPES = [(r, v) for v in (8, 504, 8192, 8200, 32000) for r in (1, 3, 69, 128)] + [(r, v) for v in (128256, 152064) for r in (1, 5)]


def _sampling(T, k, p, seed=SEED):
    return SimpleNamespace(temperature=T, top_k=k, top_p=p, seed=seed)


def _logits(rows, V, dtype, padded, device="cuda"):
    """[rows, V] view (row stride V + 24 when padded, the padding filled with a value that would win every draw) with exact
    ties at the maximum and at the 50th value, -inf entries, a row with one finite entry and a row without any."""
    g = torch.Generator().manual_seed(rows * 1000003 + V)
    x = (torch.randn(rows, V, generator=g) * 3.0).to(dtype)
    for r in range(rows):
        if V >= 64:
            srt = x[r].float().sort(descending=True)
            if r % 2 == 0:                                  # three maxima
                x[r, srt.indices[1:3]] = float(srt.values[0])
            if r % 3 != 1 and V > 200:                      # the 50th value five times: ranks 48..52
                x[r, srt.indices[47:52]] = float(srt.values[49])
        if r % 4 != 2:
            x[r, torch.randperm(V, generator=g)[:max(1, V // 16)]] = -math.inf
    if rows >= 3:
        x[1] = -math.inf
        x[1, V // 2] = 1.5                                  # one finite entry
        x[2] = -math.inf                                    # none
    if not padded:
        return x.to(device)
    buf = torch.full((rows, V + 24), 60000.0 if dtype == torch.float16 else 1e30, dtype=dtype)
    buf[:, :V] = x
    return buf.to(device)[:, :V]


def _positions(rows):
    pos = torch.tensor([(1 << 33) + 12345 + 7 * r if r % 2 else 3 + r for r in range(rows)], dtype=torch.int64)
    return pos, torch.tensor([(r * 3) % 5 for r in range(rows)], dtype=torch.int32)


def _check(x, G, out, T, k, p, what):
    """x [rows, V] float64, G = ln(-ln u) [rows, V]; out = the five outputs on the CPU."""
    idx, t2i, t2k, kept, thr = (o.numpy() for o in out)
    rows, V = x.shape
    T32 = float(np.float32(T))
    with np.errstate(invalid="ignore"):
        key = x / T32 - G
    fin = np.isfinite(x)
    any_fin = fin.any(axis=1)
    thr64 = thr.astype(np.float64)
    km = x >= thr64[:, None]
    assert np.array_equal(np.isfinite(thr64), any_fin), what
    assert np.array_equal(kept, km.sum(axis=1)), (what, kept, km.sum(axis=1))
    assert km[np.arange(rows), idx].all(), what
    assert np.array_equal(t2i[:, 0], idx), what
    # the k-th largest finite value (the smallest finite one when there are fewer, or no top-k)
    xs = np.sort(np.where(fin, x, -np.inf), axis=1)[:, ::-1]
    n_fin = fin.sum(axis=1)
    kk = np.minimum(k if k > 0 else V, np.maximum(n_fin, 1))
    t_k = xs[np.arange(rows), kk - 1]
    if p >= 1.0:
        assert np.array_equal(thr64, t_k), (what, thr64, t_k)
    for r in range(rows):
        if not any_fin[r]:
            assert (idx[r], t2i[r, 1], kept[r]) == (0, 1 if V > 1 else -1, V), what
            assert np.isneginf(t2k[r]).all(), what
            continue
        kr = np.where(km[r], key[r], -np.inf)
        delta = 2.0 ** -20 * max(1.0, np.abs(key[r][fin[r]]).max())
        best = kr.max()
        assert key[r, idx[r]] >= best - delta, (what, r, key[r, idx[r]], best, delta)
        assert abs(float(t2k[r, 0]) - key[r, idx[r]]) <= delta, (what, r)
        if kept[r] == 1:
            assert t2i[r, 1] == -1 and np.isneginf(t2k[r, 1]), (what, r)
        else:
            j2 = t2i[r, 1]
            assert j2 != idx[r] and km[r, j2], (what, r)
            kr[idx[r]] = -np.inf
            assert key[r, j2] >= kr.max() - delta and abs(float(t2k[r, 1]) - key[r, j2]) <= delta, (what, r)
            assert t2k[r, 0] >= t2k[r, 1], (what, r)
        if p < 1.0:
            assert thr64[r] >= t_k[r], (what, r)
            base = x[r] >= t_k[r]
            mass = np.where(base, np.exp((np.where(base, x[r], 0.0) - xs[r, 0]) / T32), 0.0)
            total = mass.sum()
            p32 = float(np.float32(p))
            assert mass[x[r] > thr64[r]].sum() / total < p32 + EPS_P, (what, r)
            assert mass[x[r] >= thr64[r]].sum() / total >= p32 - EPS_P, (what, r)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("rows,V", SHAPES, ids=lambda v: str(v))
def test_sample_rows_matches_the_oracle(rows, V, dtype):
    from longspec_amd import ops
    padded = (rows + V // 8) % 2 == 1
    logits = _logits(rows, V, dtype, padded)
    assert logits.stride(0) == (V + 24 if padded else V)
    pos, strm = _positions(rows)
    x = logits.float().cpu().numpy().astype(np.float64)
    u = np.stack([so.uniforms(V, int(pos[r]), int(strm[r]), SEED) for r in range(rows)])
    G = np.log(-np.log(u))
    pos_d, strm_d = pos.cuda(), strm.cuda()
    for T in TEMPS:
        for k, p in FILTERS:
            s = _sampling(T, k, p)
            out = [o.cpu() for o in ops.sample_rows(logits, pos_d, s, streams=strm_d, return_top2=True)]
            again = [o.cpu() for o in ops.sample_rows(logits, pos_d, s, streams=strm_d, return_top2=True)]
            what = f"rows={rows} V={V} {dtype} T={T} k={k} p={p}"
            for a, b in zip(out, again):
                assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                   b.view(torch.int32) if b.dtype == torch.float32 else b), what + ": two launches differ"
            assert torch.equal(ops.sample_rows(logits, pos_d, s, streams=strm_d).cpu(), out[0]), what
            _check(x, G, out, T, k, p, what)


def _bits(outs):
    return [o.cpu().view(torch.int32) if o.dtype == torch.float32 else o.cpu() for o in outs]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("V", [8200, 32000, 128256])
def test_a_row_does_not_see_the_other_rows(V, dtype):
    """A row launched alone, among 68 others and in reversed row order: identical outputs, bit for bit."""
    from longspec_amd import ops
    logits = _logits(69, V, dtype, padded=True)
    pos, strm = _positions(69)
    pos, strm = pos.cuda(), strm.cuda()
    rev = torch.arange(68, -1, -1, device="cuda")
    for T, k, p in ((0.6, 50, 0.95), (1.7, 0, 1.0), (1.0, 0, 0.9)):
        s = _sampling(T, k, p)
        full = _bits(ops.sample_rows(logits, pos, s, streams=strm, return_top2=True))
        flipped = _bits(ops.sample_rows(logits[rev].contiguous(), pos[rev], s, streams=strm[rev], return_top2=True))
        for a, b in zip(full, flipped):
            assert torch.equal(a, b.flip(0)), (V, dtype, T, k, p)
        for r in (0, 1, 2, 33, 68):
            alone = _bits(ops.sample_rows(logits[r:r + 1], pos[r:r + 1], s, streams=strm[r:r + 1], return_top2=True))
            for a, b in zip(full, alone):
                assert torch.equal(a[r:r + 1], b), (V, dtype, T, k, p, r)


def test_streams_default_to_zero_and_change_the_draw():
    from longspec_amd import ops
    logits = _logits(5, 8192, torch.float16, padded=False)
    pos = torch.full((5,), 77, dtype=torch.int64, device="cuda")
    s = _sampling(1.0, 0, 1.0)
    none = ops.sample_rows(logits, pos, s)
    assert torch.equal(none, ops.sample_rows(logits, pos, s, streams=torch.zeros(5, dtype=torch.int32, device="cuda")))
    x = logits.float().cpu().numpy().astype(np.float64)
    for strm in (0, 4):
        got = ops.sample_rows(logits, pos, s, streams=torch.full((5,), strm, dtype=torch.int32, device="cuda")).cpu()
        want = [so.sample_row(x[r], 77, strm, SEED, 1.0)[0] for r in range(5)]
        assert got.tolist() == want
    # leading dimensions are kept: [bsz, rows, V] with [bsz, rows] positions
    l3 = logits[:4].reshape(2, 2, 8192)
    assert torch.equal(ops.sample_rows(l3, pos[:4].view(2, 2), s), none[:4].view(2, 2))


def test_bad_arguments_are_refused():
    from longspec_amd import ops
    from longspec_amd._C import LongSpecHipError
    pos = torch.zeros(2, dtype=torch.int64, device="cuda")
    with pytest.raises(LongSpecHipError):
        ops.sample_rows(torch.zeros(2, 12, dtype=torch.float16, device="cuda"), pos, _sampling(1.0, 0, 1.0))
    ok = torch.zeros(2, 16, dtype=torch.float16, device="cuda")
    for bad in (_sampling(0.0, 0, 1.0), _sampling(1.0, -1, 1.0), _sampling(1.0, 0, 0.0), _sampling(1.0, 0, 1.5)):
        with pytest.raises(LongSpecHipError):
            ops.sample_rows(ok, pos, bad)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.sample_rows(ok.cpu(), pos.cpu(), _sampling(1.0, 0, 1.0))
