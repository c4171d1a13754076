"""``ops.sample_rows`` with min_p / typical_p (``ls_sample_rows_ex``, csrc/sample_band.hip) against
tests/sampling_band_oracle.py: the band [threshold, upper], the draw inside it, the defining inequalities of the two filters on
EVERY row, the independence of a row's outputs from everything but that row, and the filters-off path bit for bit.

EPS_P = 2^-20 is the mass tolerance of test_gpu_sample_rows.py (integer weights F = floor(2^40 exp(.)): a cumulative mass over
V <= 2^18 logits is off by < 2^-22 of the total; 2^-20 leaves room for the float64 sums here).

DELTA = 2^-16 bounds the error of the kernel's distances d(v) = |a(v) - A|, a(v) = (max - v) / T, A = sum q a (the entropy minus
ln Z).  The kernel forms A = E / Z from Z = sum n F and E = sum n G, G(v) = floor(F(v) a(v)), as exact integers.  Against the
exact sums in units of 2^40: each F is short by < 1, which costs a(v) < 27.8 in E (F > 0 only where a < 40 ln 2); each G is short
by < 1 more; a logit with F = 0 is left out with a true term below 27.8; so |E - E_exact| <= 29 V 2^-40 relative to Z >= 1 (the
set holds the maximum) and |Z - Z_exact| <= V 2^-40, which moves the quotient by at most A V 2^-40 <= ln(V) V 2^-40.  Together
|A - A_exact| <= V 2^-40 (29 + ln V) < 2^-16.5 for V <= 2^18; a(v) itself and the T-scaled comparison are good to 2^-50 relative.
Nothing here is fitted to the kernel's output."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sampling_band_oracle as sbo
import sampling_oracle as so

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
TEMPS = (0.3, 1.0, 1.7)
GRID = ((0.05, 1.0, 0, 1.0), (0.5, 1.0, 0, 1.0), (1.0, 1.0, 0, 1.0), (0.0, 0.9, 0, 1.0), (0.0, 0.2, 0, 1.0),
        (0.02, 0.95, 50, 0.95))                                       # (min_p, typical_p, top_k, top_p)
EPS_P = 2.0 ** -20
DELTA = 2.0 ** -16
SHAPES = [(r, v) for v in (8, 504, 8192, 8200, 32000) for r in (1, 3, 69)] + [(5, 128256)]


def _sampling(T, k=0, p=1.0, min_p=0.0, typical_p=1.0, seed=SEED):
    return SimpleNamespace(temperature=T, top_k=k, top_p=p, seed=seed, min_p=min_p, typical_p=typical_p)


def _logits(rows, V, dtype, padded, device="cuda"):
    """The rows of test_gpu_sample_rows._logits (ties at the maximum and at the 50th value, -inf entries, a one-finite row, a
    no-finite row) plus, on every fifth row, one dominant token nine above the rest."""
    g = torch.Generator().manual_seed(rows * 1000003 + V)
    x = (torch.randn(rows, V, generator=g) * 3.0).to(dtype)
    for r in range(rows):
        if V >= 64:
            srt = x[r].float().sort(descending=True)
            if r % 2 == 0:
                x[r, srt.indices[1:3]] = float(srt.values[0])
            if r % 3 != 1 and V > 200:
                x[r, srt.indices[47:52]] = float(srt.values[49])
        if r % 4 != 2:
            x[r, torch.randperm(V, generator=g)[:max(1, V // 16)]] = -math.inf
        if r % 5 == 4:
            x[r, (7 * r) % V] = float(x[r].float().max()) + 9.0
    if rows >= 3:
        x[1] = -math.inf
        x[1, V // 2] = 1.5
        x[2] = -math.inf
    if not padded:
        return x.to(device)
    buf = torch.full((rows, V + 24), 60000.0 if dtype == torch.float16 else 1e30, dtype=dtype)
    buf[:, :V] = x
    return buf.to(device)[:, :V]


def _positions(rows):
    pos = torch.tensor([(1 << 33) + 12345 + 7 * r if r % 2 else 3 + r for r in range(rows)], dtype=torch.int64)
    return pos, torch.tensor([(r * 3) % 5 for r in range(rows)], dtype=torch.int32)


def _check(x, G, out, thr_kp, T, min_p, typ, what, seen):
    """x [rows, V] float64, G = ln(-ln u); out = (idx, top2_idx, top2_key, kept, threshold, upper) on the CPU; thr_kp [rows] =
    the threshold top_k / top_p alone leave (the set the two new filters start from)."""
    idx, t2i, t2k, kept, thr, upper = (o.numpy() for o in out)
    rows, V = x.shape
    T32, mp, tp = float(np.float32(T)), float(np.float32(min_p)), float(np.float32(typ))
    with np.errstate(invalid="ignore"):
        key = x / T32 - G
    for r in range(rows):
        fin = np.isfinite(x[r])
        if not fin.any():
            assert (idx[r], t2i[r, 1], kept[r]) == (0, 1 if V > 1 else -1, V), (what, r)
            assert np.isneginf(t2k[r]).all() and np.isneginf(thr[r]) and np.isneginf(upper[r]), (what, r)
            continue
        lo, hi, m = float(thr[r]), float(upper[r]), x[r][fin].max()
        km = (x[r] >= lo) & (x[r] <= hi)
        assert kept[r] == km.sum() and kept[r] >= 1, (what, r, kept[r], km.sum())
        assert x[r][km].min() == lo and x[r][km].max() == hi, (what, r)
        # the draw and the runner-up: the best keys of the band
        assert km[idx[r]] and t2i[r, 0] == idx[r], (what, r)
        kr = np.where(km, key[r], -np.inf)
        delta = 2.0 ** -20 * max(1.0, np.abs(key[r][fin]).max())
        assert key[r, idx[r]] >= kr.max() - delta and abs(float(t2k[r, 0]) - key[r, idx[r]]) <= delta, (what, r)
        if kept[r] == 1:
            assert t2i[r, 1] == -1 and np.isneginf(t2k[r, 1]), (what, r)
        else:
            j2 = t2i[r, 1]
            assert j2 != idx[r] and km[j2], (what, r)
            kr[idx[r]] = -np.inf
            assert key[r, j2] >= kr.max() - delta and abs(float(t2k[r, 1]) - key[r, j2]) <= delta, (what, r)
            assert t2k[r, 0] >= t2k[r, 1], (what, r)
        S = fin & (x[r] >= float(thr_kp[r]))                         # what top_k / top_p kept
        assert not (km & ~S).any(), (what, r)
        w = np.where(fin, np.exp((np.where(fin, x[r], 0.0) - m) / T32), 0.0)
        if mp > 0.0:
            assert (w[km] >= mp - EPS_P).all(), (what, r)
            if tp >= 1.0:
                assert (w[S & ~km] < mp + EPS_P).all(), (what, r)
                assert hi == m, (what, r)
            S = S & (w >= mp)
        if tp < 1.0:
            v, n = np.unique(x[r][S], return_counts=True)
            Z, H, dv = sbo.typical_distances(v, n, m, T32)
            d = np.full(V, np.inf)
            d[S] = dv[np.searchsorted(v, x[r][S])]
            assert S[km].all(), (what, r)
            D = d[km].max()
            assert w[km].sum() / Z >= tp - EPS_P, (what, r, w[km].sum() / Z)
            inner = S & (d < D - DELTA)
            assert w[inner].sum() / Z < tp + EPS_P, (what, r, w[inner].sum() / Z)
            assert km[inner].all(), (what, r)
            seen["max_kept" if hi == m else "max_dropped"] += 1


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("rows,V", SHAPES, ids=lambda v: str(v))
def test_band_filters_match_the_oracle(rows, V, dtype):
    from longspec_amd import ops
    padded = (rows + V // 8) % 2 == 1
    logits = _logits(rows, V, dtype, padded)
    assert logits.stride(0) == (V + 24 if padded else V)
    pos, strm = _positions(rows)
    x = logits.float().cpu().numpy().astype(np.float64)
    u = np.stack([so.uniforms(V, int(pos[r]), int(strm[r]), SEED) for r in range(rows)])
    G = np.log(-np.log(u))
    pos_d, strm_d = pos.cuda(), strm.cuda()
    seen = {"max_kept": 0, "max_dropped": 0}
    for T in TEMPS:
        for min_p, typ, k, p in GRID:
            s = _sampling(T, k, p, min_p, typ)
            what = f"rows={rows} V={V} {dtype} T={T} min_p={min_p} typical_p={typ} k={k} p={p}"
            out = [o.cpu() for o in ops.sample_rows(logits, pos_d, s, streams=strm_d, return_top2=True, return_upper=True)]
            again = [o.cpu() for o in ops.sample_rows(logits, pos_d, s, streams=strm_d, return_top2=True, return_upper=True)]
            for a, b in zip(out, again):
                assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                   b.view(torch.int32) if b.dtype == torch.float32 else b), what + ": two launches differ"
            assert torch.equal(ops.sample_rows(logits, pos_d, s, streams=strm_d).cpu(), out[0]), what
            thr_kp = ops.sample_rows(logits, pos_d, _sampling(T, k, p), streams=strm_d, return_top2=True)[4].cpu().numpy()
            _check(x, G, out, thr_kp, T, min_p, typ, what, seen)
    if rows >= 5:          # rows with a dominant token keep their maximum, broad rows lose it: both must have been exercised
        assert seen["max_kept"] > 0 and seen["max_dropped"] > 0, (rows, V, seen)


def test_the_kernel_agrees_with_the_oracle_band_on_a_small_row():
    """q = (1/2, 1/4, 1/8, 1/16, 4 x 1/64) as fp16 logits: the bands worked out in test_sampling_band_oracle.py."""
    from longspec_amd import ops
    x = torch.log(torch.tensor([[1 / 2, 1 / 4, 1 / 8, 1 / 16, 1 / 64, 1 / 64, 1 / 64, 1 / 64]], dtype=torch.float64)).to(torch.float16)
    pos = torch.tensor([11], dtype=torch.int64, device="cuda")
    xs = x[0].double().numpy()
    for kw, want in ((dict(typical_p=0.2), [1]), (dict(typical_p=0.9), [0, 1, 2, 3]), (dict(typical_p=0.95), list(range(8))),
                     (dict(min_p=0.1), [0, 1, 2, 3]), (dict(min_p=0.6), [0]),
                     (dict(k=4, p=0.9, min_p=0.2, typical_p=0.5), [0, 1])):
        s = _sampling(1.0, **kw)
        idx, t2i, t2k, kept, thr, upper = [o.cpu() for o in ops.sample_rows(x.cuda(), pos, s, return_top2=True, return_upper=True)]
        row = sbo.sample_row(xs, 11, 0, SEED, 1.0, s.top_k, s.top_p, s.min_p, s.typical_p)
        assert (float(thr), float(upper), int(kept)) == (xs[want].min(), xs[want].max(), len(want)), kw
        assert (int(idx), int(kept), float(thr), float(upper)) == (row[0], row[2], row[3], row[4]), kw


def _bits(outs):
    return [o.cpu().view(torch.int32) if o.dtype == torch.float32 else o.cpu() for o in outs]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("V", [8200, 128256])
def test_a_row_does_not_see_the_other_rows(V, dtype):
    """A row launched alone, among 68 others and in reversed row order: identical outputs, bit for bit; two launches too."""
    from longspec_amd import ops
    logits = _logits(69, V, dtype, padded=True)
    pos, strm = _positions(69)
    pos, strm = pos.cuda(), strm.cuda()
    rev = torch.arange(68, -1, -1, device="cuda")
    run = lambda l, p_, s_, s: _bits(ops.sample_rows(l, p_, s, streams=s_, return_top2=True, return_upper=True))
    for T, k, p, mp, tp in ((0.6, 50, 0.95, 0.02, 0.95), (1.0, 0, 1.0, 0.05, 0.9), (1.7, 0, 1.0, 0.0, 0.2)):
        s = _sampling(T, k, p, mp, tp)
        full = run(logits, pos, strm, s)
        for a, b in zip(full, run(logits, pos, strm, s)):
            assert torch.equal(a, b), (V, dtype, T, "two launches differ")
        for a, b in zip(full, run(logits[rev].contiguous(), pos[rev], strm[rev], s)):
            assert torch.equal(a, b.flip(0)), (V, dtype, T, k, p, mp, tp)
        for r in (0, 1, 2, 34, 68):
            for a, b in zip(full, run(logits[r:r + 1], pos[r:r + 1], strm[r:r + 1], s)):
                assert torch.equal(a[r:r + 1], b), (V, dtype, T, k, p, mp, tp, r)


def _call_ex(logits, pos, strm, T, k, p, min_p, typ, with_upper=True):
    """``ls_sample_rows_ex`` through ctypes, with a workspace of its own."""
    import ctypes
    from longspec_amd import _C
    lib = _C.load()
    n, V = logits.shape
    dev = logits.device
    out = torch.empty(n, dtype=torch.int64, device=dev)
    t2i = torch.empty((n, 2), dtype=torch.int64, device=dev)
    t2k = torch.empty((n, 2), dtype=torch.float32, device=dev)
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    thr = torch.empty(n, dtype=torch.float32, device=dev)
    upper = torch.empty(n, dtype=torch.float32, device=dev) if with_upper else None
    d = _C.SampleDesc(logits=logits.data_ptr(), positions=pos.data_ptr(), streams=strm.data_ptr(), out_idx=out.data_ptr(),
                      out_top2_idx=t2i.data_ptr(), out_top2_key=t2k.data_ptr(), out_kept=kept.data_ptr(),
                      out_threshold=thr.data_ptr(), out_upper=upper.data_ptr() if with_upper else None, ld=logits.stride(0),
                      seed=SEED, rows=n, vocab=V, dtype=_C.LS_F16 if logits.dtype == torch.float16 else _C.LS_BF16, top_k=k,
                      temperature=T, top_p=p, min_p=min_p, typical_p=typ)
    need = lib.ls_sample_ex_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    rc = lib.ls_sample_rows_ex(ctypes.byref(d), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, need, (out, t2i, t2k, kept, thr), upper


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_filters_off_is_ls_sample_rows_bit_for_bit(dtype):
    from longspec_amd import _C, ops
    lib = _C.load()
    rows, V = 69, 8200
    logits = _logits(rows, V, dtype, padded=True)
    pos, strm = _positions(rows)
    pos, strm = pos.cuda(), strm.cuda()
    for T, k, p in ((0.6, 50, 0.95), (1.0, 0, 1.0), (1.7, 0, 0.9), (0.3, 7, 1.0)):
        rc, need, ex, upper = _call_ex(logits, pos, strm, T, k, p, 0.0, 1.0)
        assert rc == 0 and need == lib.ls_sample_workspace_bytes(rows, V)
        old = [torch.empty_like(o) for o in ex]
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        assert lib.ls_sample_rows(logits.data_ptr(), rows, V, logits.stride(0), _C.LS_F16 if dtype == torch.float16 else _C.LS_BF16,
                                  pos.data_ptr(), strm.data_ptr(), SEED, T, k, p, *[o.data_ptr() for o in old], ws.data_ptr(),
                                  ws.numel(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        via_ops = ops.sample_rows(logits, pos, _sampling(T, k, p), streams=strm, return_top2=True)
        plain = ops.sample_rows(logits, pos, SimpleNamespace(temperature=T, top_k=k, top_p=p, seed=SEED), streams=strm,
                                return_top2=True)                    # an object without the new attributes
        with_upper = ops.sample_rows(logits, pos, _sampling(T, k, p), streams=strm, return_top2=True, return_upper=True)
        for a, b, c, e, f in zip(_bits(ex), _bits(old), _bits(via_ops), _bits(plain), _bits(with_upper[:5])):
            assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, e) and torch.equal(a, f), (dtype, T, k, p)
        # upper with the filters off: the row maximum (-inf without a finite logit)
        x = logits.float()
        want = torch.where(torch.isfinite(x).any(dim=1), x.max(dim=1).values, torch.full((rows,), -math.inf, device="cuda"))
        assert torch.equal(upper, want) and torch.equal(with_upper[5], want)


def test_bad_arguments_are_refused():
    from longspec_amd import _C, ops
    from longspec_amd._C import LongSpecHipError
    pos = torch.zeros(2, dtype=torch.int64, device="cuda")
    strm = torch.zeros(2, dtype=torch.int32, device="cuda")
    ok = torch.zeros(2, 16, dtype=torch.float16, device="cuda")
    for bad in (dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=float("nan")), dict(typical_p=0.0), dict(typical_p=-0.5),
                dict(typical_p=1.5), dict(typical_p=float("nan"))):
        with pytest.raises(LongSpecHipError, match="min_p"):
            ops.sample_rows(ok, pos, _sampling(1.0, **bad))
        kw = dict(min_p=0.0, typ=1.0)
        kw.update({("typ" if n == "typical_p" else n): v for n, v in bad.items()})
        assert _call_ex(ok, pos, strm, 1.0, 0, 1.0, kw["min_p"], kw["typ"])[0] == _C.LS_ERR_INVALID_ARG
    # the old checks hold on the new entry point
    for T, k, p in ((0.0, 0, 1.0), (1.0, -1, 1.0), (1.0, 0, 0.0), (1.0, 0, 1.5)):
        with pytest.raises(LongSpecHipError):
            ops.sample_rows(ok, pos, _sampling(T, k, p, 0.1, 0.9))
    with pytest.raises(LongSpecHipError):
        ops.sample_rows(torch.zeros(2, 12, dtype=torch.float16, device="cuda"), pos, _sampling(1.0, min_p=0.1))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.sample_rows(ok.cpu(), pos.cpu(), _sampling(1.0, min_p=0.1))
    # a workspace without the typical_p tables is refused, not overrun
    d_small = _C.load().ls_sample_workspace_bytes(2, 16)
    import ctypes
    out = torch.empty(2, dtype=torch.int64, device="cuda")
    d = _C.SampleDesc(logits=ok.data_ptr(), positions=pos.data_ptr(), streams=None, out_idx=out.data_ptr(), ld=16, seed=1, rows=2,
                      vocab=16, dtype=_C.LS_F16, top_k=0, temperature=1.0, top_p=1.0, min_p=0.0, typical_p=0.5)
    ws = torch.empty(d_small, dtype=torch.uint8, device="cuda")
    assert _C.load().ls_sample_rows_ex(ctypes.byref(d), ws.data_ptr(), ws.numel(), None) == _C.LS_ERR_WORKSPACE
