"""``ops.sample_rows`` with ``cut=`` (``ls_sample_rows_cut``, csrc/sample_cut.hip) against tests/sampling_cut_oracle.py: the
defining inequalities of top_n_sigma and xtc on EVERY row, the coin bit for bit, the independence of a row's outputs from
everything but that row, and the filters-off path bit for bit.

DELTA_SIGMA = 2^-20 (1 + n sigma_ref) bounds the error of the kernel's threshold t = m - n sigma: its double sums over V <= 2^24
shifted terms y = x - m carry a relative error below 2^-29; the bound leaves 2^9 over that and is still far below the 16-bit
spacing of any realistic logit.  No case is excluded.

EPS = 2^-20 is the mass tolerance of test_gpu_sample_rows.py (integer weights F = floor(2^40 exp(.)): a mass over V <= 2^18
logits is off by < 2^-22 of the total; 2^-20 leaves room for the float64 sums here).  Nothing here is fitted to the kernel's
output."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sampling_cut_oracle as sco
from longspec_amd import Cut

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
TEMPS = (0.3, 1.0, 1.5)
EPS = 2.0 ** -20
# (top_n_sigma, xtc P, xtc theta, top_k, top_p, min_p, typical_p)
CONFIGS = ((1.0, 0.0, 0.1, 0, 1.0, 0.0, 1.0), (2.5, 0.0, 0.1, 50, 0.9, 0.0, 1.0), (0.0, 0.5, 0.1, 0, 1.0, 0.0, 1.0),
           (0.0, 1.0, 0.02, 50, 0.95, 0.0, 1.0), (3.0, 1.0, 0.05, 50, 0.95, 0.02, 0.95), (1e-6, 0.5, 0.5, 0, 1.0, 0.0, 1.0))
SHAPES = [(r, v) for v in (8, 1000, 8192, 8200, 128256) for r in (1, 3, 69)]


def _sampling(T, k=0, p=1.0, min_p=0.0, typical_p=1.0, seed=SEED):
    return SimpleNamespace(temperature=T, top_k=k, top_p=p, seed=seed, min_p=min_p, typical_p=typical_p)


def _logits(rows, V, dtype, padded, device="cuda"):
    """Random rows with ties at the maximum and at the 50th value, -inf entries and, on every fifth row, one dominant token;
    from three rows on a row with one finite logit and a row without any; from five on an all-equal row and a row whose
    second value is held by three tokens (the ties at v* of xtc)."""
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
    if rows >= 5:
        x[3] = -2.25
        x[4] = (torch.randn(V, generator=g) * 0.25 - 3.0).to(dtype)
        x[4, 0] = 5.0
        x[4, torch.tensor([1, V // 2, V - 1])] = 4.0
    if not padded:
        return x.to(device)
    buf = torch.full((rows, V + 24), 60000.0 if dtype == torch.float16 else 1e30, dtype=dtype)
    buf[:, :V] = x
    return buf.to(device)[:, :V]


def _positions(rows):
    pos = torch.tensor([(1 << 33) + 12345 + 7 * r if r % 2 else 3 + r for r in range(rows)], dtype=torch.int64)
    return pos, torch.tensor([(r * 3) % 5 for r in range(rows)], dtype=torch.int32)


def _bits(outs):
    return [o.cpu().view(torch.int32) if o.dtype == torch.float32 else o.cpu() for o in outs]


def _run(ops, logits, pos, strm, T, cfg):
    n, P, theta, k, p, mp, tp = cfg
    return ops.sample_rows(logits, pos, _sampling(T, k, p, mp, tp), streams=strm, return_top2=True, return_upper=True,
                           cut=Cut(n, P, theta))


def _band_ok(x, out, what):
    """The outputs describe a band of the row's values and the draw lies inside it."""
    idx, t2i, t2k, kept, thr, upper = out
    for r in range(x.shape[0]):
        fin = np.isfinite(x[r])
        if not fin.any():
            assert (idx[r], kept[r]) == (0, x.shape[1]) and np.isneginf(thr[r]) and np.isneginf(upper[r]), (what, r)
            continue
        km = (x[r] >= thr[r]) & (x[r] <= upper[r])
        assert kept[r] == km.sum() and kept[r] >= 1, (what, r, kept[r], km.sum())
        assert x[r][km].min() == thr[r] and x[r][km].max() == upper[r], (what, r)
        assert km[idx[r]] and t2i[r, 0] == idx[r] and thr[r] <= x[r, idx[r]] <= upper[r], (what, r)
        assert (t2i[r, 1] == -1) == (kept[r] == 1) and (kept[r] == 1 or km[t2i[r, 1]]), (what, r)


def _check_sigma(x, n, sig, front, both, what):
    """sig: the outputs with top_n_sigma alone; front: with top_k alone; both: with top_n_sigma and top_k."""
    n32 = float(np.float32(n))
    for r in range(x.shape[0]):
        fin = np.isfinite(x[r])
        if not fin.any():
            continue
        sigma, t = sco.sigma_threshold(x[r], n)
        delta = 2.0 ** -20 * (1.0 + n32 * sigma)
        km = (x[r] >= sig[4][r]) & (x[r] <= sig[5][r])
        assert km[fin & (x[r] >= t + delta)].all(), (what, r, "a logit above the threshold was dropped")
        assert not km[fin & (x[r] < t - delta)].any(), (what, r, "a logit below the threshold was kept")
        assert sig[5][r] == x[r][fin].max(), (what, r)
        # a threshold set that holds the maximum: it intersects with top_k
        assert both[4][r] == max(sig[4][r], front[4][r]) and both[5][r] == sig[5][r], (what, r)


def _check_top_p_over_both(x, T, p, both, full, what):
    """both: top_n_sigma and top_k; full: the same and top_p, whose mass is taken over what both kept."""
    T32, p32 = float(np.float32(T)), float(np.float32(p))
    for r in range(x.shape[0]):
        fin = np.isfinite(x[r])
        if not fin.any():
            continue
        S = fin & (x[r] >= both[4][r])
        w = np.where(S, np.exp((np.where(fin, x[r], 0.0) - x[r][fin].max()) / T32), 0.0)
        km = fin & (x[r] >= full[4][r])
        assert not (km & ~S).any() and w[km].sum() / w.sum() >= p32 - EPS, (what, r)
        assert w[S & (x[r] > full[4][r])].sum() / w.sum() < p32 + EPS, (what, r)


def _check_xtc(x, pos, strm, T, P, theta, off, on, what, seen):
    """off: the outputs of the same call with P = 0 (its band is S); on: with the coin."""
    T32, th = float(np.float32(T)), float(np.float32(theta))
    off_b, on_b = (_bits([torch.from_numpy(np.ascontiguousarray(o)) for o in outs]) for outs in (off, on))
    for r in range(x.shape[0]):
        fin = np.isfinite(x[r])
        if not sco.fires(SEED, int(pos[r]), int(strm[r]), P) or not fin.any():
            for a, b in zip(off_b, on_b):
                assert torch.equal(a[r], b[r]), (what, r, "the coin did not fire and an output differs from P = 0")
            continue
        seen["fired"] += 1
        lo, hi, up = off[4][r], off[5][r], on[5][r]
        S = fin & (x[r] >= lo) & (x[r] <= hi)
        assert on[4][r] == lo and lo <= up <= hi and (x[r][S] == up).any(), (what, r, "out_upper does not occur in S")
        w = np.where(S, np.exp((np.where(fin, x[r], 0.0) - x[r][fin].max()) / T32), 0.0)
        q = w / w.sum()
        assert (q[S & (x[r] > up)] >= th - EPS).all(), (what, r, "a dropped value is below the threshold")
        if up < hi:
            seen["cut"] += 1
            assert q[S & (x[r] == up)].min() >= th - EPS, (what, r, "the cut value is below the threshold")
        assert not (q[S & (x[r] < up)] >= th + EPS).any(), (what, r, "a smaller value of S reaches the threshold")
        assert on[3][r] == (S & (x[r] <= up)).sum(), (what, r)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("rows,V", SHAPES, ids=lambda v: str(v))
def test_cuts_match_the_oracle(rows, V, dtype):
    from longspec_amd import ops
    padded = (rows + V // 8) % 2 == 1 or V == 128256
    logits = _logits(rows, V, dtype, padded)
    assert logits.stride(0) == (V + 24 if padded else V)
    pos, strm = _positions(rows)
    x = logits.float().cpu().numpy().astype(np.float64)
    pos_d, strm_d = pos.cuda(), strm.cuda()
    seen = {"fired": 0, "cut": 0}
    run = lambda T, cfg: [o.cpu().numpy() for o in _run(ops, logits, pos_d, strm_d, T, cfg)]
    for cfg in CONFIGS:
        for T in TEMPS:
            n, P, theta, k, p, mp, tp = cfg
            what = f"rows={rows} V={V} {dtype} T={T} cut=({n}, {P}, {theta}) k={k} p={p} min_p={mp} typical_p={tp}"
            out = run(T, cfg)
            _band_ok(x, out, what)
            if n > 0.0:
                sig, front = run(T, (n, 0.0, 0.1, 0, 1.0, 0.0, 1.0)), run(T, (0.0, 0.0, 0.1, k, 1.0, 0.0, 1.0))
                both = run(T, (n, 0.0, 0.1, k, 1.0, 0.0, 1.0))
                _check_sigma(x, n, sig, front, both, what)
                if p < 1.0:
                    _check_top_p_over_both(x, T, p, both, run(T, (n, 0.0, 0.1, k, p, 0.0, 1.0)), what)
            if P > 0.0:
                _check_xtc(x, pos, strm, T, P, theta, run(T, (n, 0.0, theta, k, p, mp, tp)), out, what, seen)
    if rows >= 5:
        assert seen["fired"] > 0 and seen["cut"] > 0, (rows, V, seen)


def test_special_rows_by_hand():
    """An all-equal row, a one-finite row, an all -inf row and the row with three tokens tied at v*, against the oracle's band."""
    from longspec_amd import ops
    logits = _logits(5, 1000, torch.float16, padded=False)
    x = logits.float().cpu().numpy().astype(np.float64)
    pos = torch.full((5,), 77, dtype=torch.int64, device="cuda")
    assert sco.fires(SEED, 77, 0, 1.0)
    for cut in (Cut(1.0), Cut(0.0, 1.0, 0.1), Cut(2.0, 1.0, 0.1), Cut(1e-6)):
        idx, t2i, t2k, kept, thr, upper = [o.cpu().numpy() for o in ops.sample_rows(logits, pos, _sampling(1.0), return_top2=True,
                                                                                    return_upper=True, cut=cut)]
        for r in (1, 2, 3, 4):
            row = sco.sample_row(x[r], 77, 0, SEED, 1.0, cut=cut)
            assert (int(kept[r]), float(thr[r]), float(upper[r])) == (row[2], row[3], row[4]), (cut, r)
        assert (kept[1], kept[2], kept[3]) == (1, 1000, 1000) and thr[3] == upper[3] == -2.25
    kept, thr, upper = [o.cpu().numpy() for o in ops.sample_rows(logits, pos, _sampling(1.0), return_top2=True, return_upper=True,
                                                                 cut=Cut(0.0, 1.0, 0.1))[3:]]
    assert kept[4] == 999 and upper[4] == 4.0 and thr[4] == x[4].min()               # the maximum goes, the three ties stay


def test_the_coin_fires_where_the_oracle_says():
    """One row content at 2048 positions, two dominant tokens (shares 0.65 and 0.24 at T = 1, theta = 0.1: the cut takes the
    maximum wherever the coin fires).  P = 0.5: the fired pattern is the oracle's, exactly.  P = 1: the maximum is never drawn."""
    from longspec_amd import ops
    g = torch.Generator().manual_seed(9)
    row = (torch.randn(64, generator=g) * 0.5).half()
    row[0], row[1] = 6.0, 5.0
    logits = row.view(1, 64).repeat(2048, 1).cuda()
    pos = torch.arange(2048, dtype=torch.int64, device="cuda")
    for stream in (0, 3):
        strm = torch.full((2048,), stream, dtype=torch.int32, device="cuda") if stream else None
        idx, _, _, kept, thr, upper = [o.cpu() for o in ops.sample_rows(logits, pos, _sampling(1.0), streams=strm, return_top2=True,
                                                                        return_upper=True, cut=Cut(0.0, 0.5, 0.1))]
        want = torch.tensor([sco.fires(SEED, p, stream, 0.5) for p in range(2048)])
        assert torch.equal(upper == 5.0, want) and torch.equal(upper == 6.0, ~want) and torch.equal(kept == 63, want)
        assert abs(int(want.sum()) - 1024) <= 5 * math.sqrt(2048 * 0.25)
        assert not (idx[want] == 0).any() and (idx[~want] == 0).any()
    idx, _, _, kept, thr, upper = [o.cpu() for o in ops.sample_rows(logits, pos, _sampling(1.0), return_top2=True, return_upper=True,
                                                                    cut=Cut(0.0, 1.0, 0.1))]
    assert not (idx == 0).any() and (upper == 5.0).all() and (kept == 63).all() and (idx == 1).sum() > 1024


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("V", [8200, 128256])
def test_a_row_does_not_see_the_other_rows(V, dtype):
    """A row launched alone, among 68 others and in reversed row order: identical outputs, bit for bit; two launches too."""
    from longspec_amd import ops
    logits = _logits(69, V, dtype, padded=True)
    pos, strm = _positions(69)
    pos, strm = pos.cuda(), strm.cuda()
    rev = torch.arange(68, -1, -1, device="cuda")
    for T, cfg in ((0.6, CONFIGS[4]), (1.0, CONFIGS[0]), (1.5, (0.0, 0.5, 0.02, 0, 1.0, 0.0, 1.0))):
        run = lambda l, p_, s_: _bits(_run(ops, l, p_, s_, T, cfg))
        full = run(logits, pos, strm)
        for a, b in zip(full, run(logits, pos, strm)):
            assert torch.equal(a, b), (V, dtype, T, "two launches differ")
        for a, b in zip(full, run(logits[rev].contiguous(), pos[rev], strm[rev])):
            assert torch.equal(a, b.flip(0)), (V, dtype, T, cfg)
        for r in (0, 1, 2, 3, 4, 34, 68):
            for a, b in zip(full, run(logits[r:r + 1], pos[r:r + 1], strm[r:r + 1])):
                assert torch.equal(a[r:r + 1], b), (V, dtype, T, cfg, r)


def _call(logits, pos, strm, T, k, p, min_p, typ, cut="ex"):
    """``ls_sample_rows_ex`` (cut = "ex") or ``ls_sample_rows_cut`` (cut = None: a NULL pointer, or (n, P, theta, reserved))
    through ctypes, with a workspace of its own."""
    from longspec_amd import _C
    lib = _C.load()
    n, V = logits.shape
    dev = logits.device
    outs = (torch.empty(n, dtype=torch.int64, device=dev), torch.empty((n, 2), dtype=torch.int64, device=dev),
            torch.empty((n, 2), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
            torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev))
    d = _C.SampleDesc(logits=logits.data_ptr(), positions=pos.data_ptr(), streams=strm.data_ptr(), out_idx=outs[0].data_ptr(),
                      out_top2_idx=outs[1].data_ptr(), out_top2_key=outs[2].data_ptr(), out_kept=outs[3].data_ptr(),
                      out_threshold=outs[4].data_ptr(), out_upper=outs[5].data_ptr(), ld=logits.stride(0), seed=SEED, rows=n,
                      vocab=V, dtype=_C.LS_F16 if logits.dtype == torch.float16 else _C.LS_BF16, top_k=k, temperature=T, top_p=p,
                      min_p=min_p, typical_p=typ)
    stream = torch.cuda.current_stream().cuda_stream
    if cut == "ex":
        need = lib.ls_sample_ex_workspace_bytes(ctypes.byref(d))
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        rc = lib.ls_sample_rows_ex(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream)
    else:
        c = _C.SampleCut(*cut) if cut is not None else None
        cp = ctypes.byref(c) if c is not None else None
        need = lib.ls_sample_cut_workspace_bytes(ctypes.byref(d), cp)
        assert need == lib.ls_sample_ex_workspace_bytes(ctypes.byref(d))
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        rc = lib.ls_sample_rows_cut(ctypes.byref(d), cp, ws.data_ptr(), ws.numel(), stream)
    torch.cuda.synchronize()
    return rc, outs


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_cut_off_is_ls_sample_rows_ex_bit_for_bit(dtype):
    """A NULL cut pointer, and a cut with both filters off (whatever its threshold), against ``ls_sample_rows_ex``; and
    ``ops.sample_rows`` with ``cut=None`` and with an idle ``Cut``."""
    from longspec_amd import ops
    rows, V = 69, 8200
    logits = _logits(rows, V, dtype, padded=True)
    pos, strm = _positions(rows)
    pos, strm = pos.cuda(), strm.cuda()
    for T, k, p, mp, tp in ((0.6, 50, 0.95, 0.0, 1.0), (1.0, 0, 1.0, 0.0, 1.0), (1.5, 0, 0.9, 0.05, 0.9), (0.3, 7, 1.0, 0.0, 0.5)):
        rc, ex = _call(logits, pos, strm, T, k, p, mp, tp)
        assert rc == 0
        for cut in (None, (0.0, 0.0, 0.1, 0), (0.0, 0.0, 1.0, 0)):
            rc, got = _call(logits, pos, strm, T, k, p, mp, tp, cut=cut)
            assert rc == 0
            for a, b in zip(_bits(ex), _bits(got)):
                assert torch.equal(a, b), (dtype, T, k, p, mp, tp, cut)
        s = _sampling(T, k, p, mp, tp)
        for cut in (None, Cut(), Cut(xtc_threshold=0.7)):
            via = ops.sample_rows(logits, pos, s, streams=strm, return_top2=True, return_upper=True, cut=cut)
            for a, b in zip(_bits(ex), _bits(via)):
                assert torch.equal(a, b), (dtype, T, k, p, mp, tp, cut)
        # and a cut that is on does change rows
        rc, got = _call(logits, pos, strm, T, k, p, mp, tp, cut=(1.0, 1.0, 0.01, 0))
        assert rc == 0 and not torch.equal(got[3], ex[3])


def test_bad_arguments_are_refused():
    from longspec_amd import _C
    pos = torch.zeros(2, dtype=torch.int64, device="cuda")
    strm = torch.zeros(2, dtype=torch.int32, device="cuda")
    ok = torch.zeros(2, 16, dtype=torch.float16, device="cuda")
    nan, inf = math.nan, math.inf
    assert _call(ok, pos, strm, 1.0, 0, 1.0, 0.0, 1.0, cut=(1.0, 1.0, 1.0, 0))[0] == 0
    for bad in ((-0.5, 0.0, 0.1, 0), (inf, 0.0, 0.1, 0), (nan, 0.0, 0.1, 0), (0.0, -0.1, 0.1, 0), (0.0, 1.5, 0.1, 0), (0.0, nan, 0.1, 0),
                (0.0, 0.5, 0.0, 0), (0.0, 0.5, -0.1, 0), (0.0, 0.5, 1.5, 0), (0.0, 0.5, nan, 0), (0.0, 0.0, 0.0, 0), (1.0, 0.0, nan, 0),
                (1.0, 0.5, 0.1, 1), (0.0, 0.0, 0.1, -1)):
        rc, outs = _call(ok, pos, strm, 1.0, 0, 1.0, 0.0, 1.0, cut=bad)
        assert rc == _C.LS_ERR_INVALID_ARG, bad
    # the old checks hold on the new entry point
    for T, k, p, mp, tp in ((0.0, 0, 1.0, 0.0, 1.0), (1.0, -1, 1.0, 0.0, 1.0), (1.0, 0, 0.0, 0.0, 1.0), (1.0, 0, 1.0, 1.5, 1.0),
                            (1.0, 0, 1.0, 0.0, 0.0)):
        assert _call(ok, pos, strm, T, k, p, mp, tp, cut=(1.0, 0.5, 0.1, 0))[0] == _C.LS_ERR_INVALID_ARG
    assert _C.load().ls_sample_rows_cut(None, None, None, 0, None) == _C.LS_ERR_INVALID_ARG
