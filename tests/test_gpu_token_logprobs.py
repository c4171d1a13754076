"""``ops.token_logprobs`` (csrc/logprob.hip) against the float64 oracle of tests/logprob_oracle.py: indices exactly, in (logit
descending, column ascending) order; values within  topk_oracle.TOL + 2^-22 |lp|  -- TOL (1e-5) is the project's bound for an
fp32 log-sum-exp at these vocabularies, the relative term the fp32 roundings of the value itself (the difference, the division
by T, the final subtraction); derived, not measured.  Constructed rows, the exact properties (the chosen value is its list entry
bit for bit; a row's outputs do not depend on its neighbours) and the refusals."""
import math

import numpy as np
import pytest
import torch

import logprob_oracle as lo
from topk_oracle import TOL

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
# (V, rows, b, dtype, T, n): under one chunk of 8192 columns, exactly one, one plus an 8-column tail, the two real vocabularies;
# every value of every axis, and n = 20 against the 8-column tail
CASES = [(1016, 1, 1, F16, 1.0, 0), (1016, 2, 2, BF16, 0.6, 20), (8192, 2, 1, F16, 2.0, 5), (8192, 69, 2, BF16, 1.0, 1),
         (8200, 1, 2, F16, 0.6, 20), (8200, 69, 1, BF16, 2.0, 5), (128256, 69, 1, F16, 0.6, 5), (128256, 2, 2, BF16, 1.0, 20),
         (128256, 1, 1, F16, 2.0, 0), (152064, 69, 1, BF16, 0.6, 20), (152064, 1, 2, F16, 1.0, 1), (152064, 2, 1, F16, 2.0, 0),
         # the verification pass's 69 rows with a batch at the real vocabularies, both types
         (128256, 69, 2, BF16, 0.6, 5), (152064, 69, 2, F16, 1.0, 20)]


def strided(x):
    """The same values [b, R, V] on the device in a buffer with a row stride > V and a non-dense batch stride."""
    b, R, V = x.shape
    buf = torch.full((b, R + 1, V + 24), 77.0, dtype=x.dtype, device="cuda")
    view = buf[:, :R, :V]
    view.copy_(x)
    assert view.stride(1) > V and view.stride(0) > R * view.stride(1)
    return view


def run(x, ids, T, n):
    from longspec_amd import ops
    got = ops.token_logprobs(x, ids.cuda(), T, n)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in got)


def check(got, x_cpu, ids, T, n, what):
    """Indices exact, values within the bound; returns the worst value error."""
    row_lp, top_val, top_idx = got
    want_lp, want_val, want_idx = lo.token_logprobs64(x_cpu, ids, T, n)
    assert np.array_equal(top_idx.numpy(), want_idx), f"{what}: top-n indices"
    worst = 0.0
    for g, w in ((row_lp.numpy().astype(np.float64), want_lp), (top_val.numpy().astype(np.float64), want_val)):
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isinf(g), np.isinf(w)), f"{what}: NaN / inf pattern"
        fin = np.isfinite(w)
        assert (g[~fin & ~np.isnan(w)] == w[~fin & ~np.isnan(w)]).all(), what
        err = np.abs(g[fin] - w[fin])
        assert (err <= TOL + 2.0 ** -22 * np.abs(w[fin])).all(), f"{what}: value error {err.max():.3e}"
        worst = max(worst, float(err.max()) if err.size else 0.0)
    return worst


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("V,R,b,dtype,T,n", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_random_rows_against_the_oracle(V, R, b, dtype, T, n):
    g = torch.Generator().manual_seed(V + R + n)
    x = (torch.randn((b, R, V), generator=g) * 3).to(dtype)
    ids = torch.randint(0, V, (b, R), generator=g)
    got = run(strided(x), ids, T, n)
    worst = check(got, x, ids, T, n, "random")
    print(f"V={V} rows={R} b={b} {dtype} T={T} n={n}: worst value error {worst:.3e} (bound {TOL:g} + 2^-22 |lp|)")
    row_lp, top_val, top_idx = got
    hit = top_idx == ids[..., None]                                   # the chosen value IS its list entry
    assert torch.equal(bits(top_val[hit]), bits(row_lp[..., None].expand_as(top_val)[hit].contiguous()))


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_constructed_rows(dtype):
    V, n, T = 8200, 20, 0.6
    g = torch.Generator().manual_seed(1)
    x = (torch.randn((1, 6, V), generator=g) * 2).to(dtype)
    ids = torch.zeros((1, 6), dtype=torch.int64)
    # row 0: a run of equal maxima across the chunk border (8190 .. 8195), and the chosen id in the short last chunk
    x[0, 0, 8190:8196] = 12.0
    ids[0, 0] = 8195
    # row 1: +-0.0 as the largest logits, on both sides of the border: equal, ordered by column
    x[0, 1] = -x[0, 1].abs() - 1
    x[0, 1, [5, 8188, 8193, 8199]] = torch.tensor([-0.0, 0.0, -0.0, 0.0]).to(dtype)
    ids[0, 1] = 8193
    # row 2: -inf columns, the chosen id points at one
    x[0, 2, 100:4000] = -math.inf
    x[0, 2, 8192:] = -math.inf
    ids[0, 2] = 8197
    # row 3: one finite logit (the first chunk is -inf only)
    x[0, 3] = -math.inf
    x[0, 3, 8194] = -3.0
    ids[0, 3] = 8194
    # row 4: an id outside the vocabulary; row 5: a negative one
    ids[0, 4], ids[0, 5] = V, -1
    got = run(strided(x), ids, T, n)
    worst = check(got, x, ids, T, n, "constructed")
    print(f"{dtype}: worst value error {worst:.3e}")
    row_lp, top_val, top_idx = got
    assert top_idx[0, 0, :6].tolist() == [8190, 8191, 8192, 8193, 8194, 8195] and len(set(bits(top_val[0, 0, :6]).tolist())) == 1
    assert bits(row_lp[0, 0:1]).item() == bits(top_val[0, 0, 5:6].contiguous()).item()
    assert top_idx[0, 1, :4].tolist() == [5, 8188, 8193, 8199] and len(set(bits(top_val[0, 1, :4].contiguous()).tolist())) == 1
    assert bits(row_lp[0, 1:2]).item() == bits(top_val[0, 1, 2:3].contiguous()).item()
    assert row_lp[0, 2].item() == -math.inf
    assert row_lp[0, 3].item() == 0.0 and top_idx[0, 3, 0].item() == 8194 and top_val[0, 3, 0].item() == 0.0
    assert (top_val[0, 3, 1:] == -math.inf).all() and top_idx[0, 3, 1:].tolist() == list(range(19))
    assert torch.isnan(row_lp[0, 4:]).all() and not torch.isnan(top_val).any()


def test_a_list_longer_than_the_row_is_padded():
    x = torch.arange(8, dtype=torch.float16).view(1, 1, 8)
    row_lp, top_val, top_idx = run(x.cuda(), torch.tensor([[3]]), 1.0, 20)
    check((row_lp, top_val, top_idx), x, torch.tensor([[3]]), 1.0, 20, "short row")
    assert top_idx[0, 0].tolist() == [7, 6, 5, 4, 3, 2, 1, 0] + [-1] * 12 and (top_val[0, 0, 8:] == -math.inf).all()


def test_a_rows_outputs_do_not_depend_on_its_neighbours():
    V, n, T = 128256, 5, 0.6
    g = torch.Generator().manual_seed(7)
    x = (torch.randn((1, 69, V), generator=g) * 3).to(F16)
    ids = torch.randint(0, V, (1, 69), generator=g)
    full = run(x.cuda(), ids, T, n)
    alone = run(x[:, 40:41].cuda(), ids[:, 40:41], T, n)
    rev = run(x.flip(1).cuda(), ids.flip(1), T, n)
    batch = run(x.view(3, 23, V).cuda(), ids.view(3, 23), T, n)
    for f, a, r, bt in zip(full, alone, rev, batch):
        assert torch.equal(bits(f[:, 40:41].contiguous()), bits(a)), "a row alone"
        assert torch.equal(bits(f), bits(r.flip(1).contiguous())), "reversed row order"
        assert torch.equal(bits(f.reshape(bt.shape)), bits(bt)), "rows as batch"


def test_invalid_arguments_raise_before_any_launch():
    from longspec_amd import _C, ops
    lib = _C.load()
    x = torch.zeros((1, 2, 1024 + 8), dtype=F16, device="cuda")
    ids = torch.zeros((1, 2), dtype=torch.int64, device="cuda")
    lp = torch.full((1, 2), 5.0, dtype=torch.float32, device="cuda")
    tv = torch.zeros((1, 2, 20), dtype=torch.float32, device="cuda")
    ti = torch.zeros((1, 2, 20), dtype=torch.int64, device="cuda")
    ws = torch.zeros((1 << 16,), dtype=torch.uint8, device="cuda")

    def call(V=1024, ld=1032, sb=2064, T=1.0, n=5, b=1, rows=2, off=0):
        return lib.ls_token_logprobs(x.data_ptr() + off, b, rows, V, _C.LS_F16, sb, ld, ids.data_ptr(), 2, T, n, lp.data_ptr(),
                                     tv.data_ptr(), ti.data_ptr(), ws.data_ptr(), ws.numel(), None)

    assert call() == _C.LS_OK
    for bad in (dict(V=1020), dict(ld=1028), dict(sb=2060), dict(ld=1016), dict(off=2), dict(T=0.0), dict(T=-1.0), dict(T=math.nan),
                dict(n=-1), dict(n=21), dict(rows=0), dict(b=0), dict(b=1025, rows=1), dict(b=2, rows=513)):
        lp.fill_(5.0)
        assert call(**bad) == _C.LS_ERR_INVALID_ARG, bad
        torch.cuda.synchronize()
        assert (lp == 5.0).all(), f"{bad}: something was launched"
    with pytest.raises(RuntimeError):
        ops.token_logprobs(x[:, :, :1024], ids, 0.0, 5)
    with pytest.raises(RuntimeError):
        ops.token_logprobs(x[:, :, :1024], ids, 1.0, 21)
