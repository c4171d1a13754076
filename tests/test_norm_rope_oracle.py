"""tests/norm_rope_oracle.py held to what is already trusted -- the reference's goldens (norm_rope.npz) under the bars the GPU
tests use for them, and oracle.ref_ops in both dtypes -- and the proof that the cases of tests/test_gpu_norm_rope_edges.py have
teeth: at the inputs where eps matters, an RMSNorm that drops eps, adds it outside the root or divides it by hidden misses the
bar of test_rmsnorm_shapes by almost every element, while at the N(0,1) inputs the suite used so far all three pass it."""
import numpy as np
import pytest
import torch

import cases
import norm_rope_oracle as nro
from norm_rope_oracle import BF16, F16, F64
from oracle import ref_ops

DTYPES = pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])


# ---- the rounding itself ------------------------------------------------------------------------------------------------
def test_round_to_rounds_once():
    """Just above a tie: fp64 -> fp32 lands ON the tie, and the second rounding goes to even, the wrong way.  That is what
    torch's cast does; round_to must not."""
    for dtype, m in ((F16, 10), (BF16, 7)):
        x = torch.tensor([1.0 + 2.0 ** -(m + 1) + 2.0 ** -40, -(1.0 + 2.0 ** -(m + 1) + 2.0 ** -40),
                          1.0 + 3 * 2.0 ** -(m + 1) - 2.0 ** -40, 1.0 + 2.0 ** -(m + 1), 1.0 + 3 * 2.0 ** -(m + 1)], dtype=F64)
        want = torch.tensor([1.0 + 2.0 ** -m, -(1.0 + 2.0 ** -m), 1.0 + 2.0 ** -m, 1.0, 1.0 + 2.0 ** -(m - 1)], dtype=F64)
        assert torch.equal(nro.round_to(x, dtype).double(), want)
        assert not torch.equal(x.to(dtype).double(), want), "torch rounds once now: round_to can go"
    special = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 1e-60, -1e-60, 65519.99, 65520.0, 1e39, 3.5e38], dtype=F64)
    assert nro.round_to(special, F16).tolist() == [0.0, -0.0, float("inf"), -float("inf"), 0.0, -0.0, 65504.0, float("inf"),
                                                   float("inf"), float("inf")]
    assert nro.round_to(special, BF16)[-2:].tolist() == [float("inf"), float("inf")]
    assert torch.isnan(nro.round_to(torch.tensor([float("nan")], dtype=F64), F16)).all()
    # numpy casts fp64 -> fp16 in one rounding: a million values, and the neighbourhood of every tie of one binade
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1 << 20, generator=g, dtype=F64) * torch.exp2(torch.randint(-26, 13, (1 << 20,), generator=g).double())
    ties = 1.0 + (2 * torch.arange(1024, dtype=F64) + 1) * 2.0 ** -11
    x = torch.cat([x, ties, ties * (1 + 2.0 ** -50), ties * (1 - 2.0 ** -50), ties * 2.0 ** -20])
    assert torch.equal(nro.round_to(x, F16), torch.from_numpy(x.numpy().astype(np.float16)))


# ---- the goldens, under the bars tests/test_gpu_ops.py holds the kernels to ----------------------------------------------
@pytest.mark.parametrize("c", list(cases.norm_cases()), ids=lambda c: c["name"])
def test_rmsnorm64_on_the_goldens(c):
    y, s = nro.rmsnorm64(c["x"], c["w"], c["eps"])
    assert torch.equal(s, c["x"])
    d = (y.float() - c["y"].float()).abs()
    assert d.max().item() <= 1.5e-3 and d.mean().item() <= 1e-6 and (d > 0).float().mean().item() <= 0.002
    assert nro.rmsnorm_bar_holds(c["y"], y)


@pytest.mark.parametrize("c", list(cases.rope_cases()), ids=lambda c: c["name"])
def test_rope64_on_the_goldens(c):
    cos, sin = nro.rope_table64(c["pos"], c["inv_freq"], c["scaling"], F16)
    for got, want in ((cos, c["cos"]), (sin, c["sin"])):
        mx, bound, share = nro.rope_margin(want, got, c["scaling"])
        assert mx <= bound and share < 1e-3
    assert torch.equal(nro.rope_apply_ref(c["q"], c["cos"], c["sin"]), c["q_out"])
    assert torch.equal(nro.rope_apply_ref(c["k"], c["cos"], c["sin"]), c["k_out"])


# ---- both dtypes against oracle.ref_ops, at the cases of the GPU tests ------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("scaling", nro.ROPE_SCALINGS)
def test_rope_table64_agrees_with_ref_ops(dtype, scaling):
    for c in cases.rope_cases():
        for rows in nro.ROPE_ROWS:
            pos = nro.rope_positions(rows, rows)
            want = nro.rope_table64(pos, c["inv_freq"], scaling, dtype)
            got = ref_ops.rope_cos_sin(pos, c["inv_freq"], scaling, dtype)
            for a, b in zip(got, want):
                mx, bound, share = nro.rope_margin(a, b, scaling)
                assert mx <= bound and share < 1e-3, (c["name"], rows, mx, share)
                assert torch.equal(b[..., :64], b[..., 64:])
    assert int(pos[0, 0]) == 2 ** 24 + 1 and float(pos[0, 0].float()) == 2.0 ** 24


@DTYPES
@pytest.mark.parametrize("shape", nro.ROPE_APPLY_SHAPES, ids=nro.shape_id)
def test_rope_apply_ref_agrees_with_ref_ops(dtype, shape):
    inv_freq = next(iter(cases.rope_cases()))["inv_freq"]
    q, k, cos, sin = nro.rope_apply_inputs(*shape, dtype, inv_freq)
    for x in (q, k):
        want = nro.rope_apply_ref(x, cos, sin)
        assert nro.same_values(ref_ops.apply_rope(x, cos, sin), want)
        if x.shape[2]:
            # the extreme entries do what they are there for: sums that leave the format, products that do not
            assert torch.isinf(want).any() and not torch.isnan(want).any()
            assert (want.abs().double() >= 0.5 * nro.EXTREME[dtype]).sum() > torch.isinf(want).sum()


# ---- RMSNorm: ref_ops passes the bar everywhere, the wrong-eps variants only where eps does not matter ----------------------
@DTYPES
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("shape", nro.NORM_SHAPES, ids=nro.shape_id)
def test_the_eps_cases_have_teeth(shape, residual, dtype):
    for regime in ("control",) + nro.EPS_SENSITIVE:
        x, r, w, eps = nro.norm_inputs(*shape, dtype, regime, residual)
        want, s = nro.rmsnorm64(x, w, eps, residual=r)
        if residual:
            assert torch.equal(s, r + x)
        ms = s.double().pow(2).mean(-1)
        assert bool((ms < eps).all()) == (regime in nro.EPS_SENSITIVE)
        # (fp32 against fp64: up to 1e-3 of the elements differ -- in bf16 a row has 128 mantissas, and one of them near a
        # tie of x * rs moves every element that carries it)
        assert nro.rmsnorm_bar_holds(ref_ops.rmsnorm(s, w, eps), want), (regime, nro.rmsnorm_margin(ref_ops.rmsnorm(s, w, eps), want))
        for wrong in nro.WRONG_EPS:
            bad = nro.rmsnorm64(x, w, eps, residual=r, wrong_eps=wrong)[0]
            if regime == "control":
                assert nro.rmsnorm_bar_holds(bad, want), (regime, wrong, nro.rmsnorm_margin(bad, want))
            else:
                assert not nro.rmsnorm_bar_holds(bad, want), (regime, wrong)
                ulp = nro.ULP[dtype]
                out = ((bad.double() - want.double()).abs() > 2 * ulp * want.double().abs().clamp(min=1e-2)).double().mean().item()
                assert out >= 0.99, (regime, wrong, out)


@DTYPES
def test_zero_row_large_and_overflow_cases_in_the_oracle(dtype):
    """What the GPU test will ask of the kernel, stated from the oracle: a zero row gives exact zeros (rsqrt(eps) is finite),
    scale 200 stays finite, and a row with an infinite sum has rsqrt(inf) = 0: NaN at the infinities, +-0 everywhere else."""
    x, r, w, eps = nro.norm_inputs(5, 1000, dtype, "zero_row", True)
    y, s = nro.rmsnorm64(x, w, eps, residual=r)
    assert bool((y[1] == 0).all()) and bool(torch.isfinite(y).all()) and bool((y[0] != 0).any())
    assert nro.rmsnorm_bar_holds(ref_ops.rmsnorm(s, w, eps), y)
    if dtype != F16:
        return
    x, r, w, eps = nro.norm_inputs(5, 1000, F16, "large", True)
    y, s = nro.rmsnorm64(x, w, eps, residual=r)
    assert bool(torch.isfinite(y).all()) and s.abs().max().item() > 600 and nro.rmsnorm_bar_holds(ref_ops.rmsnorm(s, w, eps), y)
    x, r, w, eps, hit = nro.overflow_inputs(5, 1000)
    y, s = nro.rmsnorm64(x, w, eps, residual=r)
    assert torch.equal(s, r + x) and hit == [0, 4]
    assert int(torch.isinf(s).sum()) == 6 and torch.equal(torch.isnan(y), torch.isinf(s))
    assert bool((y[hit][~torch.isinf(s[hit])] == 0).all()) and (y[1:4] != 0).float().mean().item() > 0.99
    assert nro.rmsnorm_bar_holds(ref_ops.rmsnorm(s, w, eps), y)
