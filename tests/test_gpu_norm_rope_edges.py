"""csrc/misc.hip where eps, the dtype, the scaling and the dispatch edges change the result: RMSNorm, the pass head, the folded
norm of the projections, the rotary table, the rotation and tree_positions against tests/norm_rope_oracle.py (fp64 on the CPU,
rounded where the reference rounds).  tests/test_norm_rope_oracle.py holds that oracle to the goldens and shows that the
eps cases fail for a kernel that gets eps wrong.  Every case is a handful of launches on KB-scale data."""
import pytest
import torch

import cases
import norm_rope_oracle as nro
from conftest import record_margin
from norm_rope_oracle import BF16, F16

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])


@pytest.fixture(scope="module")
def ops():
    from longspec_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def g(t):
    return t.to(DEV) if torch.is_tensor(t) else t


def assert_norm_bar(got, want, what):
    """The bar of test_rmsnorm_shapes: |diff| <= 2 ulp * max(|want|, 1e-2), fewer than 1 % of the elements differ; the
    non-finite pattern is the oracle's."""
    worst, share = nro.rmsnorm_margin(got, want)
    print(f"{what}: max |diff| {worst:.3f} ulp (bound 2), differing share {share:.3e} (bound 1e-2)")
    record_margin(what + " [max in ulp, mean = differing share]", worst, share, 2.0, 0.01)
    assert torch.equal(torch.isfinite(got.cpu()), torch.isfinite(want)), f"{what}: non-finite pattern differs from the oracle's"
    assert worst <= 2.0, f"{what}: {worst:.2f} ulp"
    assert share < 0.01, f"{what}: {share:.3%} of the elements differ"


# --------------------------------------------------------------------------- #
# A. RMSNorm
# --------------------------------------------------------------------------- #
def _norm_case(ops, x, r, w, eps, what):
    if r is None:
        y = ops.rmsnorm(g(x), g(w), eps)
        want, _ = nro.rmsnorm64(x, w, eps)
    else:
        y, s = ops.rmsnorm(g(x), g(w), eps, residual=g(r))
        want, s_want = nro.rmsnorm64(x, w, eps, residual=r)
        assert torch.equal(s_want, r + x)                                        # the oracle's sum is torch's, bit for bit
        assert nro.same_values(s, s_want), f"{what}: sum_out"
        y2 = ops.rmsnorm(s, g(w), eps)                                           # the same row handed over already summed
        assert nro.same_values(y2, y.cpu()), f"{what}: rmsnorm(s) != rmsnorm(x, residual)"
    assert_norm_bar(y, want, what)
    return y.cpu(), want


@pytest.mark.parametrize("regime", ["control", "below_eps", "eps_dominates", "zero_row"])
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@DTYPES
@pytest.mark.parametrize("shape", nro.NORM_SHAPES, ids=nro.shape_id)
def test_rmsnorm_where_eps_and_the_edges_matter(ops, shape, dtype, residual, regime):
    """Every dispatch of ls_rmsnorm_fwd (norm_rope_oracle.NORM_SHAPES) at inputs where mean(x^2) + eps is not mean(x^2):
    scale 2^-9 (mean square 3.8e-6 < eps = 1e-5) and 2^-12 (eps dominates), next to the N(0,1) control; and a row of zeros
    among ordinary rows: rs = rsqrt(eps), y exactly 0 there, the other rows as without it."""
    x, r, w, eps = nro.norm_inputs(*shape, dtype, regime, residual)
    y, want = _norm_case(ops, x, r, w, eps, f"rmsnorm {nro.shape_id(shape)} {regime}")
    assert bool(torch.isfinite(y).all())
    if regime == "zero_row":
        assert bool((y[1] == 0).all()) and bool((want[1] == 0).all()) and bool((y[0] != 0).any())


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("shape", nro.NORM_SHAPES, ids=nro.shape_id)
def test_rmsnorm_large_inputs_f16(ops, shape, residual):
    """fp16 at scale 200: x^2 up to 1e6, its fp32 sum is safe, y is finite and meets the bar."""
    x, r, w, eps = nro.norm_inputs(*shape, F16, "large", residual)
    y, _ = _norm_case(ops, x, r, w, eps, f"rmsnorm {nro.shape_id(shape)} scale 200")
    assert bool(torch.isfinite(y).all())


@pytest.mark.parametrize("shape", nro.NORM_SHAPES, ids=nro.shape_id)
def test_rmsnorm_residual_sum_leaves_f16(ops, shape):
    """A handful of r + x sums beyond 65504 in the first and the last row: sum_out is torch's r + x, infinities included.
    By the reference's arithmetic (stated from the oracle, tests/test_norm_rope_oracle.py) such a row has mean = inf,
    rsqrt(inf) = 0: y is NaN where the sum is infinite and +-0 in the rest of the row; the other rows are ordinary."""
    x, r, w, eps, hit = nro.overflow_inputs(*shape)
    y, want = _norm_case(ops, x, r, w, eps, f"rmsnorm {nro.shape_id(shape)} overflowing sum")
    inf = torch.isinf(r + x)
    assert int(inf.sum()) == 3 * len(hit)
    assert torch.equal(torch.isnan(want), inf) and torch.equal(torch.isnan(y), inf)
    assert bool((y[hit][~inf[hit]] == 0).all())


@DTYPES
def test_rmsnorm_refuses_a_prefill_row_beyond_its_lds(ops, dtype):
    """129 rows go to the prefill kernel, whose row buffer + 16 bytes must fit 64 KiB: hidden 32760 does (tested above),
    32768 is LS_ERR_UNSUPPORTED (-2) and nothing is launched."""
    x = torch.ones((129, 32768), dtype=dtype, device=DEV)
    w = torch.ones((32768,), dtype=dtype, device=DEV)
    with pytest.raises(RuntimeError, match=r"code -2\).*too large"):
        ops.rmsnorm(x, w, 1e-5)
    with pytest.raises(RuntimeError, match=r"code -2\).*too large"):
        ops.rmsnorm(x, w, 1e-5, residual=x)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- #
# B. eps through the pass head and the folded norm
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("scale", [2.0 ** -9, 2.0 ** -12], ids=["2^-9", "2^-12"])
@pytest.mark.parametrize("b,q", [(1, 1), (1, 5), (2, 37)])
@pytest.mark.parametrize("hidden", [256, 1000, 8200])
@DTYPES
def test_pass_head_against_the_oracle_where_eps_matters(ops, dtype, hidden, b, q, scale):
    """An embedding table at scale 2^-9 / 2^-12 with eps = 1e-5: `normed` against rmsnorm64(table[ids]) -- not against
    ops.rmsnorm --, `embeds` bit-equal to table[ids], and the pass's rotary table against rope_table64."""
    gen = torch.Generator().manual_seed(hidden + 17 * b + q)
    vocab, eps, scaling = 301, 1e-5, 0.8366
    table = (torch.randn((vocab, hidden), generator=gen) * scale).to(dtype)
    wgt = (1.0 + 0.1 * torch.randn((hidden,), generator=gen)).to(dtype)
    ids = torch.randint(0, vocab, (b, q), generator=gen)
    pos = torch.randint(0, 262144, (b, q), generator=gen)
    inv_freq = next(iter(cases.rope_cases()))["inv_freq"]
    emb, nrm, (cos, sin) = ops.pass_head(g(table), g(ids), g(inv_freq), scaling, g(wgt), eps, position_ids=g(pos))
    assert torch.equal(emb.cpu(), table[ids])
    want, _ = nro.rmsnorm64(table[ids], wgt, eps)
    assert float(table[ids].double().pow(2).mean(-1).max()) < eps
    assert_norm_bar(nrm, want, f"pass_head hidden={hidden} rows={b}x{q}")
    for got, ref in zip((cos, sin), nro.rope_table64(pos, inv_freq, scaling, dtype)):
        mx, bound, share = nro.rope_margin(got, ref, scaling)
        assert mx <= bound and share < 1e-3, (mx, share)


@pytest.mark.parametrize("M", [1, 17, 74])
@DTYPES
def test_folded_norm_where_eps_matters(ops, dtype, M):
    """test_rmsnorm_folded_into_the_projections' identity -- the projection with norm=NormFold equals the same projection of
    ops.rmsnorm(h) bit for bit -- at a residual stream of scale 2^-9 (mean(h^2) < eps = 1e-5), where the fold's own
    rsqrt(tot / K + eps) (csrc/skinny_gemm.h) decides the result; and ops.rmsnorm(h) itself against the oracle.

    The FP8 and MXFP4 projections have no folded norm: csrc/gemm_w8.hip and gemm_w4.hip answer norm_weight / ssq_in with
    LS_ERR_UNSUPPORTED and ops.linear raises ValueError before that, so the fold's rsqrt is not shared with them and there is
    no identity to repeat there.  What is checked instead, with the packers of test_gpu_linear_w8 / _w4 at these shapes (K =
    256): they refuse norm=, and the chain they do run -- ops.rmsnorm, then the 8- / 4-bit projection -- equals the folded
    16-bit projection on the de-quantised weight bit for bit."""
    from longspec_amd import quant
    hidden, inter, eps = 256, 512, 1e-5

    def mk(shape, seed, scale=1.0):
        return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)

    x = g(mk((1, M, inter), 1, 2.0 ** -9))
    res = g(mk((1, M, hidden), 2, 2.0 ** -9))
    w_down = ops.pack_weight(g(mk((hidden, inter), 3, inter ** -0.5)))
    nw = (1.0 + 0.1 * mk((hidden,), 4).float()).to(dtype)
    h, ssq = ops.linear(x, w_down, None, residual=res, ssq_out=True)
    assert float(h.double().pow(2).mean(-1).max()) < eps and float(h.double().pow(2).mean(-1).min()) > 0.1 * eps
    hn = ops.rmsnorm(h, g(nw), eps)
    want, _ = nro.rmsnorm64(h.cpu(), nw, eps)
    assert_norm_bar(hn, want, f"rmsnorm of the stream M={M}")
    fold = ops.NormFold(g(nw), eps, ssq)
    gu = ops.pack_gate_up(g(mk((inter, hidden), 5, hidden ** -0.5)), g(mk((inter, hidden), 6, hidden ** -0.5)))
    assert torch.equal(ops.mlp_gate_up(h, gu, norm=fold), ops.mlp_gate_up(hn, gu))
    w2, b2 = g(mk((1000, hidden), 7, hidden ** -0.5)), g(mk((1000,), 8, 0.3))
    y_fold = ops.linear(h, ops.pack_weight(w2), b2, norm=fold)
    assert torch.equal(y_fold, ops.linear(hn, ops.pack_weight(w2), b2))
    assert not torch.equal(y_fold, ops.linear(h, ops.pack_weight(w2), b2, norm=ops.NormFold(g(nw), 0.1 * eps, ssq)))
    # 8-bit (e4m3, power-of-two row scales) and 4-bit (MXFP4) weights
    q8, s8 = ops.quantize_rows_e4m3(w2)
    q4, e4 = ops.quantize_blocks_mxfp4(w2)
    for packed, deq in ((ops.pack_weight8((q8, s8)), quant.dequantize_rows_e4m3(q8, s8, dtype)),
                        (ops.pack_weight4((q4, e4)), quant.dequantize_blocks_mxfp4(q4, e4, dtype))):
        with pytest.raises(ValueError, match="folded RMSNorm"):
            ops.linear(h, packed, b2, norm=fold)
        assert torch.equal(ops.linear(hn, packed, b2), ops.linear(h, ops.pack_weight(deq), b2, norm=fold))


# --------------------------------------------------------------------------- #
# C. rotary table
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("rows", nro.ROPE_ROWS)
@pytest.mark.parametrize("scaling", nro.ROPE_SCALINGS)
@DTYPES
@pytest.mark.parametrize("c", list(cases.rope_cases()), ids=lambda c: c["name"])
def test_rope_table_against_fp64(ops, c, dtype, scaling, rows):
    """ls_rope_cos_sin in both dtypes against rope_table64, with the four goldens' inv_freq (theta = 283461213, 1e6, linear
    x4 and x8): positions 2^24 + 1 (float(pos) rounds), 0, 1, 131071, 131072, 262143 and random ones, row counts that are
    no multiple of the 4 rows of a workgroup.  Equality is what the code promises; the bar of test_rope_golden (at most one
    ulp, fewer than 1e-3 of the entries) allows for a last-bit difference between the device's double cos and the host's.
    MEASURED on MI355X: bf16, and fp16 at scaling 1.0, differ nowhere (0 of 80 + 40 tables).  fp16 at scaling 0.8366 differs by
    one ulp in up to 6 of the 33280 entries of a 260-row table (share <= 1.8e-4; none in the smaller tables), and not because of
    cos: the compiler fuses `fp32(cos) * scaling` and the conversion into one v_fma_mixlo_f16, which rounds the exact product
    ONCE, where the reference rounds it to fp32 and then to fp16.  Rounding fp64(fp32(cos)) * fp64(fp32(scaling)) once on the
    host gives exactly the entries observed (4 / 2 / 4 / 6 cos and 0 / 4 / 2 / 0 sin entries for the four inv_freq)."""
    pos = nro.rope_positions(rows, rows)
    got = ops.rope_cos_sin(g(pos), g(c["inv_freq"]), scaling, dtype)
    want = nro.rope_table64(pos, c["inv_freq"], scaling, dtype)
    for name, a, b in zip(("cos", "sin"), got, want):
        assert a.shape == (1, rows, 128) and a.dtype == dtype
        mx, bound, share = nro.rope_margin(a, b, scaling)
        print(f"rope table {c['name']} {name}: max |diff| {mx:.3e} (bound {bound:.3e}), differing share {share:.3e}")
        record_margin(f"rope table {name} [mean = differing share]", mx, share, bound, 1e-3)
        assert mx <= bound and share < 1e-3, (name, mx, share)
        assert torch.equal(a[..., :64], a[..., 64:])


# --------------------------------------------------------------------------- #
# D. rotation
# --------------------------------------------------------------------------- #
@DTYPES
@pytest.mark.parametrize("shape", nro.ROPE_APPLY_SHAPES, ids=nro.shape_id)
def test_rope_apply_against_fp64(ops, shape, dtype):
    """ls_rope_apply in both dtypes, bit-equal to rope_apply_ref on tables at scaling 0.8366, with entries +-0 and +-65504
    (fp16) / +-3e38 (bf16): where two extreme products add up past the format the output is the oracle's infinity.  q / k are
    views of one fused QKV buffer (row stride != heads * 128, the V columns stay untouched), k may have no head at all, and a
    [1, R, 128] table is broadcast over the batch."""
    b, R, Hq, Hk, tb = shape
    inv_freq = next(iter(cases.rope_cases()))["inv_freq"]
    q, k, cos, sin = nro.rope_apply_inputs(*shape, dtype, inv_freq)
    v = torch.randn((b, R, max(Hk, 1) * 128), generator=torch.Generator().manual_seed(5)).to(dtype)
    qkv = torch.cat((q.reshape(b, R, Hq * 128), k.reshape(b, R, Hk * 128), v), -1)
    buf = g(qkv).clone()
    qv = buf[..., :Hq * 128].view(b, R, Hq, 128)
    kv = buf[..., Hq * 128:(Hq + Hk) * 128].view(b, R, Hk, 128) if Hk else qv[:, :, :0]
    ops.rope_apply_(qv, kv, g(cos), g(sin))
    want_q, want_k = nro.rope_apply_ref(q, cos, sin), nro.rope_apply_ref(k, cos, sin)
    assert bool(torch.isinf(want_q).any()) and not bool(torch.isnan(want_q).any())
    assert nro.same_values(qv, want_q) and nro.same_values(kv, want_k)
    assert torch.equal(buf[..., (Hq + Hk) * 128:].cpu(), v)


# --------------------------------------------------------------------------- #
# E. tree_positions
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("with_base", [True, False], ids=["base", "no_base"])
@pytest.mark.parametrize("top", [1, 3], ids=["0/1", "0..3"])
@pytest.mark.parametrize("b,M,N", [(1, 1, 1), (3, 5, 7), (2, 74, 96), (5, 3, 65), (1, 130, 1000), (2, 7, 64)])
def test_tree_positions_exact(ops, b, M, N, top, with_base):
    """mask.sum(-1) - 1 + base[:, None] in int64: batch rows with bases of their own (the last near 2^31, so that the sum
    leaves int32), no base at all, N below and off the 64 lanes of a row's wave, row counts off the 4 rows of a workgroup,
    and mask entries above 1 (the kernel sums, it does not count)."""
    gen = torch.Generator().manual_seed(b * 1000 + M * 10 + N)
    mask = torch.randint(0, top + 1, (b, M, N), generator=gen)
    mask[-1, -1] = top                                       # the largest sum there is
    base = torch.tensor([1234 + 100003 * z for z in range(b - 1)] + [2 ** 31 - 2000 + N // 2], dtype=torch.int32)
    want = mask.sum(-1) - 1 + (base.long()[:, None] if with_base else 0)
    if with_base and top * N > 2000:
        assert int(want.max()) > 2 ** 31 - 1
    got = ops.tree_positions(g(mask), g(base) if with_base else None)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
