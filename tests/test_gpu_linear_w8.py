"""ls_linear_w8_fwd (the skinny GEMM with e4m3 weights) and its quantiser / packer.

Yardstick: with a power-of-two scale per row, the 8-bit launch is BIT-IDENTICAL to the 16-bit launch (ls_linear_fwd) on the
de-quantised weight -- same launch plan, same k order, exact conversion, exact scale.  No tolerance is involved there.  Against
the exact (fp64) product the rule is tests/test_gpu_linear.py's with one more fp32 rounding for the scale multiply:
|got - want| <= 1.001 ulp(want) + 5 * 2^-24 * |x| . |q s|^T, and >= 99 % of the elements equal."""
import pytest
import torch

from test_gpu_linear import SHAPES, _ulp

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
MS = [1, 5, 16, 17, 32, 33, 74, 80]
SPLITS = [1, 2, 3, 5, 8]
# (a) every de-quantised value is fp16-normal or zero (s >= 2^-5, smallest non-zero |q s| = 2^-14); (b) the suite's usual
# weights, where many de-quantised values are fp16 subnormals
DISTS = {"normal_range": (4.0, 1.0 / 64), "std0.03": (0.03, 1.0)}


def _mk(shape, seed, scale=1.0, dtype=torch.float16):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda") * scale).to(dtype)


def _deq(q, s, dtype):
    from longspec_amd import quant
    return quant.dequantize_rows_e4m3(q, s, dtype)


# ---- item 4 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("N", [100, 264])
@pytest.mark.parametrize("K", [128, 192, 640, 4096, 27648])
def test_device_quantizer_equals_host_quantizer(dtype, N, K):
    from longspec_amd import ops, quant
    for std in (0.03, K ** -0.5, 4.0):
        w = _mk((N, K), N + K, std, dtype)
        w[3] = 0
        for pow2 in (True, False):
            q, s = ops.quantize_rows_e4m3(w, pow2=pow2)
            hq, hs = quant.quantize_rows_e4m3(w.cpu(), pow2=pow2)
            assert torch.equal(s.cpu(), hs), (std, pow2)
            assert torch.equal(q.cpu(), hq), (std, pow2)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_in_kernel_conversion_is_exact_for_every_byte(dtype):
    """A weight whose rows run through all 256 encodings (the two NaN encodings excepted) times one-hot rows of x returns
    q * s exactly: the fp8 -> f16 / bf16 conversion, the byte order inside the packed dwords and the layout are right."""
    from longspec_amd import ops
    N, K = 128, 256
    n, k = torch.meshgrid(torch.arange(N), torch.arange(K), indexing="ij")
    q = ((k + 37 * n) % 256).to(torch.uint8)
    q[(q & 0x7F) == 0x7F] = 0x7E
    for r in range(N):
        assert len(set(q[r].tolist())) == 254
    s = torch.exp2(((torch.arange(N) % 6) - 4).float())                 # 2^-4 .. 2^1: q s stays an fp16 normal or zero
    want = _deq(q, s, dtype).cuda()                                      # [N, K]
    pw = ops.pack_weight8((q.cuda(), s.cuda()))
    eye = torch.eye(K, dtype=dtype, device="cuda")
    for k0 in range(0, K, 64):
        for M in (64, 16, 1):
            y = ops.linear(eye[k0:k0 + M], pw)
            assert torch.equal(y, want[:, k0:k0 + M].t()), (k0, M)


# ---- item 5 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("dist", list(DISTS))
def test_linear_bit_identical_to_16bit_kernel(N, K, dtype, dist):
    """linear(x, pack_weight8(q, s)) == linear(x, pack_weight(q * s)) bit for bit at every forced split count (and the
    automatic one), with and without bias and with the residual epilogue.

    MEASURED on MI355X: see DESIGN.md, "8-bit weights" for the fp16-subnormal case (distribution std0.03)."""
    from longspec_amd import ops
    wstd, xstd = DISTS[dist]
    q, s = ops.quantize_rows_e4m3(_mk((N, K), N + K, wstd, dtype))
    p8, p16 = ops.pack_weight8((q, s)), ops.pack_weight(_deq(q, s, dtype))
    b = _mk((N,), 7, 0.1, dtype)
    for M in MS:
        x = _mk((M, K), M + K, xstd, dtype)
        r = _mk((M, N), 6, 1.0, dtype)
        for S in [0] + SPLITS:
            for kw in ({}, {"bias": b}, {"bias": b, "residual": r}):
                y8, y16 = ops.linear(x, p8, n_splits=S, **kw), ops.linear(x, p16, n_splits=S, **kw)
                assert torch.equal(y8, y16), f"M={M} S={S} {sorted(kw)}: {(y8 != y16).sum().item()} of {y8.numel()} differ"


@pytest.mark.parametrize("dims", [(4096, 1024, 4096), (512, 128, 256), (5120, 5120, 5120), (1024, 256, 896)],
                         ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("dist", list(DISTS))
def test_qkv_launches_bit_identical_to_16bit_kernel(dims, dtype, dist):
    from longspec_amd import ops
    Nq, Nkv, K = dims
    wstd, xstd = DISTS[dist]
    qs = [ops.quantize_rows_e4m3(_mk((n, K), 2 + i, wstd, dtype)) for i, n in enumerate((Nq, Nkv, Nkv))]
    bs = [_mk((n,), 7 + i, 0.5, dtype) for i, n in enumerate((Nq, Nkv, Nkv))]
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 128, 2).float() / 128))
    plain8, plain16 = [ops.pack_weight8(p) for p in qs], [ops.pack_weight(_deq(*p, dtype)) for p in qs]
    rope8 = [ops.pack_weight8(p, rope=i < 2) for i, p in enumerate(qs)]
    rope16 = [ops.pack_weight(_deq(*p, dtype), rope=i < 2) for i, p in enumerate(qs)]
    for M in MS:
        x = _mk((1, M, K), 1 + M, xstd, dtype)
        cos, sin = ops.rope_cos_sin(torch.arange(1000, 1000 + M, device="cuda")[None], inv_freq.cuda(), 1.0, dtype)
        for S in [0] + SPLITS:
            for a, c in zip(ops.linear_multi(x, plain8, bs, n_splits=S), ops.linear_multi(x, plain16, bs, n_splits=S)):
                assert torch.equal(a, c), (M, S)
            for a, c in zip(ops.linear_qkv_rope(x, rope8, bs, cos, sin, n_splits=S), ops.linear_qkv_rope(x, rope16, bs, cos, sin, n_splits=S)):
                assert torch.equal(a, c), (M, S)
        (a,), (c,) = ops.linear_qkv_rope(x, rope8[:1], None, cos, sin), ops.linear_qkv_rope(x, rope16[:1], None, cos, sin)
        assert torch.equal(a, c)


@pytest.mark.parametrize("N,K", [(14336, 4096), (512, 256), (1024, 896), (1536, 512), (13824, 5120), (27648, 5120)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("dist", list(DISTS))
def test_mlp_gate_up_bit_identical_to_16bit_kernel(N, K, dtype, dist):
    from longspec_amd import ops
    wstd, xstd = DISTS[dist]
    g, u = ops.quantize_rows_e4m3(_mk((N, K), 61, wstd, dtype)), ops.quantize_rows_e4m3(_mk((N, K), 62, wstd, dtype))
    p8, p16 = ops.pack_gate_up8(g, u), ops.pack_gate_up(_deq(*g, dtype), _deq(*u, dtype))
    for M in MS:
        x = _mk((M, K), 63 + M, xstd, dtype)
        for S in [0] + SPLITS:
            assert torch.equal(ops.mlp_gate_up(x, p8, n_splits=S), ops.mlp_gate_up(x, p16, n_splits=S)), (M, S)


def test_pack_from_16bit_weight_equals_pack_from_q_scale():
    from longspec_amd import ops
    w = _mk((1024, 512), 3, 0.03)
    a, b = ops.pack_weight8(w), ops.pack_weight8(ops.quantize_rows_e4m3(w))
    assert torch.equal(a.data, b.data) and torch.equal(a.scale, b.scale) and (a.n, a.k) == (1024, 512)
    assert a.data.numel() == 1024 * 512                            # half the bytes of the 16-bit pack
    assert ops.pack_weight(w).data.numel() * 2 == 2 * a.data.numel()


# ---- item 6 ---------------------------------------------------------------------------------------------------------
def _check_exact(got, x, q, s, cols=None):
    """`want` = the fp64 product of x and q * s rounded once to the dtype."""
    if cols is not None:
        q, s, got = q[cols], s[cols], got[:, cols]
    w64 = q.view(torch.float8_e4m3fn).float().double() * s.double()[:, None]
    x64 = x.double().reshape(-1, x.shape[-1])
    want = (x64 @ w64.t()).to(got.dtype)
    acc_tol = 5.0 * 2.0 ** -24 * (x64.abs() @ w64.abs().t())
    diff = (got.double() - want.double()).abs()
    bound = _ulp(want) * 1.001 + acc_tol
    share = (got == want).double().mean().item()
    print(f"worst excess {(diff - bound).max().item():.3e}, equal share {share:.5f}")
    assert bool((diff <= bound).all()), f"worst excess {(diff - bound).max().item():.3e}"
    assert share >= 0.99, share


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [1, 17, 74])
@pytest.mark.parametrize("pow2", [True, False], ids=["pow2", "general_scale"])
def test_linear_w8_against_exact_product(N, K, M, pow2):
    from longspec_amd import ops
    for dtype in DTYPES:
        q, s = ops.quantize_rows_e4m3(_mk((N, K), N + K, 0.03, dtype), pow2=pow2)
        x = _mk((M, K), M + K, 1.0, dtype)
        _check_exact(ops.linear(x, ops.pack_weight8((q, s))), x, q, s)


@pytest.mark.parametrize("N,K,dtype", [(152064, 5120, torch.bfloat16), (128256, 4096, torch.float16)], ids=["qwq", "llama3"])
@pytest.mark.parametrize("M", [1, 74])
@pytest.mark.parametrize("pow2", [True, False], ids=["pow2", "general_scale"])
def test_lm_head_shapes_w8(N, K, dtype, M, pow2):
    from longspec_amd import ops
    q, s = ops.quantize_rows_e4m3(_mk((N, K), N + K, 0.03, dtype), pow2=pow2)
    x = _mk((M, K), M + K, 1.0, dtype)
    cols = torch.randperm(N, generator=torch.Generator().manual_seed(5))[:2000].cuda()
    _check_exact(ops.linear(x, ops.pack_weight8((q, s))), x, q, s, cols)


# ---- item 7 ---------------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch_w8():
    from longspec_amd import ops
    for (N, K) in [(4096, 4096), (14336, 4096), (4096, 14336), (512, 256)]:
        pw = ops.pack_weight8(_mk((N, K), 21, 0.03))
        x = _mk((74, K), 22)
        full = ops.linear(x, pw)
        for rows in (slice(0, 1), slice(5, 21), slice(40, 72)):
            assert torch.equal(ops.linear(x[rows], pw), full[rows])


@pytest.mark.parametrize("S", SPLITS)
@pytest.mark.parametrize("M", [1, 74])
def test_split_k_is_deterministic_w8(S, M):
    from longspec_amd import ops
    pw = ops.pack_weight8(_mk((1024, 4096), 11, 0.03))
    x = _mk((M, 4096), 12)
    y0 = ops.linear(x, pw, n_splits=S)
    for _ in range(5):
        assert torch.equal(ops.linear(x, pw, n_splits=S), y0)


def test_unsupported_requests_fail_loudly_w8():
    from longspec_amd import ops
    from longspec_amd._C import LongSpecHipError
    w = _mk((256, 256), 81)
    p8, p16 = ops.pack_weight8(w), ops.pack_weight(w)
    x = _mk((4, 256), 82)
    with pytest.raises(LongSpecHipError, match="plain library GEMM"):
        ops.linear(torch.zeros(81, 256, dtype=torch.float16, device="cuda"), p8)
    fold = ops.NormFold(torch.ones(256, dtype=torch.float16, device="cuda"), 1e-5, torch.ones(4, 4, device="cuda"))
    with pytest.raises(ValueError, match="8-bit"):
        ops.linear(x, p8, norm=fold)
    with pytest.raises(ValueError, match="8-bit"):
        ops.linear(x, p8, ssq_out=True)
    with pytest.raises(ValueError, match="all 8-bit or all 16-bit"):
        ops.linear_multi(x, [p8, p16])
    with pytest.raises(ValueError, match="all 8-bit or all 16-bit"):
        ops.linear_multi(x, [p16, p8])
    with pytest.raises(ValueError):
        ops.linear_multi(x, [ops.pack_weight8(w, rope=True), p8])           # rope layout handed to linear_multi
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 128, 2).float() / 128))
    cos, sin = ops.rope_cos_sin(torch.arange(4, device="cuda")[None], inv_freq.cuda(), 1.0, torch.float16)
    with pytest.raises(ValueError):
        ops.linear_qkv_rope(x, [p8], None, cos, sin)                        # plain layout handed to linear_qkv_rope
    with pytest.raises(ValueError):
        ops.mlp_gate_up(x, p8)                                              # not a gate/up pair
    with pytest.raises(ValueError):
        ops.linear(x, ops.pack_gate_up8(w, w))
    with pytest.raises(ValueError):
        ops.pack_weight8(_mk((64, 96), 83))                                 # K % 64
    # the C ABI refuses the folded norm by itself
    import ctypes as C
    from longspec_amd import _C
    d = _C.LinearDesc()
    y = torch.empty(4, 256, dtype=torch.float16, device="cuda")
    d.x, d.y, d.M, d.K, d.n_seg, d.dtype, d.ldx, d.ldy = x.data_ptr(), y.data_ptr(), 4, 256, 1, _C.LS_F16, 256, 256
    d.w[0], d.n[0] = p8.data.data_ptr(), 256
    d.norm_weight = fold.weight.data_ptr()
    assert _C.load().ls_linear_w8_workspace_bytes(C.byref(d)) == 0
    assert b"folded RMSNorm" in _C.load().ls_last_error()
