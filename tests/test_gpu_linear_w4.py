"""ls_linear_w4_fwd (the skinny GEMM with MXFP4 weights) and its quantiser / packer.

Yardstick: the 4-bit launch is BIT-IDENTICAL to the 16-bit launch (ls_linear_fwd) on the de-quantised weight -- same launch
plan, same k order, and a conversion that is exact because every e2m1 value times 2^E (E in [-13, 13]) is a normal fp16 and a
bf16 number.  No tolerance is involved there.  Against the exact (fp64) product the rule is tests/test_gpu_linear.py's,
unchanged: the conversion adds no rounding.  The shapes are the smallest that reach every dispatch class of the launch ladder
(M <= 16, <= 32, above with 64-row and with 128-row slabs, ragged N, forced split counts), not the workload's."""
import pytest
import torch

from test_gpu_linear import _acc_tol, _check, _ulp  # noqa: F401  (the 16-bit rule, unchanged)

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
SHAPES = [(512, 256), (512, 896), (100, 192), (264, 640), (4096, 4096), (1024, 4096), (4096, 14336)]
MS = [1, 5, 16, 17, 32, 33, 74, 80]
SPLITS = [0, 1, 2, 3, 5, 8]
WSTD = {"std0.03": 0.03, "std4": 4.0}


def _mk(shape, seed, scale=1.0, dtype=torch.float16):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda") * scale).to(dtype)


def _deq(q, e, dtype):
    from longspec_amd import quant
    return quant.dequantize_blocks_mxfp4(q, e, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("N", [100, 264])
@pytest.mark.parametrize("K", [128, 192, 640, 4096])
def test_device_quantizer_equals_host_quantizer(dtype, N, K):
    from longspec_amd import ops, quant
    for std in (0.03, K ** -0.5, 4.0):
        w = _mk((N, K), N + K, std, dtype)
        w[3] = 0
        w[5] *= 2.0 ** -20                                   # below the lower clamp of the block exponent
        q, e = ops.quantize_blocks_mxfp4(w)
        hq, he = quant.quantize_blocks_mxfp4(w.cpu())
        assert torch.equal(e.cpu(), he), std
        assert torch.equal(q.cpu(), hq), std
        dead = w[5].float().view(-1, 32).abs().amax(1).cpu() == 0              # (fp16: a whole block may underflow to zero)
        assert bool((he[3] == 127).all()) and bool((he[5][~dead] == 114).all()) and bool((he[5][dead] == 127).all())
        assert not bool(dead.all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_in_kernel_conversion_and_layout(dtype):
    """A weight whose rows run through all 16 codes, with scale bytes that sweep every E in [-13, 13] across the blocks, times
    one-hot rows of x returns the de-quantised weight exactly: the fp4 -> f16 / bf16 conversion, the nibble order, the byte
    select and the place of every scale byte in the packed layout are right."""
    from longspec_amd import ops
    N, K = 128, 256
    n, k = torch.meshgrid(torch.arange(N), torch.arange(K), indexing="ij")
    code = (k + 5 * n + 3 * (k // 32)) % 16
    for r in range(N):
        assert len(set(code[r].tolist())) == 16
    q = (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8)
    blk = torch.arange(N)[:, None] * (K // 32) + torch.arange(K // 32)[None, :]
    e = (114 + (7 * blk) % 27).to(torch.uint8)                           # 7 and 27 coprime: every exponent, in every row position
    assert set(e.flatten().tolist()) == set(range(114, 141))
    want = _deq(q, e, dtype).cuda()                                      # [N, K]
    assert torch.equal(want.float().cpu(), _deq(q, e, torch.float32))
    pw = ops.pack_weight4((q.cuda(), e.cuda()))
    eye = torch.eye(K, dtype=dtype, device="cuda")
    for k0 in range(0, K, 64):
        for M in (64, 16, 1):
            y = ops.linear(eye[k0:k0 + M], pw)
            assert torch.equal(y, want[:, k0:k0 + M].t()), (k0, M)


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("dist", list(WSTD))
def test_linear_bit_identical_to_16bit_kernel(N, K, dtype, dist):
    """linear(x, pack_weight4(q, e)) == linear(x, pack_weight(deq(q, e))) bit for bit at every forced split count (and the
    automatic one), with and without bias and with the residual epilogue."""
    from longspec_amd import ops
    q, e = ops.quantize_blocks_mxfp4(_mk((N, K), N + K, WSTD[dist], dtype))
    p4, p16 = ops.pack_weight4((q, e)), ops.pack_weight(_deq(q, e, dtype))
    b = _mk((N,), 7, 0.1, dtype)
    n0 = ops.W4_CALLS
    for M in MS:
        x = _mk((M, K), M + K, 1.0, dtype)
        r = _mk((M, N), 6, 1.0, dtype)
        for S in SPLITS:
            for kw in ({}, {"bias": b}, {"bias": b, "residual": r}):
                y4, y16 = ops.linear(x, p4, n_splits=S, **kw), ops.linear(x, p16, n_splits=S, **kw)
                assert torch.equal(y4, y16), f"M={M} S={S} {sorted(kw)}: {(y4 != y16).sum().item()} of {y4.numel()} differ"
    assert ops.W4_CALLS - n0 == len(MS) * len(SPLITS) * 3


@pytest.mark.parametrize("dims", [(512, 128, 256), (4096, 1024, 4096)], ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("dist", list(WSTD))
def test_qkv_launches_bit_identical_to_16bit_kernel(dims, dtype, dist):
    from longspec_amd import ops
    Nq, Nkv, K = dims
    qs = [ops.quantize_blocks_mxfp4(_mk((n, K), 2 + i, WSTD[dist], dtype)) for i, n in enumerate((Nq, Nkv, Nkv))]
    bs = [_mk((n,), 7 + i, 0.5, dtype) for i, n in enumerate((Nq, Nkv, Nkv))]
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 128, 2).float() / 128))
    plain4, plain16 = [ops.pack_weight4(p) for p in qs], [ops.pack_weight(_deq(*p, dtype)) for p in qs]
    rope4 = [ops.pack_weight4(p, rope=i < 2) for i, p in enumerate(qs)]
    rope16 = [ops.pack_weight(_deq(*p, dtype), rope=i < 2) for i, p in enumerate(qs)]
    for M in MS:
        x = _mk((1, M, K), 1 + M, 1.0, dtype)
        cos, sin = ops.rope_cos_sin(torch.arange(1000, 1000 + M, device="cuda")[None], inv_freq.cuda(), 1.0, dtype)
        for S in SPLITS:
            for a, c in zip(ops.linear_multi(x, plain4, bs, n_splits=S), ops.linear_multi(x, plain16, bs, n_splits=S)):
                assert torch.equal(a, c), (M, S)
            for a, c in zip(ops.linear_qkv_rope(x, rope4, bs, cos, sin, n_splits=S), ops.linear_qkv_rope(x, rope16, bs, cos, sin, n_splits=S)):
                assert torch.equal(a, c), (M, S)
        (a,), (c,) = ops.linear_qkv_rope(x, rope4[:1], None, cos, sin), ops.linear_qkv_rope(x, rope16[:1], None, cos, sin)
        assert torch.equal(a, c)


@pytest.mark.parametrize("N,K", [(512, 256), (1536, 512), (14336, 4096)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("dist", list(WSTD))
def test_mlp_gate_up_bit_identical_to_16bit_kernel(N, K, dtype, dist):
    from longspec_amd import ops
    g = ops.quantize_blocks_mxfp4(_mk((N, K), 61, WSTD[dist], dtype))
    u = ops.quantize_blocks_mxfp4(_mk((N, K), 62, WSTD[dist], dtype))
    p4, p16 = ops.pack_gate_up4(g, u), ops.pack_gate_up(_deq(*g, dtype), _deq(*u, dtype))
    for M in MS:
        x = _mk((M, K), 63 + M, 0.25 if dist == "std4" else 1.0, dtype)
        for S in SPLITS:
            assert torch.equal(ops.mlp_gate_up(x, p4, n_splits=S), ops.mlp_gate_up(x, p16, n_splits=S)), (M, S)


def test_pack_from_16bit_weight_equals_pack_from_q_e():
    from longspec_amd import ops
    w = _mk((1024, 512), 3, 0.03)
    a, b = ops.pack_weight4(w), ops.pack_weight4(ops.quantize_blocks_mxfp4(w))
    assert torch.equal(a.data, b.data) and (a.n, a.k) == (1024, 512)
    assert a.data.numel() == 1024 * 512 * 17 // 32                 # 0.5 + 1/32 bytes per element
    assert a.data.numel() * 32 == ops.pack_weight8(w).data.numel() * 17


def _check_exact(got, x, q, e, cols=None):
    """`want` = the fp64 product of x and the de-quantised weight, rounded once to the dtype; the 16-bit rule."""
    if cols is not None:
        q, e, got = q[cols], e[cols], got[:, cols]
    w32 = _deq(q, e, torch.float32)
    want = (x.double().reshape(-1, x.shape[-1]) @ w32.double().t()).to(got.dtype)
    _check(got, want, _acc_tol(x, w32))


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [1, 17, 74])
def test_linear_w4_against_exact_product(N, K, M):
    from longspec_amd import ops
    for dtype in DTYPES:
        q, e = ops.quantize_blocks_mxfp4(_mk((N, K), N + K, 0.03, dtype))
        x = _mk((M, K), M + K, 1.0, dtype)
        _check_exact(ops.linear(x, ops.pack_weight4((q, e))), x, q, e)


@pytest.fixture(scope="module")
def lm_head_pack():
    from longspec_amd import ops
    q, e = ops.quantize_blocks_mxfp4(_mk((128256, 4096), 128256 + 4096, 0.03))
    return q, e, ops.pack_weight4((q, e))


@pytest.mark.parametrize("M", [1, 16])
def test_lm_head_shape_w4(lm_head_pack, M):
    from longspec_amd import ops
    q, e, pw = lm_head_pack
    x = _mk((M, 4096), M + 4096)
    cols = torch.randperm(128256, generator=torch.Generator().manual_seed(5))[:2000].cuda()
    _check_exact(ops.linear(x, pw), x, q, e, cols)


def test_rows_do_not_depend_on_the_batch_w4():
    from longspec_amd import ops
    for (N, K) in [(4096, 4096), (1024, 4096), (512, 256)]:
        pw = ops.pack_weight4(_mk((N, K), 21, 0.03))
        x = _mk((74, K), 22)
        full = ops.linear(x, pw)
        for rows in (slice(0, 1), slice(5, 21), slice(40, 72)):
            assert torch.equal(ops.linear(x[rows], pw), full[rows])


@pytest.mark.parametrize("S", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("M", [1, 74])
def test_split_k_is_deterministic_w4(S, M):
    from longspec_amd import ops
    pw = ops.pack_weight4(_mk((1024, 4096), 11, 0.03))
    x = _mk((M, 4096), 12)
    y0 = ops.linear(x, pw, n_splits=S)
    for _ in range(5):
        assert torch.equal(ops.linear(x, pw, n_splits=S), y0)


def test_unsupported_requests_fail_loudly_w4():
    import ctypes as C
    from longspec_amd import _C, ops
    from longspec_amd._C import LongSpecHipError
    w = _mk((256, 256), 81)
    p4, p8, p16 = ops.pack_weight4(w), ops.pack_weight8(w), ops.pack_weight(w)
    x = _mk((4, 256), 82)
    with pytest.raises(LongSpecHipError, match="plain library GEMM"):
        ops.linear(torch.zeros(81, 256, dtype=torch.float16, device="cuda"), p4)
    fold = ops.NormFold(torch.ones(256, dtype=torch.float16, device="cuda"), 1e-5, torch.ones(4, 4, device="cuda"))
    with pytest.raises(ValueError, match="4-bit"):
        ops.linear(x, p4, norm=fold)
    with pytest.raises(ValueError, match="4-bit"):
        ops.linear(x, p4, ssq_out=True)
    for mix in ([p4, p16], [p16, p4], [p4, p8], [p8, p4]):
        with pytest.raises(ValueError, match="one weight format per launch"):
            ops.linear_multi(x, mix)
    with pytest.raises(ValueError):
        ops.linear_multi(x, [ops.pack_weight4(w, rope=True), p4])           # rope layout handed to linear_multi
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 128, 2).float() / 128))
    cos, sin = ops.rope_cos_sin(torch.arange(4, device="cuda")[None], inv_freq.cuda(), 1.0, torch.float16)
    with pytest.raises(ValueError):
        ops.linear_qkv_rope(x, [p4], None, cos, sin)                        # plain layout handed to linear_qkv_rope
    with pytest.raises(ValueError):
        ops.mlp_gate_up(x, p4)                                              # not a gate/up pair
    with pytest.raises(ValueError):
        ops.linear(x, ops.pack_gate_up4(w, w))
    with pytest.raises(ValueError):
        ops.pack_weight4(_mk((64, 96), 83))                                 # K % 64
    # an exponent byte outside [114, 140]: a checkpoint quantised elsewhere with a wider range is refused, never mis-converted
    q, e = ops.quantize_blocks_mxfp4(w)
    for bad in (113, 141, 0, 255):
        e2 = e.clone()
        e2[200, 3] = bad
        with pytest.raises(LongSpecHipError, match="exponent"):
            ops.pack_weight4((q, e2))
        assert b"outside [114, 140]" in _C.load().ls_last_error()
    for ok in (114, 140):
        e2 = e.clone()
        e2[200, 3] = ok
        ops.pack_weight4((q, e2))
    # the C ABI refuses the folded norm and a K that is no multiple of 64 by itself
    lib = _C.load()
    d = _C.LinearDesc()
    y = torch.empty(4, 256, dtype=torch.float16, device="cuda")
    d.x, d.y, d.M, d.K, d.n_seg, d.dtype, d.ldx, d.ldy = x.data_ptr(), y.data_ptr(), 4, 256, 1, _C.LS_F16, 256, 256
    d.w[0], d.n[0] = p4.data.data_ptr(), 256
    assert lib.ls_linear_w4_workspace_bytes(C.byref(d)) > 0
    d.norm_weight = fold.weight.data_ptr()
    assert lib.ls_linear_w4_workspace_bytes(C.byref(d)) == 0
    assert b"folded RMSNorm" in lib.ls_last_error()
    d.norm_weight = None
    d.ssq_out = torch.empty(4, 4, device="cuda").data_ptr()
    assert lib.ls_linear_w4_fwd(C.byref(d), None, 0, None) != 0 and b"folded RMSNorm" in lib.ls_last_error()
    d.ssq_out = None
    d.K, d.ldx = 160, 160
    assert lib.ls_linear_w4_workspace_bytes(C.byref(d)) == 0 and b"multiple of 64" in lib.ls_last_error()
    assert lib.ls_linear_w4_packed_bytes(256, 160) == 0
    assert lib.ls_linear_w4_quantize(w.data_ptr(), 4, 48, _C.LS_F16, q.data_ptr(), e.data_ptr(), None) != 0
