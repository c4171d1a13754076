"""fp64 restatement of RMSNorm, the rotary table and the rotation (csrc/misc.hip), for the tests of their edges:
tests/test_norm_rope_oracle.py (CPU: the oracle against the goldens and oracle.ref_ops, and the proof that the cases have
teeth) and tests/test_gpu_norm_rope_edges.py (the kernels against it).  Plain torch on the CPU, nothing from longspec_amd.ops.

Every quantity is computed in fp64 and rounded to the storage dtype at the points where the reference rounds
(LlamaRMSNorm.forward, LlamaRotaryEmbedding.forward, apply_rotary_pos_emb); `round_to` rounds ONCE (torch's own
fp64 -> fp16 / bf16 cast goes through fp32 and rounds twice)."""
import torch

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
ULP = {F16: 2.0 ** -10, BF16: 2.0 ** -7}          # one unit in the last place, relative to the binade's lower end


def shape_id(shape):
    return "x".join(map(str, shape))


def round_to(x, dtype):
    """fp64 -> fp16 / bf16, round to nearest even, one rounding: fp64 -> fp32 with round-to-odd (the sticky bit kept in the
    last place: 24 bits >= 11 + 2), then the exact-enough fp32 -> dtype cast."""
    x = x.to(F64).contiguous()
    f = x.to(F32)
    inexact = torch.isfinite(f) & (f.double() != x)
    bits = f.view(torch.int32)
    step = torch.where(x.abs() > f.double().abs(), 1, -1).to(torch.int32)          # towards x: sign-magnitude bits
    bits = torch.where(inexact & ((bits & 1) == 0), bits + step, bits)
    return bits.view(F32).to(dtype)


# ---- RMSNorm ---------------------------------------------------------------------------------------------------------
WRONG_EPS = ("omitted", "outside_root", "over_hidden")


def rmsnorm64(x, w, eps, residual=None, dtype=None, wrong_eps=None):
    """s = dtype(residual + x) (rounded first, llama.py:492,498); y = dtype(w * dtype(s * rsqrt(mean(s^2) + eps))).
    Returns (y, s).  `eps` is taken as the fp32 number the reference and the kernel are handed.
    `wrong_eps` (CPU teeth test only): the three ways a kernel can get eps wrong without today's suite noticing --
    "omitted", "outside_root" (1 / (sqrt(mean) + eps)), "over_hidden" (eps / hidden)."""
    dtype = dtype or x.dtype
    s = x.to(dtype) if residual is None else round_to(residual.double() + x.double(), dtype)
    s64 = s.double()
    ms = s64.pow(2).mean(-1, keepdim=True)
    e = float(torch.tensor(eps, dtype=F32))
    if wrong_eps is None:
        rs = torch.rsqrt(ms + e)
    elif wrong_eps == "omitted":
        rs = torch.rsqrt(ms)
    elif wrong_eps == "outside_root":
        rs = 1.0 / (ms.sqrt() + e)
    elif wrong_eps == "over_hidden":
        rs = torch.rsqrt(ms + e / x.shape[-1])
    else:
        raise ValueError(wrong_eps)
    n = round_to(s64 * rs, dtype)
    return round_to(w.double() * n.double(), dtype), s


def rmsnorm_margin(got, want):
    """The bar of test_rmsnorm_shapes on the elements where `want` is finite: (worst |diff| in units of
    ulp * max(|want|, 1e-2), share of differing elements).  The bar itself: worst <= 2 and share < 1 %."""
    ulp = ULP[want.dtype]
    fin = torch.isfinite(want)
    g, w = got.double().cpu()[fin], want.double()[fin]
    if not bool(torch.isfinite(g).all()):
        return float("inf"), 1.0
    d = (g - w).abs()
    return (d / (ulp * w.abs().clamp(min=1e-2))).max().item(), (d > 0).double().mean().item()


def rmsnorm_bar_holds(got, want):
    worst, share = rmsnorm_margin(got, want)
    return torch.equal(torch.isfinite(got.cpu()), torch.isfinite(want)) and worst <= 2.0 and share < 0.01


# (rows, hidden): the dispatch of ls_rmsnorm_fwd each one reaches
NORM_SHAPES = [
    (3, 40),            # rows kernel, NCH 1, plain sum order
    (5, 1000),          # NCH 1, plain; 128 threads for 125 chunks: guarded tail
    (4, 4096),          # NCH 1, canonical order
    (3, 8200),          # NCH 2, plain, 576 threads, tail
    (2, 16384),         # NCH 2, canonical, full
    (2, 24584),         # NCH 4, plain, tail
    (2, 32768),         # NCH 4, canonical, 1024 threads: the largest the rows kernel takes
    (130, 512),         # prefill kernel
    (129, 1000),        # prefill kernel, tail
    (129, 32760),       # prefill kernel, its LDS row at the 64 KiB limit
]
# name -> (scale of the normalised row, eps); "zero_row": scale 1 with row 1 all zeros
NORM_REGIMES = {"control": (1.0, 1e-6), "below_eps": (2.0 ** -9, 1e-5), "eps_dominates": (2.0 ** -12, 1e-5),
                "zero_row": (1.0, 1e-5), "large": (200.0, 1e-6)}
EPS_SENSITIVE = ("below_eps", "eps_dominates")


def norm_inputs(rows, hidden, dtype, regime, residual):
    """(x, r or None, w, eps): with a residual, x and r carry the scale / sqrt(2) each, so that their sum has the regime's."""
    scale, eps = NORM_REGIMES[regime]
    g = torch.Generator().manual_seed(rows * 100003 + hidden)
    each = scale / 2 ** 0.5 if residual else scale
    x = (torch.randn((rows, hidden), generator=g) * each).to(dtype)
    r = (torch.randn((rows, hidden), generator=g) * each).to(dtype) if residual else None
    w = (1.0 + 0.1 * torch.randn((hidden,), generator=g)).to(dtype)
    if regime == "zero_row":
        x[1] = 0
        if residual:
            r[1] = 0
    return x, r, w, eps


def overflow_inputs(rows, hidden):
    """fp16 x, r, w, eps, the rows touched: ordinary N(0,1) data where a handful of r + x sums leave fp16 (+-120000 -> +-inf)
    in rows 0 and rows - 1; the rows between stay ordinary."""
    x, r, w, eps = norm_inputs(rows, hidden, F16, "control", True)
    hit = sorted({0, rows - 1})
    for row in hit:
        for j, sign in ((0, 1.0), (hidden // 2 + 1, -1.0), (hidden - 1, 1.0)):
            x[row, j] = r[row, j] = sign * 60000.0
    return x, r, w, eps, hit


# ---- rotary table and rotation -----------------------------------------------------------------------------------------
def rope_table64(pos, inv_freq, scaling, dtype):
    """pos [..., R] int64, inv_freq [64] fp32 -> cos, sin [..., R, 128]: f = fp32(pos) * inv_freq, an fp32 product as in
    the reference; cos / sin = dtype(fp32(cos64(f)) * fp32(scaling)), both halves the same."""
    f = (pos.to(F32).unsqueeze(-1) * inv_freq.to(F32)).double()
    k = torch.tensor(scaling, dtype=F32)
    c, s = (torch.cos(f).to(F32) * k).to(dtype), (torch.sin(f).to(F32) * k).to(dtype)
    return torch.cat((c, c), -1), torch.cat((s, s), -1)


def rope_apply_ref(x, cos, sin):
    """x [b, R, heads, 128], cos / sin [b or 1, R, 128]: dtype(dtype(x * cos) + dtype(rotate_half(x) * sin))."""
    dt = x.dtype
    x64, c, s = x.double(), cos.double().unsqueeze(2), sin.double().unsqueeze(2)
    rot = torch.cat((-x64[..., 64:], x64[..., :64]), -1)
    return round_to(round_to(x64 * c, dt).double() + round_to(rot * s, dt).double(), dt)


def rope_margin(got, want, scaling):
    """The bar of test_rope_golden, per dtype: (max |diff|, its bound: one ulp at the entries' magnitude -- 1e-3 for fp16
    as today, 2^-8 * scaling for bf16 --, share of differing entries; the bar: < 1e-3)."""
    d = (got.double().cpu() - want.double()).abs()
    bound = 1e-3 if want.dtype == F16 else 2.0 ** -8 * scaling
    return d.max().item(), bound, (d > 0).double().mean().item()


def same_values(got, want):
    """torch.equal that also holds NaN against NaN (and so every infinity against the same infinity)."""
    got = got.cpu()
    return torch.equal(got.isnan(), want.isnan()) and torch.equal(got.masked_fill(got.isnan(), 0), want.masked_fill(want.isnan(), 0))


# (b, R, Hq, Hk, table rows per position: b or 1)
ROPE_APPLY_SHAPES = [(1, 9, 4, 2, 1), (1, 5, 40, 8, 1), (2, 3, 1, 1, 2), (1, 7, 3, 0, 1), (3, 260, 2, 1, 1)]
EXTREME = {F16: 65504.0, BF16: 3e38}


def rope_apply_inputs(b, R, Hq, Hk, tb, dtype, inv_freq):
    """q [b,R,Hq,128], k [b,R,Hk,128] ~ N(0,1) with entries +-0 and +-EXTREME in both halves of the first and the last row,
    and the oracle's own table [tb,R,128] at scaling 0.8366 (so |cos| <= 1 is not what keeps a product finite)."""
    g = torch.Generator().manual_seed(b * 1009 + R * 31 + Hq * 7 + Hk)
    q = torch.randn((b, R, Hq, 128), generator=g).to(dtype)
    k = torch.randn((b, R, Hk, 128), generator=g).to(dtype)
    big = EXTREME[dtype]
    for t in (q, k):
        if t.shape[2] == 0:
            continue
        for row in (0, R - 1):
            t[0, row, 0, 0:4] = torch.tensor([0.0, -0.0, big, -big]).to(dtype)
            t[-1, row, -1, 64:68] = torch.tensor([big, -big, -0.0, 0.0]).to(dtype)
            t[-1, row, -1, 0:2] = big               # (x[j], x[64 + j]) both extreme: the two products add up past the format
            t[0, row, 0, 70] = -big                 # one extreme product next to an ordinary one
    pos = torch.stack([rope_positions(R, 77 + z)[0] for z in range(tb)])
    cos, sin = rope_table64(pos, inv_freq, 0.8366, dtype)
    return q, k, cos, sin


ROPE_ROWS = (1, 3, 5, 74, 260)
ROPE_SCALINGS = (1.0, 0.8366)
ROPE_SPECIAL = (2 ** 24 + 1, 0, 1, 131071, 131072, 262143)      # 2^24 + 1: float(pos) rounds, here and in the kernel alike


def rope_positions(rows, seed):
    """[1, rows] int64: the special positions first (as many as fit), then random ones below 262144."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.randint(0, 262144, (rows,), generator=g)
    n = min(rows, len(ROPE_SPECIAL))
    pos[:n] = torch.tensor(ROPE_SPECIAL[:n])
    return pos[None]
