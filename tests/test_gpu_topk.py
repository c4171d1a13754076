"""ls_logprob_topk / ls_argmax_rows against the reference's torch expression (llama_glide.py:1019-1064,1091)
on the CPU.  Indices are exact wherever the k-th and (k+1)-th values differ by more than the fp32 noise of the
log-sum-exp (different summation order: a few ulp of a value of magnitude ~10, i.e. <= 1e-5); values within 1e-5.

The exact-order cases take tests/topk_oracle.py as reference: fp64 values, ties to the smaller flat index.  Their inputs are
built so that the expected index list is unique (``expected_topk`` asserts that on the CPU before the GPU is called) and the
indices are compared with ``torch.equal``; random inputs go through ``check_topk``.  V = 8192 * (c - 1) + 8 * j: c stage-1
chunks, the last one j groups of 8 columns wide."""
import pytest
import torch

from conftest import record_margin
from topk_oracle import TOL, check_topk, expected_topk

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
GRID = torch.tensor([-3.0, -1.5, -0.25, 0.5, 1.0, 2.0, 2.5, 3.0])


def _v(c, j):
    return 8192 * (c - 1) + 8 * j


def _topk(logits, hist, k):
    from longspec_amd import ops
    gv, gi = ops.logprob_topk(logits.cuda(), hist.cuda() if hist is not None else None, k)
    return gv.cpu(), gi.cpu()


def _checked(gv, gi, logits, hist, k, what):
    """check_topk on batch element 0 of an answer, the observed value error recorded next to its bound."""
    err = check_topk(gv[0], gi[0], logits, hist, k)
    record_margin(what + " |value - fp64|", err, err, TOL)


def _exact(logits, hist, k, what):
    """logits [R, V], hist [R] or None: the kernel's indices equal the unique expected list; values within TOL of fp64."""
    want = expected_topk(logits, hist, k)                              # raises if the input does not pin the order down
    gv, gi = _topk(logits[None], hist[None] if hist is not None else None, k)
    assert gi.shape == (1, k) and gv.shape == (1, k)
    assert torch.equal(gi[0], want), f"indices {gi[0].tolist()} != expected {want.tolist()}"
    _checked(gv, gi, logits, hist, k, what)
    return gv, gi


def _ref(logits, history, k):
    lp = logits.float().log_softmax(dim=-1)
    if history is not None:
        lp = lp + history[:, :, None]
    return lp.view(lp.shape[0], -1).topk(dim=-1, k=k, largest=True, sorted=True), lp.view(lp.shape[0], -1)


@pytest.mark.parametrize("R,V,k", [(1, 128256, 4), (4, 128256, 16), (16, 128256, 16), (16, 152064, 16), (16, 32000, 16),
                                   (1, 512, 4), (16, 512, 16), (2, 512, 2), (8, 512, 8), (16, 8200, 16)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_logprob_topk(R, V, k, dtype):
    from longspec_amd import ops
    g = torch.Generator().manual_seed(R * 7 + V + k)
    logits = (torch.randn(1, R, V, generator=g) * 2.5).to(dtype)
    hist = None if R == 1 else -torch.rand(1, R, generator=g) * 3
    (rv, ri), flat = _ref(logits, hist, k)
    gv, gi = ops.logprob_topk(logits.cuda(), hist.cuda() if hist is not None else None, k)
    gv, gi = gv.cpu(), gi.cpu()
    assert torch.allclose(gv, rv, atol=1e-5, rtol=0)
    # the selected SET must be a valid top-k of the reference values (ties / 1e-6-close values may swap)
    assert torch.allclose(flat[0, gi[0]], rv[0], atol=1e-5, rtol=0)
    assert gi[0].unique().numel() == k
    clear = (rv[0, :-1] - rv[0, 1:]) > 2e-5            # positions whose order is unambiguous
    same = gi[0] == ri[0]
    unamb = torch.ones(k, dtype=torch.bool)
    unamb[:-1] &= clear
    unamb[1:] &= clear
    kth_gap = flat[0].topk(k + 1).values
    if (kth_gap[k - 1] - kth_gap[k]) <= 2e-5:
        unamb[-1] = False
    assert bool(same[unamb].all())
    _checked(gv, gi, logits, hist, k, "logprob_topk random")


def test_ties_go_to_the_smaller_index():
    from longspec_amd import ops
    V = 16384
    logits = torch.zeros(1, 3, V, dtype=torch.float16)
    logits[0, 1, 100] = logits[0, 1, 9000] = logits[0, 2, 5] = 4.0
    logits[0, 0, 77] = 2.0
    gv, gi = ops.logprob_topk(logits.cuda(), torch.zeros(1, 3).cuda(), 5)
    # row 2 has one 4.0 (smaller log-sum-exp -> larger log-prob); row 1's two 4.0 tie exactly: smaller index first
    # then row 0's 2.0, then a zero of row 0 (the smallest log-sum-exp of the three rows), column 0.  fp64 gaps >= 3e-3
    assert gi[0].tolist() == [2 * V + 5, 1 * V + 100, 1 * V + 9000, 77, 0]
    assert torch.equal(gi[0].cpu(), expected_topk(logits, torch.zeros(3), 5))
    _checked(gv.cpu(), gi.cpu(), logits, torch.zeros(3), 5, "logprob_topk ties")
    am = ops.argmax_rows(logits.cuda())
    assert am.tolist() == [[77, 100, 5]]


@pytest.mark.parametrize("R,V", [(1, 128256), (69, 128256), (74, 152064), (5, 512), (69, 32000)])
def test_argmax_rows(R, V):
    from longspec_amd import ops
    g = torch.Generator().manual_seed(R + V)
    logits = (torch.randn(1, R, V, generator=g) * 2.5).half()
    got = ops.argmax_rows(logits.cuda()).cpu()
    want = logits.argmax(dim=-1)
    # equal maxima (fp16 collisions): PyTorch-CPU and this kernel both return the first one
    assert torch.equal(got, want)


DUP_V = 8192 * 2 + 8


@pytest.mark.parametrize("R,V,k,W", [(1, 128256, 4, 8), (16, 128256, 16, 8), (16, 128256, 16, 3), (4, 152064, 16, 2), (16, 32000, 16, 8),
                                     (74, 128256, 1, 8), (74, 152064, 1, 2), (16, 512, 16, 2),
                                     # world sizes whose slot count (W * ceil(chunks / W)) exceeds the one-GPU chunk count: the empty
                                     # slots are dropped before stage 2, as dist.KVShard.head_select does
                                     (16, 152064, 16, 8), (16, 152064, 16, 3), (16, 128256, 16, 7),
                                     # duplicate-heavy rows (8-value grid): the k-th value is shared by hundreds of columns of every
                                     # chunk, on both sides of a rank boundary
                                     (16, DUP_V, 16, 2), (16, DUP_V, 16, 3), (74, DUP_V, 1, 2), (74, DUP_V, 1, 3)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_vocabulary_parallel_stages_are_bit_identical(R, V, k, W, dtype):
    """Round 3 (the lm_head sharded by vocabulary, dist.KVShard.head_select): stage 1 on each rank's slice of the logits, the
    ranks' chunk records concatenated in rank order, stage 2 on all of them -- values AND indices bit-identical to the one-GPU
    operators (log-soft-max top-k for k > 1 rows <= 16, arg-max for the 74-row verification pass), for 2, 3 and 8 ranks,
    including ranks that own no column at all (32000 = 4 chunks on 8 ranks; 512 = one chunk on 2)."""
    from longspec_amd import ops
    from longspec_amd.dist import KVShard
    g = torch.Generator().manual_seed(R + V + k + W)
    if V == DUP_V:
        logits = GRID[torch.randint(0, 8, (R, V), generator=g)].to(dtype)
    else:
        logits = (torch.randn(R, V, generator=g) * 2.5).to(dtype)
    logits[:, V // 3] = logits[:, 2 * V // 3]                     # exact ties across chunks (and ranks): index order decides
    cpu_logits = logits
    logits = logits.cuda()
    argmax = k == 1
    hist = None if (argmax or R == 1) else (-torch.rand(1, R, generator=g) * 3).cuda()
    if V == DUP_V and not argmax:
        exact = expected_topk(cpu_logits, hist.cpu(), k)
    if argmax:
        want = ops.argmax_rows(logits)
    else:
        want = ops.logprob_topk(logits.view(1, R, V), hist, k)
    recs, ncl = [], None
    for r in range(W):
        ncl, lo, hi = KVShard(r, W, 16).vocab_slice(V)
        buf = torch.full((ncl * R * (2 + 2 * k),), float("nan"), dtype=torch.float32, device="cuda")
        local = logits[:, lo:hi].contiguous() if hi > lo else None
        recs.append(ops.topk_stage1(local, R, k, lo, ncl, buf, dtype=dtype).clone())
    allrec = torch.cat(recs, dim=0).contiguous()
    assert allrec.shape == (W * ncl, R, 2 + 2 * k) and not torch.isnan(allrec[..., 0::2]).any()      # (odd fields past 1 are int columns)
    nchunks = (V + KVShard.VOCAB_CHUNK - 1) // KVShard.VOCAB_CHUNK
    got = ops.topk_stage2(allrec[:nchunks], R, V, k, hist.reshape(-1) if hist is not None else None, argmax)
    if argmax:
        assert torch.equal(got, want)
    else:
        assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])
    if V == DUP_V and argmax:
        assert torch.equal(got.cpu(), cpu_logits.float().argmax(-1))
    elif V == DUP_V:
        assert torch.equal(got[1][0].cpu(), exact)


@pytest.mark.parametrize("R,V,k,W", [(16, 152064, 16, 8), (16, 152064, 16, 3), (16, 128256, 16, 7), (16, 128256, 16, 8),
                                     (74, 128256, 1, 8), (16, 32000, 16, 2), (4, 152064, 16, 6)])
def test_head_select_end_to_end_equals_the_one_gpu_head(R, V, k, W):
    """ADVICE r3 (medium + low): ``KVShard.head_select`` itself -- sliced lm_head GEMM, stage 1, exchange, stage 2 -- against
    ``ops.linear`` on the FULL weight followed by the one-GPU selection, for world sizes whose slot count exceeds the one-GPU
    chunk count (QwQ at 3 / 6 / 8 ranks, Llama-3 at 7) and for slices whose own row count would make the launch planner split
    K (Llama-3's 13568-column tail at 8 ranks, Vicuna's 16000 columns at 2): tokens must not depend on the world size.  The W
    ranks are simulated in one process: every rank's send buffer is captured, then rank 0 merges them."""
    from longspec_amd import ops
    from longspec_amd.dist import KVShard
    Hd = 256
    g = torch.Generator().manual_seed(7 * R + V + k + W)
    lm = torch.nn.Linear(Hd, V, bias=False)
    with torch.no_grad():
        lm.weight.copy_(torch.randn(V, Hd, generator=g) * 0.05)
    lm = lm.half().cuda()
    x = torch.randn(1, R, Hd, generator=g).half().cuda()
    argmax = k == 1
    hist = None if argmax else (-torch.rand(1, R, generator=g) * 3).cuda()
    full = ops.linear(x.view(R, Hd), ops.pack_weight(lm.weight))
    want = ops.argmax_rows(full) if argmax else ops.logprob_topk(full.view(1, R, V), hist, k)
    sends = []

    class Capture(Exception):
        pass

    for r in range(W):
        sh = KVShard(r, W, 16)

        def grab(send, recv, _sh=sh):
            sends.append(send.clone())
            raise Capture()
        sh.exchange = grab
        try:
            sh.head_select(lm, x, ops, k=k, history=hist, argmax=argmax)
        except Capture:
            pass
    assert len(sends) == W
    sh0 = KVShard(0, W, 16)
    sh0.exchange = lambda send, recv: torch.stack(sends, dim=0)
    got = sh0.head_select(lm, x, ops, k=k, history=hist, argmax=argmax)
    if argmax:
        assert torch.equal(got.view(-1), want.view(-1))
    else:
        assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])


# ---- exact order: duplicate-heavy rows, engineered tie boundaries ------------------------------------------------------------

@pytest.mark.parametrize("R,V,k", [(1, 8192, 16), (4, 8200, 16), (16, 16392, 16), (8, 57352, 17), (10, 57352, 64)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicate_heavy_rows_exact_order(R, V, k, dtype):
    """Logits from an 8-value grid: the k-th value is shared by hundreds of columns in every chunk, so every chunk takes the
    boundary-tie path of stage 1 (histogram levels 3 and 4 on the column) and the merge sees k-fold ties."""
    g = torch.Generator().manual_seed(R + V + k)
    logits = GRID[torch.randint(0, 8, (R, V), generator=g)].to(dtype)
    hist = None if R == 1 else -torch.rand(R, generator=g) * 3
    _exact(logits, hist, k, "logprob_topk duplicate-heavy")


TIE_V = _v(3, 3)          # two full chunks and a tail of 24 columns
# (chunk, last winning column inside the chunk): column % 32 in {0, 31}; 32-column block 0, the middle, 255; the last 8-group of
# the partial tail (its first column and the last but one: a tied column must remain behind it); 8191 against 8192
TIE_CASES = [(0, 0), (0, 31), (0, 32), (1, 4127), (1, 4128), (0, 8160), (1, 8160), (0, 8190), (0, 8191), (1, 8191), (2, 16), (2, 22)]


@pytest.mark.parametrize("chunk,last", TIE_CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_tie_boundary_inside_a_chunk(chunk, last, dtype):
    """Row 0 is -2.0 except for a few 3.0 (strictly above the boundary) and a set of 1.0 (the boundary value) in one chunk, of
    which exactly those up to column `last` fit into the top k: more tied columns follow right behind it, in the next
    32-column block, at the chunk's end and in the next chunk."""
    V = TIE_V
    base = chunk * 8192
    n_valid = min(8192, V - base)
    before = sorted({last * f // 5 for f in range(1, 5)} | {last - 1})
    before = [c for c in before if 0 <= c < last]
    behind = sorted(c for c in {last + 1, last + 2, (last // 32 + 1) * 32, n_valid - 1} if last < c < n_valid)
    tied = before + [last] + behind
    above = [c for c in (3, 13, 40, 4001, 8100) if c < n_valid and c not in tied][:3]
    logits = torch.full((2, V), -2.0, dtype=dtype)
    logits[0, [base + c for c in tied]] = 1.0
    logits[0, [base + c for c in above]] = 3.0
    if base + 8192 < V:
        logits[0, base + 8192] = 1.0                                   # the first column of the next chunk ties too, and loses
    k = len(above) + len(before) + 1
    assert chunk == 2 or last == 8191 or len(behind) >= 1             # (8191: the tie is against column 8192, decided in stage 2)
    hist = torch.tensor([0.0, -5.0])
    gv, gi = _exact(logits, hist, k, "logprob_topk tie boundary")
    assert gi[0].tolist() == [base + c for c in above] + [base + c for c in before + [last]]


@pytest.mark.parametrize("V,k", [(8200, 16), (16392, 64)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_constant_rows_select_the_first_columns(V, k, dtype):
    logits = torch.full((3, V), 0.5, dtype=dtype)
    gv, gi = _exact(logits, None, k, "logprob_topk constant rows")
    assert gi[0].tolist() == list(range(k))


@pytest.mark.parametrize("dtype", DTYPES)
def test_identical_rows_interleave_smaller_row_first(dtype):
    V, k = 16392, 16
    g = torch.Generator().manual_seed(11)
    row = torch.randn(V, generator=g).to(dtype)
    cols = torch.randperm(V, generator=g)[:8]
    row[cols] = (6.0 + 0.25 * torch.arange(8)).to(dtype)               # eight distinct values above everything else
    logits = torch.stack([row, row, -row])
    hist = torch.tensor([-0.5, -0.5, -2.0])
    gv, gi = _exact(logits, hist, k, "logprob_topk identical rows")
    best = cols.flip(0)
    assert gi[0].tolist() == [int(c) + r * V for c in best for r in (0, 1)]
    assert torch.equal(gv[0, 0::2], gv[0, 1::2])


# ---- the merge kernel's instantiations and the edges of the fused kernel's budget ---------------------------------------------

def _planted(R, c, k, dtype, plant, tail=72):
    """Gaussian background of sigma 0.5 (maximum below 3) and k planted logits 9, 9.0625, ... (exact in bf16 up to 16): they are the
    top k, in an order that the rows' log-sum-exps and histories decide.  plant = "ends": the even ones in the first chunk of
    row 0 (first and last column of the chunk included), the odd ones in the short last chunk of the last row (last column
    of the row included) -- the first and the last record of the workspace; "single": all k in one (row, chunk) record in
    the middle."""
    V = 8192 * (c - 1) + tail
    g = torch.Generator().manual_seed(1000 * R + 10 * c + k + (plant == "single"))
    logits = (torch.randn(R, V, generator=g) * 0.5).to(dtype)
    vals = (9.0 + 0.0625 * torch.arange(k)).to(dtype)
    vals = vals[torch.randperm(k, generator=g)]
    hist = -1.0 - 2.0 * torch.rand(R, generator=g)
    if plant == "single":
        r, ch = R // 2, (c - 1) // 2
        cols = torch.randperm(8192 - 2, generator=g)[:k - 2] + 1
        cols = torch.cat([torch.tensor([0, 8191]), cols])[:k] + ch * 8192
        logits[r, cols] = vals
        hist[r] = -0.25
        flat = r * V + cols
    else:
        na = (k + 1) // 2
        ca = torch.cat([torch.tensor([0, 8191]), torch.randperm(8190, generator=g)[:na] + 1])[:na]
        cb = torch.cat([torch.tensor([V - 1, V - tail]), V - tail + 1 + torch.randperm(tail - 2, generator=g)])[:k - na]
        logits[0, ca] = vals[:na]
        logits[R - 1, cb] = vals[na:]
        hist[0], hist[R - 1] = -0.25, -0.4
        flat = torch.cat([ca, (R - 1) * V + cb])
    return logits, hist, flat


def _planted_case(R, c, k, dtype, plant):
    logits, hist, flat = _planted(R, c, k, dtype, plant)
    want = expected_topk(logits, hist, k)
    assert torch.equal(want.sort().values, flat.sort().values)         # the planted logits are the top k (a check of this input)
    gv, gi = _topk(logits[None], hist[None], k)
    assert torch.equal(gi[0], want), f"indices {gi[0].tolist()} != expected {want.tolist()}"
    _checked(gv, gi, logits, hist, k, f"logprob_topk planted R={R} c={c} k={k}")


# rows, chunks, k -> candidates: 1024 | 1088 (merge<4> | <8>), 2048 | 2176 (<8> | <16>), 4096 | 4352 (<16> | <20>), and the limits
# 5120 candidates (three ways) and 512 (row, chunk) pairs
FUSED = [(8, 8, 16), (8, 8, 17), (16, 8, 16), (16, 8, 17), (16, 16, 16), (16, 16, 17), (16, 20, 16), (10, 8, 64), (128, 4, 10)]
# just beyond: one more chunk (5376 candidates), 129 rows, k = 65, more than 512 pairs; V % 8 != 0 is its own test below
BEYOND = [(16, 21, 16), (129, 4, 8), (1, 2, 65), (128, 5, 8)]


@pytest.mark.parametrize("plant", ["ends", "single"])
@pytest.mark.parametrize("R,c,k", FUSED)
@pytest.mark.parametrize("dtype", DTYPES)
def test_merge_instantiations_and_budget_edges(R, c, k, dtype, plant):
    assert R * c * k <= 5120 and R * c <= 512 and R <= 128 and k <= 64
    _planted_case(R, c, k, dtype, plant)


@pytest.mark.parametrize("plant", ["ends", "single"])
@pytest.mark.parametrize("R,c,k", BEYOND)
@pytest.mark.parametrize("dtype", DTYPES)
def test_beyond_the_budget_the_library_path_gives_the_same_answer(R, c, k, dtype, plant):
    assert R * c * k > 5120 or R * c > 512 or R > 128 or k > 64
    _planted_case(R, c, k, dtype, plant)


@pytest.mark.parametrize("dtype", DTYPES)
def test_vocabulary_not_a_multiple_of_8(dtype):
    g = torch.Generator().manual_seed(5)
    R, V, k = 4, 8197, 16
    logits = (torch.randn(R, V, generator=g) * 2.5).to(dtype)
    hist = -torch.rand(R, generator=g) * 3
    gv, gi = _topk(logits[None], hist[None], k)
    _checked(gv, gi, logits, hist, k, "logprob_topk V % 8 != 0")


# ---- other logprob_topk cases -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_elements_are_independent(dtype):
    """b = 3: a launch per element over one shared workspace; every element equals its own call, bit for bit."""
    from longspec_amd import ops
    b, R, V, k = 3, 4, 16392, 16
    g = torch.Generator().manual_seed(21)
    logits = (torch.randn(b, R, V, generator=g) * 2.5).to(dtype)
    hist = -torch.rand(b, R, generator=g) * 3
    gv, gi = ops.logprob_topk(logits.cuda(), hist.cuda(), k)
    assert gv.shape == (b, k) and gi.shape == (b, k)
    for i in range(b):
        _checked(gv[i:i + 1].cpu(), gi[i:i + 1].cpu(), logits[i], hist[i], k, "logprob_topk batch")
        ov, oi = ops.logprob_topk(logits[i:i + 1].cuda(), hist[i:i + 1].cuda(), k)
        assert torch.equal(oi[0], gi[i]) and torch.equal(ov[0], gv[i])


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_history_is_no_history(dtype):
    R, V, k = 4, 8200, 16
    g = torch.Generator().manual_seed(22)
    logits = (torch.randn(1, R, V, generator=g) * 2.5).to(dtype)
    v0, i0 = _topk(logits, None, k)
    v1, i1 = _topk(logits, torch.zeros(1, R), k)
    assert torch.equal(i0, i1) and torch.equal(v0, v1)
    _checked(v0, i0, logits, None, k, "logprob_topk no history")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_row_with_history_minus_1e4_is_never_selected(dtype):
    R, V, k = 4, 8200, 64
    g = torch.Generator().manual_seed(23)
    logits = (torch.randn(R, V, generator=g) * 2.5).to(dtype)
    logits[2] += 8.0                                                   # the best logits by far, in the banned row
    hist = torch.tensor([-0.5, -1.0, -1e4, -2.0])
    gv, gi = _topk(logits[None], hist[None], k)
    assert bool((gi[0] // V != 2).all())
    _checked(gv, gi, logits, hist, k, "logprob_topk banned row")


@pytest.mark.parametrize("dtype", DTYPES)
def test_k_larger_than_a_row(dtype):
    """R = 4, V = 8, k = 16: every record holds 8 candidates and 8 sentinels."""
    g = torch.Generator().manual_seed(24)
    logits = (torch.randn(4, 8, generator=g) * 2.5).to(dtype)
    hist = -torch.rand(4, generator=g) * 3
    gv, gi = _topk(logits[None], hist[None], 16)
    _checked(gv, gi, logits, hist, 16, "logprob_topk k > V")


@pytest.mark.parametrize("R,V,k", [(3, 8216, 16), (5, 16400, 12)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_k_larger_than_the_tail_chunk(R, V, k, dtype):
    """The last chunk holds 24 / 16 columns, fewer than k, in several rows -- and holds the best logits."""
    g = torch.Generator().manual_seed(25 + R)
    logits = (torch.randn(R, V, generator=g) * 2.5).to(dtype)
    logits[:, V - 10:] += 12.0
    hist = -torch.rand(R, generator=g) * 3
    gv, gi = _topk(logits[None], hist[None], k)
    _checked(gv, gi, logits, hist, k, "logprob_topk k > tail")


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_negative_and_constant_chunks(dtype):
    """Row 1 lies at -1000 and below (log-soft-max is shift invariant: it competes like any other row), row 2's middle chunk
    is constant, row 0's first chunk is all negative."""
    R, V, k = 3, 16408, 16
    g = torch.Generator().manual_seed(26)
    logits = (torch.randn(R, V, generator=g) * 2.5).to(dtype)
    logits[0, :8192] = -logits[0, :8192].abs() - 1.0
    logits[1] = (-1008.0 - 60.0 * torch.rand(V, generator=g)).to(dtype)
    logits[1, [7, 9000, 16400]] = -1000.0                              # its three best, one per chunk: they lead the result
    logits[2, 8192:16384] = 1.5
    assert float(logits[1].max()) <= -1000
    hist = torch.tensor([-1.0, 0.0, -0.5])
    gv, gi = _topk(logits[None], hist[None], k)
    assert gi[0, :3].tolist() == [V + 7, V + 9000, V + 16400]
    _checked(gv, gi, logits, hist, k, "logprob_topk negative / constant chunks")


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_and_offset_views(dtype):
    """A view of a wider buffer (row stride V + 64, first column 8: aligned, read in place) and one starting 4 elements into a
    row (not 16-byte aligned: copied first) both give the contiguous call's bits.  The buffer around the view holds larger
    values than the view does."""
    from longspec_amd import ops
    R, V, k = 4, 16392, 16
    g = torch.Generator().manual_seed(27)
    logits = (torch.randn(1, R, V, generator=g) * 2.5).to(dtype)
    hist = (-torch.rand(1, R, generator=g) * 3).cuda()
    wv, wi = ops.logprob_topk(logits.cuda(), hist, k)
    _checked(wv.cpu(), wi.cpu(), logits, hist.cpu(), k, "logprob_topk contiguous")
    am = ops.argmax_rows(logits.cuda())
    assert torch.equal(am.cpu(), logits.float().argmax(-1))
    for off in (8, 4):
        buf = torch.full((1, R, V + 64), 100.0, dtype=dtype).cuda()
        view = buf[:, :, off:off + V]
        view.copy_(logits)
        assert not view.is_contiguous() and view.stride(1) == V + 64 and view.data_ptr() % 16 == (0 if off == 8 else 8)
        gv, gi = ops.logprob_topk(view, hist, k)
        assert torch.equal(gi, wi) and torch.equal(gv, wv)
        assert torch.equal(ops.argmax_rows(view), am)
        assert torch.equal(ops.argmax_rows(view[0]), am[0])


# ---- argmax_rows -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [8, 16, 8200, 24584])
@pytest.mark.parametrize("R", [1, 74, 300])
@pytest.mark.parametrize("dtype", DTYPES)
def test_argmax_rows_exact(R, V, dtype):
    """300 rows: two workgroups in the merge.  bf16 collides more often than fp16: first maximum."""
    from longspec_amd import ops
    g = torch.Generator().manual_seed(3 * R + V)
    logits = (torch.randn(R, V, generator=g) * 2.5).to(dtype)
    assert torch.equal(ops.argmax_rows(logits.cuda()).cpu(), logits.float().argmax(-1))


def _argmax_edge_rows(dtype):
    V = 24584
    g = torch.Generator().manual_seed(31)
    x = (-torch.rand(10, V, generator=g) * 4 - 1).to(dtype)            # all negative: row 9 stays as it is
    x[0, 8191] = x[0, 8192] = 3.0                                      # equal maxima on both sides of a chunk boundary
    x[1, 5] = x[1, 20000] = 3.0                                        # ... in the first and the last chunk
    x[2, 0] = 3.0                                                      # the maximum in column 0
    x[3, V - 1] = 3.0                                                  # ... in the last valid column of the partial tail
    x[4] = 0.75                                                        # all equal: 0
    x[5, 16384:] = 2.0                                                 # the whole tail chunk ties: its first column
    x[6, 8191] = 2.0                                                   # the last column of a full chunk
    x[7, V - 1] = x[7, 16383] = 2.5
    x[8] = -7.0
    want = [8191, 5, 0, V - 1, 0, 16384, 8191, 16383, 0]
    return x, want


@pytest.mark.parametrize("dtype", DTYPES)
def test_argmax_rows_edges(dtype):
    from longspec_amd import ops
    x, want = _argmax_edge_rows(dtype)
    ref = x.float().argmax(-1)
    assert ref[:9].tolist() == want
    assert torch.equal(ops.argmax_rows(x.cuda()).cpu(), ref)
    # the same rows, one at a time and as [2, 5, V]
    assert torch.equal(ops.argmax_rows(x[3:4].cuda()).cpu(), ref[3:4])
    assert torch.equal(ops.argmax_rows(x.view(2, 5, -1).cuda()).cpu(), ref.view(2, 5))


@pytest.mark.parametrize("V", [8200, 24584])
@pytest.mark.parametrize("dtype", DTYPES)
def test_argmax_rows_of_a_sliced_batch(V, dtype):
    """[2, 3, V][:, -2:, :], as the generation loop passes the last positions of a batch."""
    from longspec_amd import ops
    g = torch.Generator().manual_seed(32 + V)
    full = (torch.randn(2, 3, V, generator=g) * 2.5).to(dtype)
    full[:, 0, 7] = 50.0                                               # the rows that are sliced away hold the largest values
    got = ops.argmax_rows(full.cuda()[:, -2:, :])
    assert got.shape == (2, 2)
    assert torch.equal(got.cpu(), full[:, -2:, :].float().argmax(-1))


# ---- signed zeros: -0.0 == +0.0, the smaller index wins -----------------------------------------------------------------------

def _zero_rows(dtype):
    V = 8200
    x = torch.full((4, V), -1.0, dtype=dtype)
    x[0, 5], x[0, 40] = -0.0, 0.0                                      # inside one chunk (and one 8-column group apart)
    x[1, 5], x[1, 40] = 0.0, -0.0
    x[2, 8191], x[2, 8192] = -0.0, 0.0                                 # across a chunk boundary
    x[3, 100], x[3, 101] = -0.0, 0.0                                   # neighbours
    return x, [5, 5, 8191, 100], [40, 40, 8192, 101]


@pytest.mark.parametrize("dtype", DTYPES)
def test_signed_zeros_argmax(dtype):
    from longspec_amd import ops
    x, first, _ = _zero_rows(dtype)
    assert x.float().argmax(-1).tolist() == first and x.argmax(-1).tolist() == first
    assert ops.argmax_rows(x.cuda()).tolist() == first
    for r in range(4):
        assert ops.argmax_rows(x[r:r + 1].cuda()).tolist() == first[r:r + 1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_signed_zeros_logprob_topk(dtype):
    x, first, second = _zero_rows(dtype)
    for r in range(4):
        row = x[r:r + 1]
        gv, gi = _exact(row, None, 1, "logprob_topk signed zeros")
        assert gi[0].tolist() == [first[r]]
        gv, gi = _exact(row, None, 2, "logprob_topk signed zeros")
        assert gi[0].tolist() == [first[r], second[r]] and gv[0, 0] == gv[0, 1]
