// logprob.hip -- log-probabilities of emitted tokens and their top-n alternatives (logprobs=; gfx950 / CDNA4).
//
// For a row of 16-bit TARGET logits x as the token was picked from them (behind ls_penalize_rows), a temperature T and
//   m = max_i x_i,   lse = ln sum_i exp((x_i - m) / T),   lp_j = (x_j - m) / T - lse        (fp32, every operation rounded once)
// ls_token_logprobs writes lp of one chosen column per row and the row's n largest logits -- ordered by (logit descending,
// column ascending), -0.0 == +0.0, the order of ls_argmax_rows -- with their lp.  Within a row lp is monotone in the logit, so
// that order is the order by log-probability, and the list entry of the chosen column is the same expression on the same
// floats: bit-equal.  The distribution is the tempered soft-max over the FULL vocabulary; a top-k / top-p cut of the sampler
// is not applied.
//
//   stage 1  grid (chunks of 8192 logits, rows * b): chunk max cm, chunk sum of exp((x - cm) / T) (0 when cm = -inf), and the
//            chunk's n largest logits (value, column), selected exactly as csrc/topk.hip selects them (two 256-bin histogram
//            levels on the ordered 16-bit pattern, two more on the column when the n-th value is shared);
//   stage 2  one workgroup per row: m over the chunk maxima, the chunk sums rescaled in chunk order, lse; the chunks'
//            candidates merged into the sorted top n (each wave extracts its n best with DPP reductions, wave 0 merges the four
//            lists); the chosen column's logit read once.
// A row's outputs depend on that row, its chosen id, T and n only: no sum crosses rows, no floating-point atomics.
//
// ls_logprob_commit moves the rows a round accepted to the output columns of the tokens they produced.
//
// The selection helpers below repeat those of topk.hip instead of sharing a header with it: that file's kernels stay as they
// compile today.
#include <math.h>

#include "ls_common.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_CHUNK = 8192;          // logits per stage-1 workgroup: 32 per thread
constexpr int LP_MAXN = 20;
constexpr int LP_MAX_CHUNKS = 64;       // vocab <= 524288: stage 2 holds the row's chunk records in LDS and 5 candidates a thread
constexpr int LP_OWN = LP_MAX_CHUNKS * LP_MAXN / LP_THREADS;      // 5
constexpr int LP_MAX_ROWS = 1024;

// record of (row, chunk): float max, float sum, then n x (float logit, int column; -inf, -1 = none), in no particular order
__device__ __forceinline__ float* lp_rec(float* ws, long row, int chunk, int nchunks, int n) {
    return ws + (row * nchunks + chunk) * (2 + 2 * n);
}

// 16-bit float pattern -> unsigned key that orders like the value (no NaNs on this path); -0.0 and +0.0 share the key 0x8000
__device__ __forceinline__ unsigned order_key(unsigned bits16) {
    return (bits16 & 0x8000u) ? 0x8000u - (bits16 & 0x7fffu) : (bits16 | 0x8000u);
}
// fp32 -> unsigned key that orders like the value, the two zeros on one key
__device__ __forceinline__ unsigned order_key32(float f) {
    const unsigned b = f == 0.f ? 0u : __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_mov(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xf, false);   // disabled lanes keep v
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long dpp_max64(unsigned long long v) {
    const unsigned lo = dpp_mov<CTRL, ROW_MASK>((unsigned)v), hi = dpp_mov<CTRL, ROW_MASK>((unsigned)(v >> 32));
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    return o > v ? o : v;
}
// wave-wide max of a 64-bit key through the DPP network: quad swaps, row rotations, row broadcasts; lane 63 holds the total
__device__ __forceinline__ unsigned long long wave_umax64(unsigned long long v) {
    v = dpp_max64<0xB1, 0xf>(v);      // quad_perm [1,0,3,2]
    v = dpp_max64<0x4E, 0xf>(v);      // quad_perm [2,3,0,1]
    v = dpp_max64<0x124, 0xf>(v);     // row_ror:4
    v = dpp_max64<0x128, 0xf>(v);     // row_ror:8
    v = dpp_max64<0x142, 0xa>(v);     // row_bcast:15 into rows 1 and 3
    v = dpp_max64<0x143, 0xc>(v);     // row_bcast:31 into rows 2 and 3
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
    return ((unsigned long long)hi << 32) | lo;
}

// Executed by wave 0 on a 256-bin histogram in LDS: the bin holding the `want`-th item (want >= 1) counted from the top
// (from_top) or from the bottom, and how many items lie strictly beyond it on that side.
__device__ __forceinline__ void find_bin(const int* hist, int want, bool from_top, int lane, int& bin, int& beyond) {
    int c[4], tot = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = hist[from_top ? 255 - (lane * 4 + j) : lane * 4 + j];
        tot += c[j];
    }
    int incl = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    const int excl = incl - tot;
    const bool here = excl < want && incl >= want;    // exactly one lane
    int b = 0, bey = 0;
    if (here) {
        int run = excl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (run < want && run + c[j] >= want) { b = lane * 4 + j; bey = run; }
            run += c[j];
        }
    }
    const unsigned long long mask = __ballot(here);
    const int src = mask ? __ffsll((long long)mask) - 1 : 0;
    b = __shfl(b, src);
    bey = __shfl(bey, src);
    bin = from_top ? 255 - b : b;
    beyond = bey;
}

// Stage 1: one workgroup per (chunk of 8192 logits, row of batch z).  TOPN = false (n == 0): max and sum only.
template <typename E, bool TOPN>
__global__ __launch_bounds__(LP_THREADS) void logprob_chunk_kernel(const typename E::T* __restrict__ logits, long stride_b,
                                                                   long stride_r, int rows, int V, float temperature, int n,
                                                                   float* __restrict__ ws) {
    __shared__ float s_red[8];
    __shared__ int s_hist[256];
    __shared__ int s_sel[4];          // [0] bin / threshold, [1] count beyond, [2] output cursor, [3] count in the bin
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, row = blockIdx.y;                 // row = z * rows + r
    const typename E::T* src = logits + (long)(row / rows) * stride_b + (long)(row % rows) * stride_r;
    const int base = chunk * LP_CHUNK;
    const int n_valid = min(LP_CHUNK, V - base);                    // >= 8: the grid has ceil(V / 8192) chunks

    uint32_t raw[16];                 // 32 logits as 16-bit patterns; element e = j*8 + i sits at column col0[j] + i
    int col0[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = base + (j * LP_THREADS + tid) * 8;
        col0[j] = c;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);                       // masked by column
        if (c < V) v = *reinterpret_cast<const uint4*>(src + c);    // V % 8 == 0: all-in or all-out
        raw[j * 4 + 0] = v.x; raw[j * 4 + 1] = v.y; raw[j * 4 + 2] = v.z; raw[j * 4 + 3] = v.w;
    }
    auto bits = [&](int e) -> unsigned { return (raw[e >> 1] >> ((e & 1) * 16)) & 0xffffu; };
    auto val = [&](int e) -> float {
        const unsigned short h = (unsigned short)bits(e);
        return E::to_f32(__builtin_bit_cast(typename E::T, h));
    };
    auto valid = [&](int e) -> bool { return col0[e >> 3] < V; };
    if (TOPN) {
        s_hist[tid] = 0;
        if (tid == 0) s_sel[2] = 0;
    }

    // ---- chunk max and sum of exp((x - max) / T)
    float m = -INFINITY;
#pragma unroll
    for (int e = 0; e < 32; ++e)
        if (valid(e)) m = fmaxf(m, val(e));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if (lane == 0) s_red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    float s = 0.f;
    if (m != -INFINITY) {             // (a chunk of -inf only adds nothing to the row; -inf - -inf would be NaN)
#pragma unroll
        for (int e = 0; e < 32; ++e)
            if (valid(e)) s += expf((val(e) - m) / temperature);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) s_red[4 + wave] = s;
    float* rec = lp_rec(ws, row, chunk, gridDim.x, n);
    if (!TOPN) {
        __syncthreads();
        if (tid == 0) {
            rec[0] = m;
            rec[1] = (s_red[4] + s_red[5]) + (s_red[6] + s_red[7]);
        }
        return;
    }
    const int kk = min(n, n_valid);

    // ---- level 1: high byte of the key
#pragma unroll
    for (int e = 0; e < 32; ++e)
        if (valid(e)) atomicAdd(&s_hist[order_key(bits(e)) >> 8], 1);
    __syncthreads();
    if (wave == 0) {
        int b, bey;
        find_bin(s_hist, kk, true, lane, b, bey);
        if (lane == 0) { s_sel[0] = b; s_sel[1] = bey; }
    }
    __syncthreads();
    const int hi = s_sel[0], above_hi = s_sel[1];
    __syncthreads();
    s_hist[tid] = 0;
    __syncthreads();
    // ---- level 2: low byte among the elements of that bin
#pragma unroll
    for (int e = 0; e < 32; ++e) {
        const unsigned key = order_key(bits(e));
        if (valid(e) && (int)(key >> 8) == hi) atomicAdd(&s_hist[key & 255u], 1);
    }
    __syncthreads();
    if (wave == 0) {
        int b, bey;
        find_bin(s_hist, kk - above_hi, true, lane, b, bey);
        if (lane == 0) { s_sel[0] = (hi << 8) | b; s_sel[1] = above_hi + bey; s_sel[3] = s_hist[b]; }
    }
    __syncthreads();
    const unsigned T = (unsigned)s_sel[0];          // key of the kk-th largest logit
    const int n_gt = s_sel[1];                      // logits strictly larger
    const int n_eq = s_sel[3];                      // logits equal to it
    const int need = kk - n_gt;                     // how many of the equal ones belong to the top n (>= 1)
    int col_limit = 0x7fffffff;                     // equal logits are taken up to this column
    if (need < n_eq) {                              // a tie at the boundary: the `need` smallest columns win
        __syncthreads();
        s_hist[tid] = 0;
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 32; ++e)
            if (valid(e) && order_key(bits(e)) == T) atomicAdd(&s_hist[(col0[e >> 3] + (e & 7) - base) >> 5], 1);
        __syncthreads();
        if (wave == 0) {
            int b, bey;
            find_bin(s_hist, need, false, lane, b, bey);
            if (lane == 0) { s_sel[0] = b; s_sel[1] = bey; }
        }
        __syncthreads();
        const int cb = s_sel[0], below = s_sel[1];
        __syncthreads();
        s_hist[tid] = 0;
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 32; ++e) {
            const int rc = col0[e >> 3] + (e & 7) - base;
            if (valid(e) && order_key(bits(e)) == T && (rc >> 5) == cb) atomicAdd(&s_hist[rc & 31], 1);
        }
        __syncthreads();
        if (wave == 0) {
            int b, bey;
            find_bin(s_hist, need - below, false, lane, b, bey);
            if (lane == 0) s_sel[0] = base + cb * 32 + b;
        }
        __syncthreads();
        col_limit = s_sel[0];
    }
    // ---- emit exactly kk candidates (any order; the cursor stays below kk <= n), pad with (-inf, -1) up to n
#pragma unroll
    for (int e = 0; e < 32; ++e) {
        const unsigned key = order_key(bits(e));
        const int c = col0[e >> 3] + (e & 7);
        if (valid(e) && (key > T || (key == T && c <= col_limit))) {
            const int slot = atomicAdd(&s_sel[2], 1);
            if (slot < n) {
                rec[2 + 2 * slot] = val(e);
                reinterpret_cast<int*>(rec)[3 + 2 * slot] = c;
            }
        }
    }
    if (tid < n - kk) {
        rec[2 + 2 * (kk + tid)] = -INFINITY;
        reinterpret_cast<int*>(rec)[3 + 2 * (kk + tid)] = -1;
    }
    if (tid == 0) {
        rec[0] = m;
        rec[1] = (s_red[4] + s_red[5]) + (s_red[6] + s_red[7]);
    }
}

// Stage 2: one workgroup per row (blockIdx.x = z * rows + r).
__global__ __launch_bounds__(LP_THREADS) void logprob_row_kernel(const void* __restrict__ logits, int dtype, long stride_b,
                                                                 long stride_r, int rows, int V, const int64_t* __restrict__ ids,
                                                                 long ids_stride_b, float temperature, int n, int nchunks,
                                                                 const float* __restrict__ ws, float* __restrict__ row_lp,
                                                                 float* __restrict__ row_top_val,
                                                                 int64_t* __restrict__ row_top_idx) {
    __shared__ float s_cm[LP_MAX_CHUNKS], s_cs[LP_MAX_CHUNKS];
    __shared__ unsigned long long s_w[4 * LP_MAXN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row = blockIdx.x;
    const int z = (int)(row / rows), r = (int)(row % rows);
    const int rec_f = 2 + 2 * n;
    const float* recs = ws + row * nchunks * rec_f;
    if (tid < nchunks) {
        const float2 ms = *reinterpret_cast<const float2*>(recs + (long)tid * rec_f);
        s_cm[tid] = ms.x;
        s_cs[tid] = ms.y;
    }
    // the candidates, issued before the barrier: (ordered key of the logit) << 32 | ~column; 0 = none
    const int ncand = nchunks * n;                                  // <= 256 * LP_OWN
    unsigned long long pk[LP_OWN];
    float2 ld[LP_OWN];
#pragma unroll
    for (int j = 0; j < LP_OWN; ++j) {
        const int id = min(j * LP_THREADS + tid, max(ncand - 1, 0));     // clamped: every load is unconditional
        const int c = n > 0 ? id / n : 0, slot = n > 0 ? id - c * n : 0;
        ld[j] = n > 0 ? *reinterpret_cast<const float2*>(recs + (long)c * rec_f + 2 + 2 * slot) : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < LP_OWN; ++j) {
        const int col = __float_as_int(ld[j].y);
        const unsigned long long key = ((unsigned long long)order_key32(ld[j].x) << 32) | (0xffffffffu - (unsigned)col);
        pk[j] = (j * LP_THREADS + tid < ncand && col >= 0) ? key : 0ull;
    }
    __syncthreads();
    // ---- max and log-sum-exp in fixed chunk order (every thread, on LDS broadcasts)
    float m = -INFINITY;
    for (int c = 0; c < nchunks; ++c) m = fmaxf(m, s_cm[c]);
    float s = 0.f;
    for (int c = 0; c < nchunks; ++c) s += s_cs[c] * expf((s_cm[c] - m) / temperature);
    const float lse = logf(s);
    // ---- the chosen column
    if (tid == 0) {
        const int64_t id = ids[(long)z * ids_stride_b + r];
        float lp = __builtin_nanf("");
        if (id >= 0 && id < V) {
            const long off = (long)z * stride_b + (long)r * stride_r + id;
            float x = dtype == LS_F16 ? ElemF16::to_f32(static_cast<const _Float16*>(logits)[off])
                                      : ElemBF16::to_f32(static_cast<const __bf16*>(logits)[off]);
            x = x == 0.f ? 0.f : x;                                 // -0.0 as +0.0, as the list's keys hold it
            lp = (x - m) / temperature - lse;
        }
        row_lp[row] = lp;
    }
    if (n == 0) return;
    // ---- each wave extracts its n best (no barrier), wave 0 merges the four sorted lists
    for (int i = 0; i < n; ++i) {
        unsigned long long b = pk[0];
#pragma unroll
        for (int j = 1; j < LP_OWN; ++j) b = pk[j] > b ? pk[j] : b;
        const unsigned long long w = wave_umax64(b);
        if (lane == 0) s_w[wave * LP_MAXN + i] = w;
#pragma unroll
        for (int j = 0; j < LP_OWN; ++j) pk[j] = pk[j] == w ? 0ull : pk[j];          // keys are unique (or 0)
    }
    __syncthreads();
    if (wave == 0) {
        unsigned long long mk[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int id = q * 64 + lane;
            mk[q] = id < 4 * n ? s_w[(id / n) * LP_MAXN + id % n] : 0ull;
        }
        for (int i = 0; i < n; ++i) {
            const unsigned long long b = mk[1] > mk[0] ? mk[1] : mk[0];
            const unsigned long long w = wave_umax64(b);
#pragma unroll
            for (int q = 0; q < 2; ++q) mk[q] = mk[q] == w ? 0ull : mk[q];
            if (lane == 0) {
                float v = -INFINITY;
                int64_t col = -1;
                if (w != 0ull) {
                    const unsigned k = (unsigned)(w >> 32);
                    const float x = __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
                    v = (x - m) / temperature - lse;
                    col = (int64_t)(0xffffffffu - (unsigned)w);
                }
                row_top_val[row * n + i] = v;
                row_top_idx[row * n + i] = col;
            }
        }
    }
}

// One workgroup per batch row: accepted row j -> output column base[z] + base_add + j.
__global__ __launch_bounds__(LP_THREADS) void logprob_commit_kernel(const float* __restrict__ row_lp,
                                                                    const float* __restrict__ row_top_val,
                                                                    const int64_t* __restrict__ row_top_idx, int rows, int n,
                                                                    const int64_t* __restrict__ map, int max_rows,
                                                                    const int64_t* __restrict__ num, long num_stride,
                                                                    const int32_t* __restrict__ base, int base_add,
                                                                    float* __restrict__ out_token, float* __restrict__ out_top_val,
                                                                    int64_t* __restrict__ out_top_idx, int out_cap) {
    const int z = blockIdx.x;
    int cnt = max_rows;
    if (num) {
        const int64_t c = num[(long)z * num_stride];
        cnt = c < 0 ? 0 : c < max_rows ? (int)c : max_rows;
    }
    const long b0 = (long)base[z] + base_add;
    const int per = n + 1;
    for (int i = threadIdx.x; i < cnt * per; i += LP_THREADS) {
        const int j = i / per, e = i - j * per;
        const int64_t src = map ? map[(long)z * max_rows + j] : j;
        const long dst = b0 + j;
        if (src < 0 || src >= rows || dst < 0 || dst >= out_cap) continue;
        const long s = (long)z * rows + src, d = (long)z * out_cap + dst;
        if (e == 0) {
            out_token[d] = row_lp[s];
        } else {
            out_top_val[d * n + e - 1] = row_top_val[s * n + e - 1];
            out_top_idx[d * n + e - 1] = row_top_idx[s * n + e - 1];
        }
    }
}

bool misaligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

}  // namespace

extern "C" {

size_t ls_token_logprobs_workspace_bytes(int b, int rows, int vocab, int n) {
    if (b < 1 || rows < 1 || vocab < 8 || n < 0 || n > LP_MAXN) return 0;
    const size_t nchunks = ((size_t)vocab + LP_CHUNK - 1) / LP_CHUNK;
    return (size_t)b * rows * nchunks * (2 + 2 * n) * sizeof(float);
}

int ls_token_logprobs(const void* logits, int b, int rows, int vocab, int dtype, int64_t stride_b, int64_t stride_r,
                      const int64_t* ids, int64_t ids_stride_b, float temperature, int n, float* row_lp, float* row_top_val,
                      int64_t* row_top_idx, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "ls_token_logprobs";
    if (!logits || !ids || !row_lp || !workspace) LS_FAIL(LS_ERR_INVALID_ARG, "%s: null pointer", what);
    if (dtype != LS_F16 && dtype != LS_BF16) LS_FAIL(LS_ERR_INVALID_ARG, "%s: dtype", what);
    if (n < 0 || n > LP_MAXN) LS_FAIL(LS_ERR_INVALID_ARG, "%s: n=%d (0..%d)", what, n, LP_MAXN);
    if (n > 0 && (!row_top_val || !row_top_idx)) LS_FAIL(LS_ERR_INVALID_ARG, "%s: null top-n outputs with n=%d", what, n);
    if (b < 1 || rows < 1 || (long)b * rows > LP_MAX_ROWS)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: b=%d rows=%d (rows * b must be 1..%d)", what, b, rows, LP_MAX_ROWS);
    if (vocab < 8 || vocab % 8 != 0 || stride_r % 8 != 0 || stride_b % 8 != 0 || stride_r < vocab || stride_b < 0 ||
        ids_stride_b < 0)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: vocab=%d strides %ld / %ld (multiples of 8, row stride >= vocab)", what, vocab,
                (long)stride_b, (long)stride_r);
    if (!(temperature > 0.f) || isinf(temperature)) LS_FAIL(LS_ERR_INVALID_ARG, "%s: temperature must be positive and finite", what);
    if (misaligned(logits, 16) || misaligned(ids, 8) || misaligned(row_lp, 4) || misaligned(row_top_val, 4) ||
        misaligned(row_top_idx, 8) || misaligned(workspace, 8))
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: misaligned pointer", what);
    const int nchunks = (vocab + LP_CHUNK - 1) / LP_CHUNK;
    if (nchunks > LP_MAX_CHUNKS) LS_FAIL(LS_ERR_UNSUPPORTED, "%s: vocab=%d (at most %d)", what, vocab, LP_MAX_CHUNKS * LP_CHUNK);
    if (workspace_bytes < ls_token_logprobs_workspace_bytes(b, rows, vocab, n)) LS_FAIL(LS_ERR_WORKSPACE, "%s: workspace too small", what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* ws = static_cast<float*>(workspace);
    const dim3 grid(nchunks, b * rows), block(LP_THREADS);
#define LP_STAGE1(E, TOPN)                                                                                                    \
    hipLaunchKernelGGL((logprob_chunk_kernel<E, TOPN>), grid, block, 0, s, static_cast<const typename E::T*>(logits), (long)stride_b, \
                       (long)stride_r, rows, vocab, temperature, n, ws)
    if (dtype == LS_F16) {
        if (n > 0) LP_STAGE1(ElemF16, true); else LP_STAGE1(ElemF16, false);
    } else {
        if (n > 0) LP_STAGE1(ElemBF16, true); else LP_STAGE1(ElemBF16, false);
    }
#undef LP_STAGE1
    LS_CHECK_LAUNCH("logprob_chunk_kernel");
    hipLaunchKernelGGL(logprob_row_kernel, dim3(b * rows), block, 0, s, logits, dtype, (long)stride_b, (long)stride_r, rows, vocab, ids,
                       (long)ids_stride_b, temperature, n, nchunks, ws, row_lp, row_top_val, row_top_idx);
    LS_CHECK_LAUNCH("logprob_row_kernel");
    return LS_OK;
}

int ls_logprob_commit(const float* row_lp, const float* row_top_val, const int64_t* row_top_idx, int b, int rows, int n,
                      const int64_t* map, int max_rows, const int64_t* num, int64_t num_stride, const int32_t* base, int base_add,
                      float* out_token, float* out_top_val, int64_t* out_top_idx, int out_cap, void* stream) {
    const char* what = "ls_logprob_commit";
    if (!row_lp || !base || !out_token) LS_FAIL(LS_ERR_INVALID_ARG, "%s: null pointer", what);
    if (n < 0 || n > LP_MAXN) LS_FAIL(LS_ERR_INVALID_ARG, "%s: n=%d (0..%d)", what, n, LP_MAXN);
    if (n > 0 && (!row_top_val || !row_top_idx || !out_top_val || !out_top_idx))
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: null top-n buffers with n=%d", what, n);
    if (b < 1 || rows < 1 || (long)b * rows > LP_MAX_ROWS || max_rows < 1 || max_rows > LP_MAX_ROWS || out_cap < 1 || num_stride < 0)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: b=%d rows=%d max_rows=%d out_cap=%d", what, b, rows, max_rows, out_cap);
    hipLaunchKernelGGL(logprob_commit_kernel, dim3(b), dim3(LP_THREADS), 0, static_cast<hipStream_t>(stream), row_lp, row_top_val,
                       row_top_idx, rows, n, map, max_rows, num, (long)num_stride, base, base_add, out_token, out_top_val,
                       out_top_idx, out_cap);
    LS_CHECK_LAUNCH("logprob_commit_kernel");
    return LS_OK;
}

}  // extern "C"
