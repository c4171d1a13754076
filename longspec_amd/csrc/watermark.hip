// watermark.hip -- the keyed green-list watermark on the TARGET's lm_head logits and its detector (watermark=; gfx950 / CDNA4).
// No counterpart in the reference.
//
// The table is one int32 buffer of LS_WATERMARK_TABLE_WORDS words (longspec_amd/watermark.py builds it once per decode state):
//   [0] h, the context length (1..LS_WATERMARK_MAX_CONTEXT)   [1] T = floor(gamma * 2^32) as bits   [2] delta as fp32 bits
//   [3] LS_WATERMARK_TABLE_WORDS   [4] key, low word   [5] key, high word   [6] [7] zero
// h is clamped to the layout before it counts anything.
//
// All arithmetic on unsigned 64-bit words (include/longspec_hip.h has the contract): fin = the SplitMix64 finaliser, the state
// of a context c_1 .. c_h is s = fin(key + M1) folded with s = fin((s ^ c_i) + M1), u(s, v) = fin(s + (v + 1) * M1), and v is
// green iff (u >> 32) < T.
//
//   watermark_rows_kernel    grid (slices of WM_SLICE ids, rows, batch), 256 threads.  Wave 0 assembles the row's path
//                            (select_path), takes the last h tokens of t = output_ids[z, :w] ++ path -- from the path's tail and,
//                            where the path is shorter, from the end of the committed columns --, folds them serially and leaves
//                            s in LDS; a row with m < h returns there.  Then every thread sweeps WM_ITERS groups of eight ids.
//                            The groups are 16-byte aligned IN MEMORY (a row is only 2-byte aligned: group g of a row whose
//                            address is `off` elements behind a 16-byte boundary holds the ids 8g - off .. 8g - off + 7), so a
//                            whole group is one 16-byte load and, if one of its ids is green, one 16-byte store; the groups
//                            that hang over the row's two ends go element by element.  x = s + (v + 1) * M1 is multiplied out
//                            once per thread and advances by additions from there.
//   watermark_score_kernel   grid (ceil(n / 256), batch), 256 threads, a thread per position: its own context state from the h
//                            ids in front of it, u, the flag and the hash; the counts by ballots, one integer atomic add per
//                            workgroup and counter on words the host function has zeroed in front of the launch.
#include "rule_rows.h"

namespace {

constexpr int WM_THREADS = 256, WM_WAVE = 64, WM_IDS = 8, WM_ITERS = 4;
constexpr int WM_GROUPS = WM_THREADS * WM_ITERS;             // groups of eight ids per workgroup
constexpr int WM_SLICE = WM_GROUPS * WM_IDS;                 // ids per workgroup
constexpr int WM_WORDS = 8, WM_MAX_CTX = 8, WM_MAX_EXTRA = LS_BAN_MAX_EXTRA;
static_assert(WM_WORDS == LS_WATERMARK_TABLE_WORDS, "watermark table layout");
static_assert(WM_MAX_CTX == LS_WATERMARK_MAX_CONTEXT && WM_MAX_CTX <= WM_WAVE, "watermark context");
constexpr unsigned long long WM_M1 = 0x9E3779B97F4A7C15ull, WM_M2 = 0xBF58476D1CE4E5B9ull, WM_M3 = 0x94D049BB133111EBull;

struct WmTable {
    unsigned long long key;
    unsigned T;
    float delta;
    int h;
};

struct WmRowsArgs {
    RuleRows rr;
    const int32_t* table;
    const int64_t* out;      // output_ids [b, width], row stride out_sb; null with width 0
    long out_sb;
    int width;
    RuleColumn col;          // w, clamped to 0..width
    RowExtras ex;            // C <= WM_MAX_EXTRA
};

struct WmScoreArgs {
    const int64_t* ids;      // [b, n], row stride sb
    long sb, n;
    const int32_t* lengths;  // [b] or null: n
    const int32_t* table;
    int* counts;             // [b, 2]: scored, green; zero at the launch
    signed char* flags;      // [b, n] dense or null
    unsigned long long* hashes;      // [b, n] dense or null
};

__device__ __forceinline__ WmTable read_table(const int32_t* t) {
    WmTable o;
    o.h = clampi(t[0], 1, WM_MAX_CTX);
    o.T = (unsigned)t[1];
    o.delta = __builtin_bit_cast(float, t[2]);
    o.key = (unsigned long long)(unsigned)t[4] | ((unsigned long long)(unsigned)t[5] << 32);
    return o;
}

__device__ __forceinline__ unsigned long long fin(unsigned long long z) {
    z = (z ^ (z >> 30)) * WM_M2;
    z = (z ^ (z >> 27)) * WM_M3;
    return z ^ (z >> 31);
}

// logits element `e` plus `delta`: fp32 add, round to nearest even; a NaN keeps its bits
__device__ __forceinline__ unsigned short marked(unsigned short e, float delta, bool f16) {
    if (f16) {
        const float x = (float)__builtin_bit_cast(_Float16, e);
        if (x != x) return e;
        return __builtin_bit_cast(unsigned short, (_Float16)(x + delta));
    }
    const float x = __builtin_bit_cast(float, (unsigned)e << 16);
    if (x != x) return e;
    unsigned u = __builtin_bit_cast(unsigned, x + delta);        // finite or an infinity
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

__global__ __launch_bounds__(WM_THREADS) void watermark_rows_kernel(const WmRowsArgs a) {
    __shared__ int64_t s_path[WM_MAX_EXTRA];
    __shared__ unsigned long long s_state;
    __shared__ int s_live;
    const int tid = threadIdx.x, lane = tid & 63;
    const int r = blockIdx.y, z = blockIdx.z;
    const WmTable t = read_table(a.table);
    int d = 0;
    if (tid < WM_WAVE) d = select_path(a.ex, z, r, lane, s_path);
    __syncthreads();
    if (tid < WM_WAVE) {
        const long w64 = rule_column(a.col, z);
        const int w = w64 < 0 ? 0 : w64 > a.width ? a.width : (int)w64;
        const int m = w + d;
        int64_t c = 0;                                             // lane i: t[m - h + i], from the path or the columns
        if (m >= t.h && lane < t.h) {
            const int i = m - t.h + lane;
            c = i >= w ? s_path[i - w] : a.out[(long)z * a.out_sb + i];          // (i < w only with w > 0: out is there)
        }
        unsigned long long s = fin(t.key + WM_M1);
        for (int i = 0; i < t.h; ++i) {
            const unsigned lo = __shfl((unsigned)c, i, WM_WAVE), hi = __shfl((unsigned)((unsigned long long)c >> 32), i, WM_WAVE);
            s = fin((s ^ ((unsigned long long)lo | ((unsigned long long)hi << 32))) + WM_M1);
        }
        if (lane == 0) {
            s_state = s;
            s_live = m >= t.h;
        }
    }
    __syncthreads();
    if (!s_live) return;                                           // (uniform) fewer than h tokens: the row keeps its bits

    const unsigned long long s = s_state;
    const bool f16 = a.rr.ninf == 0xfc00;
    const long V = a.rr.vocab;
    unsigned short* row = a.rr.logits + (long)z * a.rr.sb + (long)r * a.rr.sr;
    const int off = (int)((reinterpret_cast<uintptr_t>(row) >> 1) & 7);          // elements behind a 16-byte boundary
    const long v0 = ((long)blockIdx.x * WM_GROUPS + tid) * WM_IDS - off;       // the first id of the thread's first group (> -8)
    constexpr long STEP = (long)WM_THREADS * WM_IDS;
    uint4 q[WM_ITERS];
#pragma unroll
    for (int it = 0; it < WM_ITERS; ++it) {
        const long v = v0 + it * STEP;
        q[it] = make_uint4(0, 0, 0, 0);
        if (v >= 0 && v + WM_IDS <= V) q[it] = *reinterpret_cast<const uint4*>(row + v);
    }
    unsigned long long x = s + (unsigned long long)(v0 + 1) * WM_M1;             // of id v0; id v0 + j: x + j * M1
#pragma unroll
    for (int it = 0; it < WM_ITERS; ++it, x += (unsigned long long)STEP * WM_M1) {
        const long v = v0 + it * STEP;
        if (v >= V) continue;                                      // (behind the row: nothing)
        if (v >= 0 && v + WM_IDS <= V) {
            unsigned wd[4] = {q[it].x, q[it].y, q[it].z, q[it].w};
            bool any = false;
            unsigned long long xj = x;
#pragma unroll
            for (int j = 0; j < WM_IDS; ++j, xj += WM_M1) {
                const bool green = (unsigned)(fin(xj) >> 32) < t.T;
                const unsigned sh = 16 * (j & 1);
                const unsigned short e = (unsigned short)(wd[j >> 1] >> sh);
                const unsigned short ne = green ? marked(e, t.delta, f16) : e;
                wd[j >> 1] = (wd[j >> 1] & ~(0xffffu << sh)) | ((unsigned)ne << sh);
                any |= green;
            }
            if (any) *reinterpret_cast<uint4*>(row + v) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
        } else {
            // a group that hangs over the row's head (v < 0) or its tail: the ids inside [0, V), element by element
            unsigned long long xj = x;
#pragma unroll 1
            for (int j = 0; j < WM_IDS; ++j, xj += WM_M1) {
                const long vj = v + j;
                if (vj < 0 || vj >= V) continue;
                if ((unsigned)(fin(xj) >> 32) < t.T) row[vj] = marked(row[vj], t.delta, f16);
            }
        }
    }
}

__global__ __launch_bounds__(WM_THREADS) void watermark_score_kernel(const WmScoreArgs a) {
    __shared__ int s_cnt[2][WM_THREADS / WM_WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int z = blockIdx.y;
    const WmTable t = read_table(a.table);
    const long c = (long)blockIdx.x * WM_THREADS + tid;
    long len = a.n;
    if (a.lengths) {
        const long l = a.lengths[z];
        len = l < 0 ? 0 : l > a.n ? a.n : l;
    }
    const int64_t* x = a.ids + (long)z * a.sb;
    const bool scored = c >= t.h && c < len;
    unsigned long long u = 0;
    bool green = false;
    if (scored) {
        unsigned long long s = fin(t.key + WM_M1);
        for (int i = t.h; i >= 1; --i) s = fin((s ^ (unsigned long long)x[c - i]) + WM_M1);
        u = fin(s + ((unsigned long long)x[c] + 1ull) * WM_M1);
        green = (unsigned)(u >> 32) < t.T;
    }
    if (c < a.n) {
        if (a.flags) a.flags[(long)z * a.n + c] = scored ? (green ? 1 : 0) : -1;
        if (a.hashes) a.hashes[(long)z * a.n + c] = u;
    }
    const int ns = __popcll(__ballot(scored)), ng = __popcll(__ballot(green));
    if (lane == 0) {
        s_cnt[0][wave] = ns;
        s_cnt[1][wave] = ng;
    }
    __syncthreads();
    if (tid < 2) {                                                 // integer adds: the sums do not depend on their order
        int tot = 0;
#pragma unroll
        for (int k = 0; k < WM_THREADS / WM_WAVE; ++k) tot += s_cnt[tid][k];
        if (tot != 0) atomicAdd(a.counts + 2 * z + tid, tot);
    }
}

}  // namespace

extern "C" {

int ls_watermark_rows(void* logits, int b, int rows, int vocab, int dtype, int64_t stride_b, int64_t stride_r, const int32_t* table,
                      int table_words, const int64_t* output_ids, int64_t out_stride_b, int width, const int32_t* base,
                      const int32_t* base_sub, int base_add, const int64_t* extra_ids, int64_t ids_stride_b, const int64_t* extra_mask,
                      int64_t mask_stride_b, int64_t mask_stride_r, int n_extra, void* stream) {
    const char* what = "ls_watermark_rows";
    WmRowsArgs a;
    if (int rc = rule_rows_check(what, logits, table != nullptr, b, rows, vocab, dtype, stride_b, stride_r, a.rr)) return rc;
    if (table_words != LS_WATERMARK_TABLE_WORDS)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: the watermark table has %d words, not %d", what, table_words, LS_WATERMARK_TABLE_WORDS);
    if (width < 0 || width > (1 << 23) || (width > 0 && (!output_ids || out_stride_b < width)))
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: width=%d (0..2^23) needs output_ids with a row stride %ld >= width", what, width, (long)out_stride_b);
    if (int rc = row_extras_check(what, extra_ids, ids_stride_b, extra_mask, mask_stride_b, mask_stride_r, n_extra, LS_BAN_MAX_EXTRA, a.ex))
        return rc;
    a.table = table; a.out = width > 0 ? output_ids : nullptr; a.out_sb = width > 0 ? (long)out_stride_b : 0l; a.width = width;
    a.col = RuleColumn{base, base_sub, base_add};
    // (a row may start up to 7 elements behind a 16-byte boundary: its groups cover vocab + 7 ids at the most)
    const long slices = ((long)vocab + (WM_IDS - 1) + WM_SLICE - 1) / WM_SLICE;
    const dim3 grid((unsigned)slices, rows, b), block(WM_THREADS);
    hipLaunchKernelGGL(watermark_rows_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
    LS_CHECK_LAUNCH("watermark_rows_kernel");
    return LS_OK;
}

int ls_watermark_score(const int64_t* ids, int b, int64_t n, int64_t stride_b, const int32_t* lengths, const int32_t* table,
                       int table_words, int32_t* counts, int8_t* flags, uint64_t* hashes, void* stream) {
    const char* what = "ls_watermark_score";
    if (!table || !counts || (n > 0 && !ids)) LS_FAIL(LS_ERR_INVALID_ARG, "%s: null pointer", what);
    if (table_words != LS_WATERMARK_TABLE_WORDS)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: the watermark table has %d words, not %d", what, table_words, LS_WATERMARK_TABLE_WORDS);
    if (b < 1 || b > 65535 || n < 0 || n > 0x7fffffffl || stride_b < (b > 1 ? n : 0))
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: b=%d (1..65535) n=%ld (0..2^31-1) row stride %ld (>= n)", what, b, (long)n, (long)stride_b);
    if (reinterpret_cast<uintptr_t>(counts) % 4 != 0 || reinterpret_cast<uintptr_t>(hashes) % 8 != 0)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: misaligned counts or hashes", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(counts, 0, sizeof(int32_t) * 2 * (size_t)b, st) != hipSuccess) {
        (void)hipGetLastError();
        LS_FAIL(LS_ERR_LAUNCH, "%s: clearing the counts failed", what);
    }
    if (n == 0) return LS_OK;
    WmScoreArgs a{ids, (long)stride_b, (long)n, lengths, table, counts, reinterpret_cast<signed char*>(flags),
                  reinterpret_cast<unsigned long long*>(hashes)};
    const dim3 grid((unsigned)((n + WM_THREADS - 1) / WM_THREADS), b), block(WM_THREADS);
    hipLaunchKernelGGL(watermark_score_kernel, grid, block, 0, st, a);
    LS_CHECK_LAUNCH("watermark_score_kernel");
    return LS_OK;
}

}  // extern "C"
