// guide.hip -- guided decoding: a token-level DFA on the TARGET's lm_head logits (guide=; gfx950 / CDNA4).  No counterpart in
// the reference.
//
// The guide table is one int32 buffer (longspec_amd/guide.py builds it once per decode state), 16-byte aligned:
//   [0] S   [1] C (1..16384)   [2] start   [3] vocab   [4] the word count   [5 : 8] reserved
//   [8 : 8 + K]   the classes of ids 0 .. vocab - 1, 16 bits each, two per word, 0xFFFF = forbidden; K = ceil(vocab / 2) rounded
//                 up to a multiple of 4 words, so that what follows is 16-byte aligned
//   [8 + K : 8 + K + S * C]   next, int32 [S, C]: the state behind a token of class c in state s, -1 = none
// A header whose areas do not fit table_words is refused as a whole (every row dead, every state -1); a class >= C counts as
// forbidden and a state outside [-1, S) as -1: nothing read from the table indexes memory unclamped.
//
//   guide_rows_kernel     grid (slices of LS_GUIDE_SLICE ids, rows, batch), 256 threads.  Every workgroup redoes its row's walk: wave 0
//                         assembles the row's ordered path in LDS (select_path, rule_rows.h), the workgroup looks the classes
//                         of all path tokens up in parallel, a lane per position, and follows the chain through next, the one
//                         serial part (measured: 1.2-1.6 us of the kernel's 11-13, less than the launch a pre-pass would add).
//                         A dead row: the workgroup returns.  Then the workgroup packs next[s, :] into C allow bits in LDS (a
//                         ballot per 64 classes) and streams its slice: 16 bytes of classes in, and per group of eight ids
//                         nothing (all allowed), one 16-byte store of the -inf pattern (all forbidden, the address aligned) or
//                         16-bit stores of the forbidden ones.  The logits are never read.
//   guide_advance_kernel  one wave per batch row: the classes of the accepted ids in parallel, the chain serially.
// No scratch, no atomics, no floating-point arithmetic.
#include "rule_rows.h"

namespace {

constexpr int GD_THREADS = 256, GD_WAVE = 64;
constexpr int GD_MAX_EXTRA = LS_GUIDE_MAX_EXTRA, GD_MAX_C = LS_GUIDE_MAX_CLASSES, GD_HDR = LS_GUIDE_HEADER_WORDS;
constexpr int GD_SLICE = LS_GUIDE_SLICE, GD_GROUPS = GD_SLICE / 8;          // ids / 16-byte class groups per workgroup
constexpr int GD_NO_CLASS = LS_GUIDE_NO_CLASS;
static_assert(GD_GROUPS % GD_THREADS == 0 && GD_MAX_C % 64 == 0 && GD_HDR % 4 == 0 && GD_MAX_EXTRA % GD_WAVE == 0, "guide tiling");

// The table's header, every field checked against table_words; ok == false: nothing else of the table is read.
struct GuideTable {
    bool ok;
    int S, C, vocab;                 // vocab: ids at and beyond it have no class
    const unsigned short* cls;       // [vocab] (padded to a multiple of 8)
    const int32_t* next;             // [S, C]
};

__device__ __forceinline__ GuideTable read_header(const int32_t* table, int table_words) {
    GuideTable t;
    t.S = table[0]; t.C = table[1]; t.vocab = table[3];
    t.ok = t.S >= 1 && t.C >= 1 && t.C <= GD_MAX_C && t.vocab >= 1 && t.vocab < (1 << 30) && (long)t.S * t.C <= (long)LS_GUIDE_MAX_CELLS;
    const int K = t.ok ? (((t.vocab + 1) / 2 + 3) / 4) * 4 : 0;
    t.ok = t.ok && (long)GD_HDR + K + (long)t.S * t.C <= (long)table_words;
    t.cls = reinterpret_cast<const unsigned short*>(table + GD_HDR);
    t.next = table + GD_HDR + K;
    return t;
}

// The class of a path token as an index into next's rows, or -1: outside [0, vocab), forbidden, or a class the table does not have.
__device__ __forceinline__ int class_of(const GuideTable& t, int64_t id, int vocab) {
    if (id < 0 || id >= (int64_t)vocab) return -1;
    const int c = t.cls[id];
    return c < t.C ? c : -1;
}

// s walked along cls[0 .. d-1] (classes in LDS, -1 = forbidden).  Every lane computes the same chain.
__device__ __forceinline__ int follow(const GuideTable& t, int s, const int* cls, int d) {
    if (s < -1 || s >= t.S) s = -1;
    for (int q = 0; q < d && s >= 0; ++q) {
        const int c = cls[q];
        if (c < 0) { s = -1; break; }
        const int nx = t.next[(long)s * t.C + c];
        s = nx >= 0 && nx < t.S ? nx : -1;
    }
    return s;
}

struct GuideRowsArgs {
    RuleRows rr;
    const int32_t* table;
    int table_words;
    const int32_t* state;    // [b]
    RowExtras ex;            // C <= GD_MAX_EXTRA
};

__global__ __launch_bounds__(GD_THREADS) void guide_rows_kernel(const GuideRowsArgs a) {
    __shared__ int64_t s_path[GD_MAX_EXTRA];
    __shared__ int s_cls[GD_MAX_EXTRA];
    __shared__ unsigned s_allow[GD_MAX_C / 32];
    __shared__ int s_depth;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.y, z = blockIdx.z;
    const GuideTable t = read_header(a.table, a.table_words);
    if (!t.ok) return;                                             // (uniform)
    const int V = a.rr.vocab, tv = t.vocab < V ? t.vocab : V;         // ids in [tv, V) have no class: forbidden

    // ---- the row's state: the committed state walked along the row's path
    if (wave == 0) {
        const int d = select_path(a.ex, z, r, lane, s_path);
        if (lane == 0) s_depth = d;
    }
    __syncthreads();
    const int d = s_depth;
    if (tid < d) s_cls[tid] = class_of(t, s_path[tid], tv);        // d <= GD_MAX_EXTRA <= GD_THREADS: a lane per position
    __syncthreads();
    const int s = follow(t, a.state[z], s_cls, d);                 // (every lane the same chain: uniform loads)
    if (s < 0) return;                                             // a dead row keeps its bits (uniform)

    // ---- the state's allow bits: bit c = next[s, c] is a state
    const int32_t* nrow = t.next + (long)s * t.C;
    for (int c0 = wave * GD_WAVE; c0 < t.C; c0 += GD_THREADS) {
        const int c = c0 + lane;
        const int nx = c < t.C ? nrow[c] : -1;
        const unsigned long long bal = __ballot(nx >= 0 && nx < t.S);
        if (lane == 0) { s_allow[c0 >> 5] = (unsigned)bal; s_allow[(c0 >> 5) + 1] = (unsigned)(bal >> 32); }
    }
    __syncthreads();

    // ---- the slice: ids [g * 8, g * 8 + 8) per group
    unsigned short* row = a.rr.logits + (long)z * a.rr.sb + (long)r * a.rr.sr;
    const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15) == 0;        // then every group of the row is 16-byte aligned
    const unsigned short ninf = a.rr.ninf;
    const unsigned nn = (unsigned)ninf * 0x00010001u;
    const int g0 = blockIdx.x * GD_GROUPS, groups = (V + 7) >> 3, full_cls = tv >> 3;    // groups < full_cls: eight classes to read
#pragma unroll 4
    for (int p = 0; p < GD_GROUPS / GD_THREADS; ++p) {
        const int g = g0 + p * GD_THREADS + tid;
        if (g >= groups) continue;
        const int v0 = g << 3;
        unsigned forbid = 0;                                       // bit i: id v0 + i is forbidden
        if (g < full_cls) {
            const uint4 w = *reinterpret_cast<const uint4*>(t.cls + v0);      // 16-byte aligned: the table is, and the class area
            const unsigned ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const unsigned c = (ws[i >> 1] >> ((i & 1) * 16)) & 0xffffu;
                const bool ok = c < (unsigned)t.C && ((s_allow[c >> 5] >> (c & 31)) & 1u);
                forbid |= (ok ? 0u : 1u) << i;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int v = v0 + i;
                bool ok = false;
                if (v < tv) {
                    const unsigned c = t.cls[v];
                    ok = c < (unsigned)t.C && ((s_allow[c >> 5] >> (c & 31)) & 1u);
                }
                forbid |= (ok ? 0u : 1u) << i;
            }
        }
        const int left = V - v0;                                   // >= 1
        if (left < 8) forbid &= (1u << left) - 1u;                 // the ragged tail: nothing at or beyond V
        if (forbid == 0) continue;
        if (forbid == 0xffu && aligned) {
            *reinterpret_cast<uint4*>(row + v0) = make_uint4(nn, nn, nn, nn);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if ((forbid >> i) & 1u) row[v0 + i] = ninf;
        }
    }
}

struct GuideAdvanceArgs {
    int32_t* state;          // [b]
    const int32_t* table;
    int table_words;
    const int64_t* ids;      // [b, n], row stride ids_sb
    long ids_sb;
    const int64_t* num;      // [b] with stride num_s, or null: n
    long num_s;
    int n;
};

__global__ __launch_bounds__(GD_WAVE) void guide_advance_kernel(const GuideAdvanceArgs a) {
    __shared__ int s_cls[GD_MAX_EXTRA];
    const int lane = threadIdx.x, z = blockIdx.x;
    const GuideTable t = read_header(a.table, a.table_words);
    if (!t.ok) {
        if (lane == 0) a.state[z] = -1;
        return;
    }
    int64_t m = a.num ? a.num[(long)z * a.num_s] : (int64_t)a.n;
    const int d = m < 0 ? 0 : m > a.n ? a.n : (int)m;              // n <= GD_MAX_EXTRA
    const int64_t* ids = a.ids + (long)z * a.ids_sb;
    for (int q = lane; q < d; q += GD_WAVE) s_cls[q] = class_of(t, ids[q], t.vocab);
    __syncthreads();
    const int s = follow(t, a.state[z], s_cls, d);
    if (lane == 0) a.state[z] = s;
}

}  // namespace

extern "C" {

int ls_guide_rows(void* logits, int b, int rows, int vocab, int dtype, int64_t stride_b, int64_t stride_r, const int32_t* table,
                  int table_words, const int32_t* state, const int64_t* extra_ids, int64_t ids_stride_b, const int64_t* extra_mask,
                  int64_t mask_stride_b, int64_t mask_stride_r, int n_extra, void* stream) {
    const char* what = "ls_guide_rows";
    GuideRowsArgs a;
    if (int rc = rule_rows_check(what, logits, table && state, b, rows, vocab, dtype, stride_b, stride_r, a.rr)) return rc;
    if (table_words < LS_GUIDE_HEADER_WORDS || reinterpret_cast<uintptr_t>(table) % 16 != 0)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: the guide table has %d words (at least %d) and is 16-byte aligned", what, table_words,
                LS_GUIDE_HEADER_WORDS);
    if (int rc = row_extras_check(what, extra_ids, ids_stride_b, extra_mask, mask_stride_b, mask_stride_r, n_extra, LS_GUIDE_MAX_EXTRA, a.ex))
        return rc;
    a.table = table; a.table_words = table_words; a.state = state;
    const dim3 grid((unsigned)((vocab + GD_SLICE - 1) / GD_SLICE), rows, b), block(GD_THREADS);
    hipLaunchKernelGGL(guide_rows_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
    LS_CHECK_LAUNCH("guide_rows_kernel");
    return LS_OK;
}

int ls_guide_advance(int32_t* state, int b, const int32_t* table, int table_words, const int64_t* ids, int n, int64_t ids_stride_b,
                     const int64_t* num, int64_t num_stride, void* stream) {
    const char* what = "ls_guide_advance";
    if (!state || !table || !ids) LS_FAIL(LS_ERR_INVALID_ARG, "%s: null pointer", what);
    if (b < 1 || b > 65535 || n < 1 || n > LS_GUIDE_MAX_EXTRA || ids_stride_b < 0 || num_stride < 0)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: b=%d n=%d (1..%d) strides %ld / %ld", what, b, n, LS_GUIDE_MAX_EXTRA, (long)ids_stride_b,
                (long)num_stride);
    if (table_words < LS_GUIDE_HEADER_WORDS || reinterpret_cast<uintptr_t>(table) % 16 != 0)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: the guide table has %d words (at least %d) and is 16-byte aligned", what, table_words,
                LS_GUIDE_HEADER_WORDS);
    GuideAdvanceArgs a;
    a.state = state; a.table = table; a.table_words = table_words; a.ids = ids; a.ids_sb = (long)ids_stride_b;
    a.num = num; a.num_s = (long)num_stride; a.n = n;
    hipLaunchKernelGGL(guide_advance_kernel, dim3(b), dim3(GD_WAVE), 0, static_cast<hipStream_t>(stream), a);
    LS_CHECK_LAUNCH("guide_advance_kernel");
    return LS_OK;
}

}  // extern "C"
