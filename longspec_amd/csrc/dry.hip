// dry.hip -- the DRY repetition penalty on the TARGET's lm_head logits (dry=; gfx950 / CDNA4).  No counterpart in the reference.
//
// The table is one int32 buffer of LS_DRY_TABLE_WORDS words (longspec_amd/dry.py builds it once per decode state):
//   [0] number of breakers (0..64)   [1] allowed_length (1..32)   [2] last_n (0 = the whole text)   [3] LS_DRY_TABLE_WORDS
//   [4 : 37] pen[0 .. 32] as fp32 bits   [37 : 101] breaker ids, padded with -1
// Every count read from it is clamped to the layout before it indexes anything.
//
// A row's text is t = output_ids[z, :w] ++ path(r), m tokens, as in ban.hip (include/longspec_hip.h has the contract).  With
// ctx[k] = t[m-1-k], a position j in [lo, m-2] matches to the depth L(j) = the number of leading k < min(clen, j - lo + 1) with
// t[j-k] == ctx[k], where clen = the number of leading ctx entries inside [lo, m) that are no breakers (<= 32): a breaker inside
// a match is a breaker of the context, so the breaker test is made once per row and never per position.
//
//   dry_rows_kernel   grid (rows / 4 path workgroups + chunks of LS_BAN_CHUNK text columns x tiles of 32 rows, batch), 256 threads,
//                     launched TWICE (pass 0, pass 1) with the same arguments.
//     path workgroup    one row per wave: the positions j in [w-1, m-2], whose candidate v = t[j+1] is a token of the row's
//                       path -- the seam (j = w-1, v = the path's first token) and the matches that end in the path.  Reads the
//                       last 32 committed columns and the path from LDS.
//     chunk workgroup   the positions j in [c0, min(c0 + LS_BAN_CHUNK, w-1)), whose candidate is the committed column j+1 and
//                       so the same for every row: the chunk with 32 columns in front of it and one behind in LDS, the
//                       contexts of its 32 rows in LDS (a wave per row), then every position against every row.  A chunk at or
//                       behind w-1, or wholly in front of every row's lo: the workgroup returns at once.
//     pass 0            atomicMax(scratch[z, r, v], L) for every position with L >= allowed_length and v inside [0, vocab).
//     pass 1            the same positions; the ONE thread whose atomicCAS(scratch[z, r, v], L -> 0) succeeds -- L is then the
//                       cell's maximum -- rewrites logits[z, r, v] = dtype(float(logits[z, r, v]) - pen[L]): one fp32 subtract,
//                       one round to nearest even, one plain 16-bit store.  Every cell pass 0 raised is zero again.
// Lanes of a wave that hit one cell send one atomic (the first lane with the largest L); a relaxed agent-scope load in front of
// each atomic skips those that cannot change the cell (the cells are written by atomics only, pass 0 only raises them and pass 1
// only clears them, so a load never misleads).  Which thread wins a cell is up to the scheduler; what it writes is not.
#include "rule_rows.h"

namespace {

constexpr int DR_THREADS = 256, DR_WAVE = 64, DR_WAVES = DR_THREADS / DR_WAVE;
constexpr int DR_CHUNK = LS_BAN_CHUNK, DR_MAX = LS_DRY_MAX_MATCH, DR_MAX_EXTRA = LS_BAN_MAX_EXTRA, DR_MAX_BRK = 64;
constexpr int DR_PEN = 4, DR_BRK = DR_PEN + DR_MAX + 1, DR_WORDS = DR_BRK + DR_MAX_BRK;
constexpr int DR_ROW_TILE = 32;         // rows a chunk workgroup tests its positions against
static_assert(DR_WORDS == LS_DRY_TABLE_WORDS, "dry table layout");
static_assert(DR_MAX == 32 && DR_MAX <= DR_WAVE && DR_CHUNK % DR_THREADS == 0 && DR_ROW_TILE % DR_WAVES == 0, "dry tiling");

struct DryRowsArgs {
    RuleRows rr;
    const int32_t* table;
    const int64_t* out;      // output_ids [b, width], row stride out_sb; null with width 0
    long out_sb;
    int width;
    RuleColumn col;          // w, clamped to 0..width
    RowExtras ex;            // C <= DR_MAX_EXTRA
    int* scratch;            // [b, rows, vocab] dense, zero on entry and on exit
    int pass;
};

// logits element `h` minus `pen`: fp32 subtract, round to nearest even; a NaN keeps its bits
__device__ __forceinline__ unsigned short penalised(unsigned short h, float pen, bool f16) {
    if (f16) {
        const float x = (float)__builtin_bit_cast(_Float16, h);
        if (x != x) return h;
        return __builtin_bit_cast(unsigned short, (_Float16)(x - pen));
    }
    const float x = __builtin_bit_cast(float, (unsigned)h << 16);
    if (x != x) return h;
    unsigned u = __builtin_bit_cast(unsigned, x - pen);      // finite or an infinity
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

// One position's result for one row, called by whole waves: lanes with `hit` hold a depth L >= allowed_length for the id v inside
// [0, vocab) in row r of batch z (uniform).
__device__ __forceinline__ void commit(const DryRowsArgs& a, bool hit, int v, int L, int z, int r, const float* pen, int lane) {
    const unsigned long long bal = __ballot(hit);
    if (bal == 0) return;
    const int v0 = __shfl(v, __ffsll((long long)bal) - 1, DR_WAVE);
    if (__ballot(hit && v == v0) == bal) {                         // one cell for the wave's hits: its best lane alone goes on
        int mx = hit ? L : 0;
#pragma unroll
        for (int o = DR_WAVE / 2; o >= 1; o >>= 1) {
            const int other = __shfl_xor(mx, o, DR_WAVE);
            mx = other > mx ? other : mx;
        }
        hit = lane == __ffsll((long long)__ballot(hit && L == mx)) - 1;
    }
    if (!hit) return;
    int* cell = a.scratch + ((long)z * a.rr.rows + r) * a.rr.vocab + v;
    const int now = __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.pass == 0) {
        if (now < L) atomicMax(cell, L);
    } else if (now == L && atomicCAS(cell, L, 0) == L) {
        unsigned short* elem = a.rr.logits + (long)z * a.rr.sb + (long)r * a.rr.sr + v;
        *elem = penalised(*elem, pen[L], a.rr.ninf == 0xfc00);
    }
}

__global__ __launch_bounds__(DR_THREADS) void dry_rows_kernel(const DryRowsArgs a) {
    __shared__ int64_t s_path[DR_WAVES][DR_MAX_EXTRA];
    __shared__ int64_t s_ctx[DR_ROW_TILE][DR_MAX];                 // [row][k] = t[m - 1 - k], k < min(32, m)
    __shared__ int64_t s_text[DR_MAX + DR_CHUNK + 1];
    __shared__ float s_pen[DR_MAX + 1];
    __shared__ int s_brk[DR_MAX_BRK];
    __shared__ int s_lo[DR_ROW_TILE], s_clen[DR_ROW_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int z = blockIdx.y;
    const int V = a.rr.vocab, rows = a.rr.rows;
    const int nb = clampi(a.table[0], 0, DR_MAX_BRK), allowed = clampi(a.table[1], 1, DR_MAX), last_n = clampi(a.table[2], 0, 1 << 23);
    const long w64 = rule_column(a.col, z);
    const int w = w64 < 0 ? 0 : w64 > a.width ? a.width : (int)w64;
    const int64_t* out = a.out + (long)z * a.out_sb;               // (never read with w = 0)
    const int path_blocks = (rows + DR_WAVES - 1) / DR_WAVES;
    const unsigned long long lt = (1ull << lane) - 1ull;

    if ((int)blockIdx.x < path_blocks) {
        // ---- one row per wave: the positions j = w - 1 + q, q < d, whose candidate is path[q]
        const int r = blockIdx.x * DR_WAVES + wave;
        int64_t* path = s_path[wave];
        if (tid <= DR_MAX) s_pen[tid] = __builtin_bit_cast(float, a.table[DR_PEN + tid]);
        if (tid >= DR_WAVE && tid < DR_WAVE + DR_MAX_BRK) s_brk[tid - DR_WAVE] = a.table[DR_BRK + tid - DR_WAVE];
        if (tid >= 2 * DR_WAVE && tid < 2 * DR_WAVE + DR_MAX) {
            const int g = w - DR_MAX + tid - 2 * DR_WAVE;
            s_text[tid - 2 * DR_WAVE] = g >= 0 ? out[g] : 0;
        }
        const int d = r < rows ? select_path(a.ex, z, r, lane, path) : 0;         // (r is the wave's: uniform)
        __syncthreads();                                           // (every wave of the workgroup gets here)
        if (r >= rows || d == 0) return;
        auto text = [&](int i) -> int64_t { return i < w ? s_text[i - (w - DR_MAX)] : path[i - w]; };      // t[i], m - 32 <= i < m
        const int m = w + d;
        const int lo = last_n > 0 && m > last_n ? m - last_n : 0;
        const int navail = m - lo < DR_MAX ? m - lo : DR_MAX;
        bool stop = lane >= navail;                                // the first lane that is outside [lo, m) or holds a breaker
        if (!stop) {
            const int64_t cv = text(m - 1 - lane);
#pragma clang loop unroll(disable) vectorize(disable)
            for (int q = 0; q < nb; ++q) stop |= cv == (int64_t)s_brk[q];
        }
        const int clen = __ffsll((long long)__ballot(stop)) - 1;   // (lanes 32.. always stop)
        if (clen == 0) return;
        for (int q0 = 0; q0 < d; q0 += DR_WAVE) {
            const int q = q0 + lane, j = w - 1 + q;                // j <= m - 2
            int L = 0, v = 0;
            bool hit = false;
            if (q < d && j >= lo) {
                const int kmax = clen < j - lo + 1 ? clen : j - lo + 1;
                while (L < kmax && text(j - L) == text(m - 1 - L)) ++L;
                const int64_t id = path[q];
                hit = L >= allowed && id >= 0 && id < (int64_t)V;
                v = (int)id;
            }
            commit(a, hit, v, L, z, r, s_pen, lane);
        }
        return;
    }

    // ---- a chunk of the committed text against a tile of rows: positions j in [c0, min(c0 + DR_CHUNK, w - 1))
    const int tiles = (rows + DR_ROW_TILE - 1) / DR_ROW_TILE;
    const int idx = blockIdx.x - path_blocks;
    const int c0 = (idx / tiles) * DR_CHUNK, t0 = (idx % tiles) * DR_ROW_TILE;
    const int lo_min = last_n > 0 && w > last_n ? w - last_n : 0;  // the lo of a row without a path; no row's is smaller
    if (c0 >= w - 1 || c0 + DR_CHUNK <= lo_min) return;            // (uniform)
    const int tile_rows = rows - t0 < DR_ROW_TILE ? rows - t0 : DR_ROW_TILE;
    for (int i = tid; i < DR_MAX + DR_CHUNK + 1; i += DR_THREADS) {
        const int g = c0 - DR_MAX + i;
        s_text[i] = g >= 0 && g < w ? out[g] : 0;
    }
    if (tid <= DR_MAX) s_pen[tid] = __builtin_bit_cast(float, a.table[DR_PEN + tid]);
    if (tid >= DR_WAVE && tid < DR_WAVE + DR_MAX_BRK) s_brk[tid - DR_WAVE] = a.table[DR_BRK + tid - DR_WAVE];
    // the contexts: the end of each row's path and, in front of it, the end of the committed text (lane i: column w - 1 - i)
    const int64_t tail = lane < DR_MAX && w - 1 - lane >= 0 ? out[w - 1 - lane] : 0;
    for (int rt = wave; rt < tile_rows; rt += DR_WAVES) {
        const RowExtras& e = a.ex;
        int64_t* ctx = s_ctx[rt];
        int d = 0;
        if (e.C > 0) {
            const int64_t* ids = e.ids + (long)z * e.ids_sb;
            const int64_t* mask = e.mask + (long)z * e.mask_sb + (long)(t0 + rt) * e.mask_sr;
            for (int q0 = 0; q0 < e.C; q0 += DR_WAVE) d += __popcll(__ballot(q0 + lane < e.C && mask[q0 + lane] != 0));
            int cnt = 0;
            for (int q0 = 0; q0 < e.C; q0 += DR_WAVE) {
                const int c = q0 + lane;
                const int64_t mk = c < e.C ? mask[c] : 0, id = c < e.C ? ids[c] : 0;
                const unsigned long long bal = __ballot(mk != 0);
                const int from_end = d - 1 - (cnt + __popcll(bal & lt));         // the path's q-th token is t[m - 1 - (d - 1 - q)]
                if (mk != 0 && from_end < DR_MAX) ctx[from_end] = id;
                cnt += __popcll(bal);
            }
        }
        const int64_t tv = __shfl(tail, lane >= d ? lane - d : 0, DR_WAVE);
        if (lane >= d && lane < DR_MAX) ctx[lane] = tv;            // (columns in front of 0 hold 0 and lie outside [lo, m))
        if (lane == 0) {
            const int m = w + d, lo = last_n > 0 && m > last_n ? m - last_n : 0;
            s_lo[rt] = lo;
            s_clen[rt] = m - lo < DR_MAX ? m - lo : DR_MAX;        // (for now: the context entries inside [lo, m))
        }
    }
    __syncthreads();
    for (int rt = wave; rt < tile_rows; rt += DR_WAVES) {
        bool stop = lane >= s_clen[rt];                            // the first lane that is outside [lo, m) or holds a breaker
        if (!stop) {
            const int64_t cv = s_ctx[rt][lane];
#pragma clang loop unroll(disable) vectorize(disable)
            for (int q = 0; q < nb; ++q) stop |= cv == (int64_t)s_brk[q];
        }
        const int clen = __ffsll((long long)__ballot(stop)) - 1;
        if (lane == 0) s_clen[rt] = clen;
    }
    __syncthreads();
#pragma unroll 1
    for (int p = 0; p < DR_CHUNK / DR_THREADS; ++p) {
        const int jl = p * DR_THREADS + tid, j = c0 + jl;
        const int64_t xj = s_text[DR_MAX + jl], id = s_text[DR_MAX + jl + 1];
        const bool live = j <= w - 2 && id >= 0 && id < (int64_t)V;
        for (int rt = 0; rt < tile_rows; ++rt) {
            int L = 0;
            if (live && xj == s_ctx[rt][0]) {
                const int lo = s_lo[rt], clen = s_clen[rt];
                const int kmax = clen < j - lo + 1 ? clen : j - lo + 1;           // (j < lo: none)
                while (L < kmax && s_text[DR_MAX + jl - L] == s_ctx[rt][L]) ++L;
            }
            commit(a, L >= allowed, (int)id, L, z, t0 + rt, s_pen, lane);
        }
    }
}

}  // namespace

extern "C" {

int ls_dry_rows(void* logits, int b, int rows, int vocab, int dtype, int64_t stride_b, int64_t stride_r, const int32_t* table,
                int table_words, const int64_t* output_ids, int64_t out_stride_b, int width, int32_t* scratch, int64_t scratch_words,
                const int32_t* base, const int32_t* base_sub, int base_add, const int64_t* extra_ids, int64_t ids_stride_b,
                const int64_t* extra_mask, int64_t mask_stride_b, int64_t mask_stride_r, int n_extra, void* stream) {
    const char* what = "ls_dry_rows";
    DryRowsArgs a;
    if (int rc = rule_rows_check(what, logits, table != nullptr && scratch != nullptr, b, rows, vocab, dtype, stride_b, stride_r, a.rr))
        return rc;
    if (table_words != LS_DRY_TABLE_WORDS) LS_FAIL(LS_ERR_INVALID_ARG, "%s: the dry table has %d words, not %d", what, table_words, LS_DRY_TABLE_WORDS);
    if (scratch_words < (int64_t)b * rows * vocab || reinterpret_cast<uintptr_t>(scratch) % 4 != 0)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: scratch of %ld words, b * rows * vocab = %ld needed", what, (long)scratch_words, (long)b * rows * vocab);
    if (width < 0 || width > (1 << 23) || (width > 0 && (!output_ids || out_stride_b < width)))
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: width=%d (0..2^23) needs output_ids with a row stride %ld >= width", what, width, (long)out_stride_b);
    if (int rc = row_extras_check(what, extra_ids, ids_stride_b, extra_mask, mask_stride_b, mask_stride_r, n_extra, LS_BAN_MAX_EXTRA, a.ex))
        return rc;
    a.table = table; a.out = width > 0 ? output_ids : nullptr; a.out_sb = width > 0 ? (long)out_stride_b : 0l; a.width = width;
    a.col = RuleColumn{base, base_sub, base_add};
    a.scratch = scratch;
    const long chunks = (width + DR_CHUNK - 1) / DR_CHUNK, tiles = (rows + DR_ROW_TILE - 1) / DR_ROW_TILE;
    const long blocks = (rows + DR_WAVES - 1) / DR_WAVES + chunks * tiles;
    if (blocks > 0x7fffffffl) LS_FAIL(LS_ERR_INVALID_ARG, "%s: rows=%d x width=%d needs %ld workgroups", what, rows, width, blocks);
    const dim3 grid((unsigned)blocks, b), block(DR_THREADS);
    for (a.pass = 0; a.pass < 2; ++a.pass) {
        hipLaunchKernelGGL(dry_rows_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
        LS_CHECK_LAUNCH("dry_rows_kernel");
    }
    return LS_OK;
}

}  // extern "C"
