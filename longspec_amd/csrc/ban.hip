// ban.hip -- banned sequences and no-repeat n-grams on the TARGET's lm_head logits (ban=; gfx950 / CDNA4).  No counterpart in
// the reference.
//
// The ban table is one int32 buffer of LS_BAN_TABLE_WORDS words (longspec_amd/ban.py builds it once per decode state):
//   [0] n_seqs (0..64)   [1] n = no_repeat_ngram (0..16)   [2] reserved   [3] LS_BAN_TABLE_WORDS
//   [4 : 69] sequence offsets into the token area   [69 : 1093] sequence tokens, back to back
// Every count and offset read from it is clamped to the layout before it indexes anything.
//
// A row's text is t = output_ids[z, :w] ++ path(r): the committed columns, then the row's selected extras in increasing column
// (include/longspec_hip.h has the contract).  All rows of a batch row share output_ids[z, :w] and differ in their path only:
//
//   ban_rows_kernel   grid (rows / 4 path workgroups + chunks of LS_BAN_CHUNK text columns x tiles of 32 rows, batch), 256 threads.
//     path workgroup    one row per wave: the wave assembles the row's ordered path in LDS (ballot + prefix over 64 mask columns
//                       at a time; the running count keeps the order), then a lane per listed sequence compares it with the
//                       end of t and a lane per PATH position j >= w compares t[j-n+1 .. j-1] with t[m-n+1 .. m-1] -- the
//                       matches wholly in the path and those that straddle text and path.
//     chunk workgroup   reads its text columns and the 16 in front of them once into LDS, puts the last n - 1 tokens of each
//                       of its 32 rows' t into LDS (a wave per row, no barrier between rows: the prefix count gives every
//                       selected column its distance from the end) and tests each of its positions j < w against every
//                       row -- the matches wholly in the text, those across a chunk edge included.  A chunk at or behind w,
//                       or n = 0: the workgroup returns at once.
// A forbidden id inside [0, vocab) is one plain 16-bit store of the -inf pattern; lanes that hit one address store one value.
// No scratch, no atomics, no floating-point arithmetic; ids are compared as 64-bit integers.
#include "rule_rows.h"

namespace {

constexpr int BN_THREADS = 256, BN_WAVE = 64, BN_WAVES = BN_THREADS / BN_WAVE;
constexpr int BN_CHUNK = LS_BAN_CHUNK, BN_HALO = 16, BN_MAX_EXTRA = LS_BAN_MAX_EXTRA;
constexpr int BN_MAX_SEQS = 64, BN_MAX_SEQ_LEN = 16, BN_MAX_N = 16;
constexpr int BN_OFFS = 4, BN_TOKS = BN_OFFS + BN_MAX_SEQS + 1, BN_WORDS = BN_TOKS + BN_MAX_SEQS * BN_MAX_SEQ_LEN;
constexpr int BN_ROW_TILE = 32;         // rows a chunk workgroup tests its positions against
static_assert(BN_WORDS == LS_BAN_TABLE_WORDS, "ban table layout");
static_assert(BN_HALO >= BN_MAX_N - 1 && BN_CHUNK % BN_THREADS == 0 && BN_ROW_TILE % BN_WAVES == 0, "ban tiling");

struct BanRowsArgs {
    RuleRows rr;
    const int32_t* table;
    const int64_t* out;      // output_ids [b, width], row stride out_sb; null with width 0
    long out_sb;
    int width;
    RuleColumn col;          // w, clamped to 0..width
    RowExtras ex;            // C <= BN_MAX_EXTRA
};

// ctx[i] = t[m - 1 - i] for i < keep (= n - 1 <= 15) of row r < rows, whose text has m = w + d >= keep + 1 tokens: the end of the
// row's path, and in front of it the end of the committed text.  No barrier and no LDS read: a wave builds one row after the
// other.  Called by whole waves.
__device__ __forceinline__ void build_context(const RowExtras& a, int z, int r, int lane, int keep, int64_t tail, int64_t* ctx) {
    const unsigned long long lt = (1ull << lane) - 1ull;
    int d = 0;
    if (a.C > 0) {
        const int64_t* ids = a.ids + (long)z * a.ids_sb;
        const int64_t* mask = a.mask + (long)z * a.mask_sb + (long)r * a.mask_sr;
        // the first 64 columns stay in registers: one round trip for the trees and chains the loops pass (C <= 79)
        const int64_t mk0 = lane < a.C ? mask[lane] : 0, id0 = lane < a.C ? ids[lane] : 0;
        const unsigned long long bal0 = __ballot(mk0 != 0);
        d = __popcll(bal0);
        for (int c0 = BN_WAVE; c0 < a.C; c0 += BN_WAVE) d += __popcll(__ballot(c0 + lane < a.C && mask[c0 + lane] != 0));
        int from_end = d - 1 - __popcll(bal0 & lt);              // the path's q-th token is t[w + q] = t[m - 1 - (d - 1 - q)]
        if (mk0 != 0 && from_end < keep) ctx[from_end] = id0;
        int cnt = __popcll(bal0);
        for (int c0 = BN_WAVE; c0 < a.C; c0 += BN_WAVE) {
            const int c = c0 + lane;
            const int64_t mk = c < a.C ? mask[c] : 0, id = c < a.C ? ids[c] : 0;
            const unsigned long long bal = __ballot(mk != 0);
            from_end = d - 1 - (cnt + __popcll(bal & lt));
            if (mk != 0 && from_end < keep) ctx[from_end] = id;
            cnt += __popcll(bal);
        }
    }
    // `tail`: lane i holds output_ids[z, w - 1 - i] (i < 15): in front of the path, the end of the committed text
    const int64_t v = __shfl(tail, lane >= d ? lane - d : 0, BN_WAVE);
    if (lane >= d && lane < keep) ctx[lane] = v;                              // w + d >= keep + 1: column w - 1 - (lane - d) >= 1
}

__global__ __launch_bounds__(BN_THREADS) void ban_rows_kernel(const BanRowsArgs a) {
    __shared__ int64_t s_path[BN_WAVES][BN_MAX_EXTRA];
    __shared__ int64_t s_ctx[BN_ROW_TILE][BN_MAX_N];               // [row][i] = t[m - 1 - i], i < n - 1
    __shared__ int64_t s_text[BN_HALO + BN_CHUNK];
    __shared__ int32_t s_table[BN_WORDS];                          // (path workgroups)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int z = blockIdx.y;
    const int V = a.rr.vocab, rows = a.rr.rows;
    const unsigned short ninf = a.rr.ninf;
    const int n = clampi(a.table[1], 0, BN_MAX_N);
    const long w64 = rule_column(a.col, z);
    const int w = w64 < 0 ? 0 : w64 > a.width ? a.width : (int)w64;
    const int64_t* out = a.out + (long)z * a.out_sb;              // (never read with w = 0)
    unsigned short* logits = a.rr.logits + (long)z * a.rr.sb;
    const int path_blocks = (rows + BN_WAVES - 1) / BN_WAVES;

    if ((int)blockIdx.x < path_blocks) {
        // ---- one row per wave: the listed sequences against the end of t, and the positions j >= w of the row's path
        // Everything the tests read goes to LDS first, in one round of loads: the table, the last 16 committed columns (no test
        // reaches further back than 15 tokens from the end of t) and the path.
        const int r = blockIdx.x * BN_WAVES + wave;
        int64_t* path = s_path[wave];
        for (int i = tid; i < BN_WORDS; i += BN_THREADS) s_table[i] = a.table[i];
        if (tid < BN_HALO) s_text[tid] = w - BN_HALO + tid >= 0 ? out[w - BN_HALO + tid] : 0;
        const int d = r < rows ? select_path(a.ex, z, r, lane, path) : 0;         // (r is the wave's: uniform)
        __syncthreads();                                           // (every wave of the workgroup gets here)
        if (r >= rows) return;
        auto text = [&](int i) -> int64_t { return i < w ? s_text[i - (w - BN_HALO)] : path[i - w]; };      // t[i], m - 16 <= i < m
        const int m = w + d;
        unsigned short* row = logits + (long)r * a.rr.sr;
        const int n_seqs = clampi(s_table[0], 0, BN_MAX_SEQS);
        for (int q = lane; q < n_seqs; q += BN_WAVE) {
            const int off = clampi(s_table[BN_OFFS + q], 0, BN_MAX_SEQS * BN_MAX_SEQ_LEN);
            const int end = clampi(s_table[BN_OFFS + q + 1], off, BN_MAX_SEQS * BN_MAX_SEQ_LEN);
            const int len = end - off > BN_MAX_SEQ_LEN ? BN_MAX_SEQ_LEN : end - off;
            if (len < 1 || len - 1 > m) continue;
            bool hit = true;
            for (int i = 0; hit && i < len - 1; ++i) hit = text(m - len + 1 + i) == (int64_t)s_table[BN_TOKS + off + i];
            const int id = s_table[BN_TOKS + off + len - 1];
            if (hit && id >= 0 && id < V) row[id] = ninf;
        }
        if (n >= 1) {
            for (int q = lane; q < d; q += BN_WAVE) {             // position j = w + q of the path; j <= m - 1
                const int j = w + q;
                if (j < n - 1) continue;
                bool hit = true;
                for (int k = 1; hit && k < n; ++k) hit = text(j - k) == text(m - k);
                const int64_t id = path[q];
                if (hit && id >= 0 && id < (int64_t)V) row[id] = ninf;
            }
        }
        return;
    }

    // ---- a chunk of the committed text against a tile of rows: positions j in [max(c0, n - 1), min(w, c0 + BN_CHUNK))
    const int tiles = (rows + BN_ROW_TILE - 1) / BN_ROW_TILE;
    const int idx = blockIdx.x - path_blocks;
    const int c0 = (idx / tiles) * BN_CHUNK, t0 = (idx % tiles) * BN_ROW_TILE;
    if (n == 0 || c0 >= w || w < n) return;                       // (uniform; w < n: no position; from here on every m >= n)
    const int tile_rows = rows - t0 < BN_ROW_TILE ? rows - t0 : BN_ROW_TILE;
    for (int i = tid; i < BN_HALO + BN_CHUNK; i += BN_THREADS) {
        const int g = c0 - BN_HALO + i;
        s_text[i] = g >= 0 && g < w ? out[g] : 0;
    }
    const int64_t tail = lane < BN_MAX_N - 1 && w - 1 - lane >= 0 ? out[w - 1 - lane] : 0;
    for (int rt = wave; rt < tile_rows; rt += BN_WAVES) build_context(a.ex, z, t0 + rt, lane, n - 1, tail, s_ctx[rt]);
    __syncthreads();
#pragma unroll
    for (int p = 0; p < BN_CHUNK / BN_THREADS; ++p) {
        const int jl = p * BN_THREADS + tid, j = c0 + jl;
        if (j < n - 1 || j >= w) continue;
        const int64_t id = s_text[BN_HALO + jl];
        if (id < 0 || id >= (int64_t)V) continue;
        for (int rt = 0; rt < tile_rows; ++rt) {
            bool hit = true;
            for (int k = 1; hit && k < n; ++k) hit = s_text[BN_HALO + jl - k] == s_ctx[rt][k - 1];
            if (hit) logits[(long)(t0 + rt) * a.rr.sr + id] = ninf;
        }
    }
}

}  // namespace

extern "C" {

int ls_ban_rows(void* logits, int b, int rows, int vocab, int dtype, int64_t stride_b, int64_t stride_r, const int32_t* table,
                int table_words, const int64_t* output_ids, int64_t out_stride_b, int width, const int32_t* base,
                const int32_t* base_sub, int base_add, const int64_t* extra_ids, int64_t ids_stride_b, const int64_t* extra_mask,
                int64_t mask_stride_b, int64_t mask_stride_r, int n_extra, void* stream) {
    const char* what = "ls_ban_rows";
    BanRowsArgs a;
    if (int rc = rule_rows_check(what, logits, table != nullptr, b, rows, vocab, dtype, stride_b, stride_r, a.rr)) return rc;
    if (table_words != LS_BAN_TABLE_WORDS) LS_FAIL(LS_ERR_INVALID_ARG, "%s: the ban table has %d words, not %d", what, table_words, LS_BAN_TABLE_WORDS);
    if (width < 0 || width > (1 << 23) || (width > 0 && (!output_ids || out_stride_b < width)))
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: width=%d (0..2^23) needs output_ids with a row stride %ld >= width", what, width, (long)out_stride_b);
    if (int rc = row_extras_check(what, extra_ids, ids_stride_b, extra_mask, mask_stride_b, mask_stride_r, n_extra, LS_BAN_MAX_EXTRA, a.ex))
        return rc;
    a.table = table; a.out = width > 0 ? output_ids : nullptr; a.out_sb = width > 0 ? (long)out_stride_b : 0l; a.width = width;
    a.col = RuleColumn{base, base_sub, base_add};
    const long chunks = (width + BN_CHUNK - 1) / BN_CHUNK, tiles = (rows + BN_ROW_TILE - 1) / BN_ROW_TILE;
    const long blocks = (rows + BN_WAVES - 1) / BN_WAVES + chunks * tiles;
    if (blocks > 0x7fffffffl) LS_FAIL(LS_ERR_INVALID_ARG, "%s: rows=%d x width=%d needs %ld workgroups", what, rows, width, blocks);
    const dim3 grid((unsigned)blocks, b), block(BN_THREADS);
    hipLaunchKernelGGL(ban_rows_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
    LS_CHECK_LAUNCH("ban_rows_kernel");
    return LS_OK;
}

}  // extern "C"
