// stop.hip -- stop conditions of the decode loops (stop=; gfx950 / CDNA4): stop token ids, stop sequences, min_tokens.
//
// The stop table is one int32 buffer of LS_STOP_TABLE_WORDS words (longspec_amd/stop.py builds it once per decode state):
//   [0] n_ids (0..64)   [1] n_seqs (0..16)   [2] min_tokens   [3] LS_STOP_TABLE_WORDS
//   [4 : 68] ids, -1 padded   [68 : 85] sequence offsets into the token area   [85 : 341] sequence tokens, back to back
// Every count and offset read from it is clamped to the layout before it indexes anything.
//
// ls_stop_scan      one wave per batch row, behind the round's commit and in front of its one host read.  Over the columns the
//                   round wrote, lanes take (column, stop) pairs; a pair that matches at a column >= min_tokens offers the key
//                   column * 128 + stop, and the wave's minimum is the earliest column and, there, the first stop in listing
//                   order.  A hit is recorded in stop_state [b, 4] (length, which, match_start, reserved), the columns at or
//                   behind `length` go back to their fill, and bit 1 of the round's state[z, 1] is raised.  A row that has
//                   stopped already matches nothing new: it erases [length, written) again and raises the bit again.
// ls_stop_ban_rows  one wave per row of 16-bit target logits: where the row predicts a column < min_tokens, the stop ids' entries
//                   become -inf (16-bit vector stores of the pattern); every other row and element keeps its bits.
// No scratch, no LDS, no floating-point arithmetic, no atomics: distinct ids are distinct addresses.
#include "rule_rows.h"

namespace {

constexpr int ST_WAVE = 64;
constexpr int ST_MAX_IDS = 64, ST_MAX_SEQS = 16, ST_MAX_SEQ_LEN = 16;
constexpr int ST_IDS = 4, ST_OFFS = ST_IDS + ST_MAX_IDS, ST_TOKS = ST_OFFS + ST_MAX_SEQS + 1;
constexpr int ST_WORDS = ST_TOKS + ST_MAX_SEQS * ST_MAX_SEQ_LEN;
static_assert(ST_WORDS == LS_STOP_TABLE_WORDS, "stop table layout");
constexpr int ST_NO_HIT = 0x7fffffff;

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int o = __shfl_xor(v, off, ST_WAVE);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, ST_WAVE);
    return v;
}

// length of sequence q and its first token's index in the table, both inside the layout whatever the table holds
__device__ __forceinline__ void seq_span(const int32_t* __restrict__ table, int q, int& off, int& len) {
    off = clampi(table[ST_OFFS + q], 0, ST_MAX_SEQS * ST_MAX_SEQ_LEN);
    const int end = clampi(table[ST_OFFS + q + 1], off, ST_MAX_SEQS * ST_MAX_SEQ_LEN);
    len = end - off > ST_MAX_SEQ_LEN ? ST_MAX_SEQ_LEN : end - off;
}

struct ScanArgs {
    int64_t* out;            // output_ids [b, width], row stride out_sb
    long out_sb;
    int width;
    RuleColumn written;      // columns written so far (written.base is never null)
    const int64_t* num;      // columns this round wrote = num[z * num_stride], or num_const without the pointer
    long num_stride;
    int num_const;
    const int32_t* table;
    int32_t* stop_state;     // [b, 4]
    int64_t fill;
    int64_t* round_state;    // [b, state_sb...]: word 1 |= 2 on a stop; may be null
    long state_sb;
    int64_t* spec_mask;      // [b, width] row stride mask_sb, erased with 0; may be null
    long mask_sb;
    float* lp_token;         // [b, width] dense; may be null
    float* lp_top;           // [b, width, lp_n] dense
    int64_t* lp_top_ids;
    int lp_n;
};

__global__ __launch_bounds__(ST_WAVE) void stop_scan_kernel(ScanArgs a) {
    const int z = blockIdx.x, lane = threadIdx.x;
    int64_t* out = a.out + (long)z * a.out_sb;
    __builtin_assume(a.written.base != nullptr);                   // (ls_stop_scan refuses a null `written`)
    const long w64 = rule_column(a.written, z);
    const int w = w64 < 0 ? 0 : w64 > a.width ? a.width : (int)w64;
    int32_t* ss = a.stop_state + (long)z * 4;
    int length = ss[0];
    if (length < 0) {
        const int64_t n64 = a.num ? a.num[(long)z * a.num_stride] : (int64_t)a.num_const;
        const int n_new = n64 < 0 ? 0 : n64 > w ? w : (int)n64;
        const int c0 = w - n_new;
        const int n_ids = clampi(a.table[0], 0, ST_MAX_IDS), n_seqs = clampi(a.table[1], 0, ST_MAX_SEQS);
        const int min_tokens = a.table[2] < 0 ? 0 : a.table[2];
        const int n_stops = n_ids + n_seqs;                       // <= 80 < 128
        int best = ST_NO_HIT;
        for (int p = lane; p < n_new * n_stops; p += ST_WAVE) {
            const int j = p / n_stops, s = p - j * n_stops;
            const int c = c0 + j;                                  // 0 <= c < w <= width
            if (c < min_tokens) continue;
            bool hit;
            if (s < n_ids) {
                hit = out[c] == (int64_t)a.table[ST_IDS + s];
            } else {
                int off, len;
                seq_span(a.table, s - n_ids, off, len);
                hit = len >= 1 && len <= c + 1;                    // never in front of column 0; its last column is c < w
                for (int i = 0; hit && i < len; ++i) hit = out[c - len + 1 + i] == (int64_t)a.table[ST_TOKS + off + i];
            }
            if (hit) {
                const int key = c * 128 + s;
                best = key < best ? key : best;
            }
        }
        best = wave_min(best);
        if (best == ST_NO_HIT) return;
        const int c = best >> 7, s = best & 127;
        int len = 1;
        if (s >= n_ids) {
            int off;
            seq_span(a.table, s - n_ids, off, len);
        }
        length = c + 1;
        if (lane == 0) {
            ss[0] = length;
            ss[1] = s;
            ss[2] = c - len + 1;
        }
    }
    if (lane == 0 && a.round_state) a.round_state[(long)z * a.state_sb + 1] |= 2;
    // columns [length, w) back to their fill
    const int per = 1 + a.lp_n;
    const int cols = w > length ? w - length : 0;
    for (int i = lane; i < cols * per; i += ST_WAVE) {
        const int j = i / per, e = i - j * per;
        const int col = length + j;
        const long d = (long)z * a.width + col;
        if (e == 0) {
            out[col] = a.fill;
            if (a.spec_mask) a.spec_mask[(long)z * a.mask_sb + col] = 0;
            if (a.lp_token) a.lp_token[d] = __uint_as_float(0x7fc00000u);
        } else if (a.lp_top) {
            a.lp_top[d * a.lp_n + e - 1] = __uint_as_float(0xff800000u);
            a.lp_top_ids[d * a.lp_n + e - 1] = -1;
        }
    }
}

struct BanArgs {
    RuleRows rr;
    const int32_t* table;
    RuleColumn col;          // row r predicts this column + depth(r)
    int depth_mode;          // 0: depth 0; 1: depth r; 2: the row sum of mask[z, r, 1:mask_cols]
    const int64_t* mask;
    long mask_sb, mask_sr;
    int mask_cols;
};

__global__ __launch_bounds__(ST_WAVE) void stop_ban_rows_kernel(BanArgs a) {
    const int r = blockIdx.x, z = blockIdx.y, lane = threadIdx.x;
    const int min_tokens = a.table[2];
    if (min_tokens <= 0) return;
    long col = rule_column(a.col, z);
    if (col >= min_tokens) return;                                 // the usual case once the minimum is passed: no mask read
    if (a.depth_mode == 1) {
        col += r;
    } else if (a.depth_mode == 2) {
        const int64_t* row = a.mask + (long)z * a.mask_sb + (long)r * a.mask_sr;
        int d = 0;
        for (int c = 1 + lane; c < a.mask_cols; c += ST_WAVE) d += row[c] != 0 ? 1 : 0;
        col += wave_sum(d);
    }
    if (col >= min_tokens) return;
    const int n_ids = clampi(a.table[0], 0, ST_MAX_IDS);
    if (lane < n_ids) {
        const int id = a.table[ST_IDS + lane];
        if (id >= 0 && id < a.rr.vocab) a.rr.logits[(long)z * a.rr.sb + (long)r * a.rr.sr + id] = a.rr.ninf;
    }
}

}  // namespace

extern "C" {

int ls_stop_scan(int64_t* output_ids, int b, int64_t out_stride_b, int width, const int32_t* written, const int32_t* written_sub,
                 int written_add, const int64_t* num, int64_t num_stride, int num_const, const int32_t* table, int table_words,
                 int32_t* stop_state, int64_t fill, int64_t* round_state, int64_t state_stride_b, int64_t* spec_mask,
                 int64_t mask_stride_b, float* lp_token, float* lp_top, int64_t* lp_top_ids, int lp_n, void* stream) {
    const char* what = "ls_stop_scan";
    if (!output_ids || !written || !table || !stop_state) LS_FAIL(LS_ERR_INVALID_ARG, "%s: null pointer", what);
    if (b < 1 || b > 65535 || width < 1 || width > (1 << 23) || out_stride_b < width || num_stride < 0 || num_const < 0)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: b=%d width=%d row stride %ld num stride %ld num_const=%d", what, b, width, (long)out_stride_b,
                (long)num_stride, num_const);
    if (table_words != LS_STOP_TABLE_WORDS) LS_FAIL(LS_ERR_INVALID_ARG, "%s: the stop table has %d words, not %d", what, table_words, LS_STOP_TABLE_WORDS);
    if (round_state && state_stride_b < 2) LS_FAIL(LS_ERR_INVALID_ARG, "%s: the round's state needs two words a row", what);
    if (spec_mask && mask_stride_b < width) LS_FAIL(LS_ERR_INVALID_ARG, "%s: spec_mask row stride %ld < width %d", what, (long)mask_stride_b, width);
    if (lp_n < 0 || lp_n > 20 || (lp_n > 0 && (!lp_token || !lp_top || !lp_top_ids)) || (!lp_token && (lp_top || lp_top_ids)))
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: lp_n=%d (0..20) and the log-prob buffers do not go together", what, lp_n);
    ScanArgs a;
    a.out = output_ids; a.out_sb = (long)out_stride_b; a.width = width;
    a.written = RuleColumn{written, written_sub, written_add};
    a.num = num; a.num_stride = (long)num_stride; a.num_const = num_const;
    a.table = table; a.stop_state = stop_state; a.fill = fill;
    a.round_state = round_state; a.state_sb = (long)state_stride_b;
    a.spec_mask = spec_mask; a.mask_sb = (long)mask_stride_b;
    a.lp_token = lp_token; a.lp_top = lp_n > 0 ? lp_top : nullptr; a.lp_top_ids = lp_n > 0 ? lp_top_ids : nullptr;
    a.lp_n = lp_token ? lp_n : 0;
    hipLaunchKernelGGL(stop_scan_kernel, dim3(b), dim3(ST_WAVE), 0, static_cast<hipStream_t>(stream), a);
    LS_CHECK_LAUNCH("stop_scan_kernel");
    return LS_OK;
}

int ls_stop_ban_rows(void* logits, int b, int rows, int vocab, int dtype, int64_t stride_b, int64_t stride_r, const int32_t* table,
                     int table_words, const int32_t* base, const int32_t* base_sub, int base_add, int depth_mode,
                     const int64_t* mask, int64_t mask_stride_b, int64_t mask_stride_r, int mask_cols, void* stream) {
    const char* what = "ls_stop_ban_rows";
    BanArgs a;
    if (int rc = rule_rows_check(what, logits, table != nullptr, b, rows, vocab, dtype, stride_b, stride_r, a.rr)) return rc;
    if (table_words != LS_STOP_TABLE_WORDS) LS_FAIL(LS_ERR_INVALID_ARG, "%s: the stop table has %d words, not %d", what, table_words, LS_STOP_TABLE_WORDS);
    if (depth_mode < 0 || depth_mode > 2) LS_FAIL(LS_ERR_INVALID_ARG, "%s: depth_mode=%d", what, depth_mode);
    if (depth_mode == 2 && (!mask || mask_cols < 1 || mask_stride_r < mask_cols || mask_stride_b < 0))
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: depth from a mask needs the mask, mask_cols=%d >= 1 and a row stride %ld >= mask_cols", what,
                mask_cols, (long)mask_stride_r);
    a.table = table; a.col = RuleColumn{base, base_sub, base_add};
    a.depth_mode = depth_mode; a.mask = mask; a.mask_sb = (long)mask_stride_b; a.mask_sr = (long)mask_stride_r; a.mask_cols = mask_cols;
    hipLaunchKernelGGL(stop_ban_rows_kernel, dim3(rows, b), dim3(ST_WAVE), 0, static_cast<hipStream_t>(stream), a);
    LS_CHECK_LAUNCH("stop_ban_rows_kernel");
    return LS_OK;
}

}  // extern "C"
