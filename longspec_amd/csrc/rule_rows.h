// rule_rows.h -- what the operators on the TARGET's lm_head logits share (ban.hip, guide.hip, stop.hip, penalty.hip): the rows an
// operator rewrites in place, a row's selected extras, and the committed column a batch row stands at.  The argument structs of
// those kernels embed the three PODs below; include/longspec_hip.h has the contract, longspec_amd/ops.py the Python side of it.
#pragma once
#include "ls_common.h"

struct RuleRows {
    unsigned short* logits;  // [b, rows, vocab] 16-bit, strides in elements
    long sb, sr;
    int rows, vocab;
    unsigned short ninf;     // the type's -inf pattern
};

// Row r of batch z selects every ids[z, c] with mask[z, r, c] != 0; mask_sb = 0: one [rows, C] mask for the whole batch.
struct RowExtras {
    const int64_t* ids;      // [b, C], row stride ids_sb
    const int64_t* mask;     // [b, rows, C], strides mask_sb / mask_sr
    long ids_sb, mask_sb, mask_sr;
    int C;
};

struct RuleColumn {          // (base ? base[z] : 0) - (base_sub ? base_sub[z] : 0) + base_add
    const int32_t* base;
    const int32_t* base_sub;
    int base_add;
};

// ---- host: each returns an LS_ERR_* code with the message set, or LS_OK with `o` filled
// `others`: the operator's other required pointers are all there (one "null pointer" refusal for them and the logits).
static inline int rule_rows_check(const char* what, void* logits, bool others, int b, int rows, int vocab, int dtype, int64_t stride_b,
                                  int64_t stride_r, RuleRows& o) {
    if (!logits || !others) LS_FAIL(LS_ERR_INVALID_ARG, "%s: null pointer", what);
    if (dtype != LS_F16 && dtype != LS_BF16) LS_FAIL(LS_ERR_INVALID_ARG, "%s: dtype", what);
    if (b < 1 || b > 65535 || rows < 1 || rows > 65535 || vocab < 1 || stride_r < vocab || stride_b < 0)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: b=%d rows=%d vocab=%d strides %ld / %ld (row stride >= vocab)", what, b, rows, vocab,
                (long)stride_b, (long)stride_r);
    if (reinterpret_cast<uintptr_t>(logits) % 2 != 0) LS_FAIL(LS_ERR_INVALID_ARG, "%s: misaligned logits", what);
    o = RuleRows{static_cast<unsigned short*>(logits), (long)stride_b, (long)stride_r, rows, vocab,
                 (unsigned short)(dtype == LS_F16 ? 0xfc00 : 0xff80)};
    return LS_OK;
}

static inline int row_extras_check(const char* what, const int64_t* ids, int64_t ids_stride_b, const int64_t* mask, int64_t mask_stride_b,
                                   int64_t mask_stride_r, int n_extra, int limit, RowExtras& o) {
    if (n_extra < 0 || n_extra > limit) LS_FAIL(LS_ERR_INVALID_ARG, "%s: n_extra=%d outside 0..%d", what, n_extra, limit);
    if (n_extra > 0 && (!ids || !mask || ids_stride_b < 0 || mask_stride_b < 0 || mask_stride_r < 0))
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: n_extra=%d needs extra_ids and extra_mask with strides >= 0", what, n_extra);
    o = RowExtras{ids, mask, (long)ids_stride_b, (long)mask_stride_b, (long)mask_stride_r, n_extra};
    return LS_OK;
}

// ---- device
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__device__ __forceinline__ long rule_column(const RuleColumn& c, int z) {
    return (c.base ? (long)c.base[z] : 0l) - (c.base_sub ? (long)c.base_sub[z] : 0l) + c.base_add;
}

// Row r's selected extras into `path`, in increasing column (ballot + prefix over 64 mask columns at a time; the running count
// keeps the order); returns their number (<= C).  Called by whole waves, r < rows.
__device__ __forceinline__ int select_path(const RowExtras& e, int z, int r, int lane, int64_t* path) {
    int cnt = 0;
    if (e.C > 0) {                                                     // (uniform)
        const int64_t* ids = e.ids + (long)z * e.ids_sb;
        const int64_t* mask = e.mask + (long)z * e.mask_sb + (long)r * e.mask_sr;
        for (int c0 = 0; c0 < e.C; c0 += LS_WAVE) {
            const int c = c0 + lane;
            const int64_t mk = c < e.C ? mask[c] : 0, id = c < e.C ? ids[c] : 0;      // (two independent loads)
            const bool sel = mk != 0;
            const unsigned long long bal = __ballot(sel);
            const int before = __popcll(bal & ((1ull << lane) - 1ull));
            if (sel) path[cnt + before] = id;                          // cnt + before < C
            cnt += __popcll(bal);
        }
    }
    return cnt;
}
