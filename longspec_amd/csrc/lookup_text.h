// lookup_text.h -- what the two drafters of prompt-lookup speculation share (lookup.hip, lookup_tree.hip): the text of a batch
// row as a prompt part and an output part, and the 64-bit maximum of a wave.
#pragma once
#include "ls_common.h"

namespace {

constexpr int NG_WAVE = 64;

// the row's text: il prompt tokens, w output tokens (both inside their buffers)
struct Text {
    const int64_t* p;
    const int64_t* o;
    int il, L;
    __device__ __forceinline__ int64_t at(int i) const { return i < il ? p[i] : o[i - il]; }   // 0 <= i < L
};

// il_raw prompt tokens and w_raw output tokens as the device holds them: both are clamped to their buffers here
__device__ __forceinline__ Text text_from(const int64_t* prompt_row, int prompt_cols, const int64_t* out_row, int out_cap, long il_raw,
                                          long w_raw) {
    Text t;
    t.p = prompt_row;
    t.o = out_row;
    t.il = il_raw < 0 ? 0 : il_raw > prompt_cols ? prompt_cols : (int)il_raw;
    const int w = w_raw < 0 ? 0 : w_raw > out_cap ? out_cap : (int)w_raw;
    t.L = t.il + w;                                                // <= 2^31 - 2: the host bounds both column counts by 2^30 - 1
    return t;
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, off, NG_WAVE), hi = __shfl_xor((unsigned)(v >> 32), off, NG_WAVE);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

}  // namespace
