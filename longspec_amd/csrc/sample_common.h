// sample_common.h -- what sample.hip (the draw, top-k, top-p), sample_band.hip (min_p, typical_p) and sample_cut.hip
// (top_n_sigma, xtc) share: the per-row selection state, the ordered 16-bit key, the chunk loader and the Philox of
// ls_sample_rows / ls_sample_rows_ex / ls_sample_rows_cut.
#pragma once
#include "ls_common.h"

constexpr int SM_THREADS = 256;
constexpr int SM_CHUNK = 8192;          // logits per workgroup: 32 per thread

struct RowState {
    unsigned lower;                     // ordered 16-bit key: logits below it take no part (0 = all)
    unsigned bin;                       // level 0 result: the high byte that holds the target
    unsigned long long target;          // what is left of the target inside `bin`
    float m;                            // row maximum
    unsigned upper;                     // ordered 16-bit key: logits above it take no part (0xffff = all)
    unsigned pad[2];                    // xtc: [0] the cut key (0 = no cut), [1] the smallest occupied key at or above it
};

__device__ __forceinline__ unsigned order_key(unsigned bits16) {       // as topk.hip: -0.0 and +0.0 share 0x8000
    return (bits16 & 0x8000u) ? 0x8000u - (bits16 & 0x7fffu) : (bits16 | 0x8000u);
}
// the 16-bit pattern of an ordered key (0x8000 -> +0.0)
__device__ __forceinline__ unsigned order_key_bits(unsigned key) {
    return (key & 0x8000u) ? (key & 0x7fffu) : (0x8000u | (0x8000u - key));
}
// the value of an ordered key in the row's 16-bit format
__device__ __forceinline__ float order_key_value(unsigned key, int dtype) {
    const unsigned short h = (unsigned short)order_key_bits(key);
    return dtype == LS_F16 ? (float)__builtin_bit_cast(_Float16, h) : __uint_as_float((unsigned)h << 16);
}
// ordered keys of the smallest and the largest finite value
__device__ __forceinline__ unsigned min_finite_key(int dtype) { return dtype == LS_F16 ? 0x0401u : 0x0081u; }
__device__ __forceinline__ unsigned max_finite_key(int dtype) { return dtype == LS_F16 ? 0xfbffu : 0xff7fu; }

struct Philox {
    unsigned w[4];
};
__device__ __forceinline__ Philox philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox{{c0, c1, c2, c3}};
}

// the 32 logits of a thread: element e = j*8 + i sits at column col0[j] + i
template <typename E>
struct Chunk {
    uint32_t raw[16];
    int col0[4];
    int V;
    __device__ __forceinline__ void load(const typename E::T* src, int base, int V_, int tid) {
        V = V_;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = base + (j * SM_THREADS + tid) * 8;
            col0[j] = c;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (c < V) v = *reinterpret_cast<const uint4*>(src + c);                       // V % 8 == 0: all-in or all-out
            raw[j * 4 + 0] = v.x; raw[j * 4 + 1] = v.y; raw[j * 4 + 2] = v.z; raw[j * 4 + 3] = v.w;
        }
    }
    __device__ __forceinline__ unsigned bits(int e) const { return (raw[e >> 1] >> ((e & 1) * 16)) & 0xffffu; }
    __device__ __forceinline__ float val(int e) const {
        const unsigned short h = (unsigned short)bits(e);
        return E::to_f32(__builtin_bit_cast(typename E::T, h));
    }
    __device__ __forceinline__ bool valid(int e) const { return col0[e >> 3] < V; }
};

// sample_band.hip: the launches of the two band filters, issued by ls_sample_rows_ex between the top-k / top-p selection
// and the key pass.  `state` holds m, lower and upper of every row (sample_select_kernel, level 0, wrote them).
size_t ls_sample_band_bytes(int rows);                                   // counts + prefix sums of typical_p, per call
int ls_sample_minp_launch(int rows, int dtype, float temperature, float min_p, RowState* state, hipStream_t s);
int ls_sample_band_launch(const void* logits, int rows, int vocab, long ld, int dtype, float temperature, float typical_p,
                          RowState* state, void* band_ws, hipStream_t s);

// sample_cut.hip: the launches of the two cuts of ls_sample_rows_cut.  top_n_sigma runs behind the top-k levels and in front
// of the top-p levels (lower = max(lower, key of m - n sigma)); xtc runs behind ls_sample_band_launch and in front of the key
// pass (upper = key of v*, on the rows whose coin fires).  `scratch`: ls_sample_cut_scratch_bytes, rewritten by every call --
// sample.hip hands over its histogram area, which is free between two of its passes, after checking that it is large enough.
size_t ls_sample_cut_scratch_bytes(int rows, int vocab);
int ls_sample_sigma_launch(const void* logits, int rows, int vocab, long ld, int dtype, float n_sigma, RowState* state, void* scratch,
                           hipStream_t s);
int ls_sample_xtc_launch(const void* logits, int rows, int vocab, long ld, int dtype, float temperature, float probability,
                         float threshold, const int64_t* positions, const int32_t* streams, unsigned seed_lo, unsigned seed_hi,
                         RowState* state, void* scratch, hipStream_t s);
