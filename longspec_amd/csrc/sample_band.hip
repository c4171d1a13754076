// sample_band.hip -- the min_p and typical_p filters of ls_sample_rows_ex (gfx950 / CDNA4): they run after the top-k / top-p
// selection of sample.hip and leave the row's kept set as a band lower <= key <= upper of ordered 16-bit keys in its RowState,
// which sample_key_kernel then draws from.  No counterpart in the reference.
//
// min_p       keep v iff w(v) = exp((v - m) / T) >= min_p (m the row maximum): w is monotone in v, so the filter is the
//             smallest 16-bit value that passes -- a bisection over the ordered keys, one thread per row, same double
//             precision exp as the top-p weights.  lower = max(lower, that key).
// typical_p   S = what is kept so far.  With a(v) = (m - v) / T >= 0, q(v) = exp(-a(v)) / Z and A = sum_S q a, the surprise of v
//             is ln Z + a(v) and the entropy ln Z + A: ln Z cancels and the distance is d(v) = |a(v) - A|.  The logits are
//             16-bit, so the counts n(v) of the 2^16 ordered keys describe the row:
//   sample_count_kernel   one workgroup per row: n(v) of the finite logits in S, a quarter of the key space at a time in LDS
//                         (integer LDS atomics), written out with plain stores
//   sample_band_kernel    one workgroup per row, 64 keys per thread:
//       1. F(v) = floor(2^40 exp(-a(v))) as in top-p, G(v) = floor(F(v) a(v)); Z = sum n F, E = sum n G and the inclusive
//          prefix sums of n F over the keys, all in unsigned 64-bit integers: order-free, exact.
//          Width: x e^-x <= 1/e, so G < 2^40 / e < 2^39 and E < 2^24 * 2^39 = 2^63 for every vocabulary ls_sample_rows takes
//          (<= 2^24); Z <= 2^24 * 2^40 as in top-p.  A = E / Z in double.
//       2. The kernel measures distances scaled by T: D(v) = |(m - v) - A T| (no division per key; D = T d up to 2^-52
//          relative).  mass(D) = sum n F over {v in S : D(v) <= D} is a step function of D whose steps are the D(v), and
//          {D(v) <= D} is a run [lo(D), hi(D)] of keys found by two bisections (m - v is monotone in the key), its mass a
//          difference of two prefix sums.  D* = the smallest double with mass(D*) >= ceil(typical_p Z): a 256-ary search
//          over the 8 bytes of the (non-negative) double's bit pattern, one candidate per thread and level.
//       3. lower = lo(D*), upper = hi(D*).  Ties at D* are all inside; the band holds at least the value that attains D*.
// A row without a finite logit is left alone (lower = 0, upper = 0xffff: everything is kept, as in ls_sample_rows).
// Error of A against the exact value: each F and each G is off by < 1 unit of 2^-40 (+ 2^-52 relative), a(v) < 27.8 wherever
// F(v) > 0 and the omitted terms (F = 0) are below 27.8 * 2^-40 each, Z >= 2^40 (S holds the maximum), A <= ln |S|:
// |A - A_exact| <= V 2^-40 (29 + ln V) < 2^-16 for V <= 2^18 -- the delta of the tests.
#include "sample_common.h"

namespace {

constexpr int COUNT_THREADS = 1024;
constexpr int BAND_THREADS = 1024;
constexpr int BAND_KEYS = 65536 / BAND_THREADS;          // 64 consecutive ordered keys per thread
constexpr unsigned long long INF_BITS = 0x7ff0000000000000ull;

// n(v) of one row: one workgroup, four passes over the row, each counting one quarter of the key space in a 64 KiB LDS table
// (integer LDS atomics) and writing it out with plain stores -- every entry of the row's table is written, nothing has to be
// cleared beforehand and no two workgroups meet in a cache line.  Finite logits with lower <= key <= upper count.
__global__ __launch_bounds__(COUNT_THREADS) void sample_count_kernel(const unsigned short* __restrict__ logits, long ld, int V, int dtype,
                                                                     const RowState* __restrict__ state, unsigned* __restrict__ counts) {
    __shared__ unsigned s_n[16384];
    const int tid = threadIdx.x, row = blockIdx.x;
    const unsigned short* src = logits + (long)row * ld;
    unsigned lo = state[row].lower, hi = state[row].upper;
    if (lo < min_finite_key(dtype)) lo = min_finite_key(dtype);
    if (hi > max_finite_key(dtype)) hi = max_finite_key(dtype);
    unsigned* c = counts + (size_t)row * 65536;
    for (unsigned quarter = 0; quarter < 4; ++quarter) {
        for (int i = tid; i < 16384; i += COUNT_THREADS) s_n[i] = 0u;
        __syncthreads();
        if (lo <= hi && (quarter << 14) <= hi && ((quarter + 1) << 14) > lo) {               // the same for every thread
            for (int col = tid * 8; col < V; col += COUNT_THREADS * 8) {                     // V % 8 == 0: eight columns inside
                const uint4 v = *reinterpret_cast<const uint4*>(src + col);
                const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const unsigned key = order_key((w[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
                    if (key >= lo && key <= hi && (key >> 14) == quarter) atomicAdd(&s_n[key & 16383u], 1u);
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < 16384; i += COUNT_THREADS) c[(quarter << 14) + i] = s_n[i];
        __syncthreads();
    }
}

// ordered key of the row maximum (a value of the 16-bit format), clamped to the finite range
__device__ __forceinline__ unsigned max_key(float m, int dtype) {
    const unsigned bits = dtype == LS_F16 ? (unsigned)__builtin_bit_cast(unsigned short, (_Float16)m) : __float_as_uint(m) >> 16;
    const unsigned k = order_key(bits);
    return k < max_finite_key(dtype) ? k : max_finite_key(dtype);
}

__global__ __launch_bounds__(SM_THREADS) void sample_minp_kernel(int rows, int dtype, float T, float min_p,
                                                                 RowState* __restrict__ state) {
    const int row = blockIdx.x * SM_THREADS + threadIdx.x;
    if (row >= rows) return;
    const float mf = state[row].m;
    if (!(mf > -INFINITY)) return;                       // no finite logit: the row stays as it is
    const double m = (double)mf, Td = (double)T, p = (double)min_p;
    unsigned lo = min_finite_key(dtype), hi = max_key(mf, dtype);       // w(m) = 1 >= min_p: hi passes
    while (lo < hi) {                                    // the first key that passes
        const unsigned mid = (lo + hi) >> 1;
        if (exp(((double)order_key_value(mid, dtype) - m) / Td) >= p) hi = mid;
        else lo = mid + 1;
    }
    if (lo > state[row].lower) state[row].lower = lo;
}

__device__ __forceinline__ unsigned long long shfl_up64(unsigned long long v, int off) {
    const unsigned lo = __shfl_up((unsigned)v, off), hi = __shfl_up((unsigned)(v >> 32), off);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl_xor64b(unsigned long long v, int off) {
    const unsigned lo = __shfl_xor((unsigned)v, off), hi = __shfl_xor((unsigned)(v >> 32), off);
    return ((unsigned long long)hi << 32) | lo;
}

struct Band {
    unsigned lo, hi;                                     // empty when lo > hi
};
// {k in [klo, kmax] : |(m - value(k)) - C| <= D}: (m - value) falls as k grows, so each side is one bisection
__device__ __forceinline__ Band band_of(double D, double m, double C, unsigned klo, unsigned kmax, int dtype) {
    unsigned a = klo, b = kmax + 1;                      // the first key with C - (m - v) > D
    while (a < b) {
        const unsigned mid = (a + b) >> 1;
        if (C - (m - (double)order_key_value(mid, dtype)) <= D) a = mid + 1;
        else b = mid;
    }
    const unsigned end = a;
    a = klo; b = kmax + 1;                               // the first key with (m - v) - C <= D
    while (a < b) {
        const unsigned mid = (a + b) >> 1;
        if ((m - (double)order_key_value(mid, dtype)) - C <= D) b = mid;
        else a = mid + 1;
    }
    return Band{a, end - 1};                             // end >= klo >= 1
}

__global__ __launch_bounds__(BAND_THREADS) void sample_band_kernel(int dtype, float T, float typical_p, RowState* __restrict__ state,
                                                                   const unsigned* __restrict__ counts,
                                                                   unsigned long long* __restrict__ prefix) {
    __shared__ unsigned long long s_off[BAND_THREADS];   // weight of the keys below the thread's 64
    __shared__ unsigned long long s_wz[16], s_wg[16];
    __shared__ int s_nf[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.x;
    const float mf = state[row].m;
    if (!(mf > -INFINITY)) return;                       // no finite logit (the whole workgroup leaves)
    const double m = (double)mf, Td = (double)T;
    const unsigned klo = state[row].lower > min_finite_key(dtype) ? state[row].lower : min_finite_key(dtype);
    const unsigned kmax = max_key(mf, dtype);
    if (klo > kmax) return;
    const unsigned* cr = counts + (size_t)row * 65536;
    unsigned long long* pr = prefix + (size_t)row * 65536;
    // 1. weights, sums and prefix sums
    unsigned long long z = 0ull, g = 0ull;
    const unsigned k0 = (unsigned)tid * BAND_KEYS;
    if (k0 + BAND_KEYS > klo && k0 <= kmax) {
        for (int i = 0; i < BAND_KEYS; i += 4) {
            const uint4 n4 = *reinterpret_cast<const uint4*>(cr + k0 + i);
            const unsigned n[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned key = k0 + i + j;
                if (n[j] && key >= klo && key <= kmax) {
                    const double e = ((double)order_key_value(key, dtype) - m) / Td;       // <= 0
                    const unsigned long long F = (unsigned long long)(exp(e) * 1099511627776.0);          // 2^40, as top-p
                    const unsigned long long G = (unsigned long long)((double)F * (-e));                  // < 2^39
                    z += (unsigned long long)n[j] * F;
                    g += (unsigned long long)n[j] * G;
                }
                pr[key] = z;
            }
        }
    }
    unsigned long long incl = z;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = shfl_up64(incl, off);
        if (lane >= off) incl += o;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) g += shfl_xor64b(g, off);
    if (lane == 63) s_wz[wave] = incl;
    if (lane == 0) s_wg[wave] = g;
    __syncthreads();
    unsigned long long Z = 0ull, Esum = 0ull, woff = 0ull;
    for (int q = 0; q < 16; ++q) {
        if (q < wave) woff += s_wz[q];
        Z += s_wz[q];
        Esum += s_wg[q];
    }
    s_off[tid] = woff + incl - z;
    __threadfence_block();                               // the prefix sums are read back by other threads below
    __syncthreads();
    if (Z == 0ull) return;                               // cannot happen while S holds the maximum
    const double C = (double)Esum / (double)Z * Td;      // A T
    unsigned long long target = (unsigned long long)ceil((double)typical_p * (double)Z);
    if (target < 1ull) target = 1ull;
    if (target > Z) target = Z;
    // 2. the smallest D with mass(D) >= target: byte by byte, thread t < 256 tries byte t (the largest D of its bucket)
    unsigned long long pre = 0ull;
    for (int level = 7; level >= 0; --level) {
        const int shift = level * 8;
        bool infeasible = false;
        if (tid < 256) {
            unsigned long long cand = pre | ((unsigned long long)tid << shift) | ((1ull << shift) - 1ull);
            if (cand > INF_BITS) cand = INF_BITS;        // +inf takes every key: the last bucket always reaches the target
            const Band bd = band_of(__longlong_as_double((long long)cand), m, C, klo, kmax, dtype);
            unsigned long long mass = 0ull;
            if (bd.lo <= bd.hi) {
                mass = pr[bd.hi] + s_off[bd.hi / BAND_KEYS];
                if (bd.lo > klo) mass -= pr[bd.lo - 1] + s_off[(bd.lo - 1) / BAND_KEYS];
            }
            infeasible = mass < target;
        }
        const unsigned long long bal = __ballot(infeasible);
        if (lane == 0 && wave < 4) s_nf[wave] = __popcll(bal);
        __syncthreads();
        const int nf = (s_nf[0] + s_nf[1]) + (s_nf[2] + s_nf[3]);      // mass is monotone in D: the first byte that reaches it
        __syncthreads();
        pre |= (unsigned long long)(nf < 255 ? nf : 255) << shift;
    }
    // 3. the band of D*
    if (tid == 0) {
        const Band bd = band_of(__longlong_as_double((long long)pre), m, C, klo, kmax, dtype);
        if (bd.lo <= bd.hi) {
            state[row].lower = bd.lo;
            state[row].upper = bd.hi;
        }
    }
}

}  // namespace

size_t ls_sample_band_bytes(int rows) { return (size_t)rows * 65536 * (sizeof(unsigned) + sizeof(unsigned long long)); }

int ls_sample_minp_launch(int rows, int dtype, float temperature, float min_p, RowState* state, hipStream_t s) {
    hipLaunchKernelGGL(sample_minp_kernel, dim3((rows + SM_THREADS - 1) / SM_THREADS), dim3(SM_THREADS), 0, s, rows, dtype,
                       temperature, min_p, state);
    LS_CHECK_LAUNCH("sample_minp_kernel");
    return LS_OK;
}

int ls_sample_band_launch(const void* logits, int rows, int vocab, long ld, int dtype, float temperature, float typical_p,
                          RowState* state, void* band_ws, hipStream_t s) {
    unsigned* counts = static_cast<unsigned*>(band_ws);
    unsigned long long* prefix = reinterpret_cast<unsigned long long*>(counts + (size_t)rows * 65536);
    hipLaunchKernelGGL(sample_count_kernel, dim3(rows), dim3(COUNT_THREADS), 0, s, static_cast<const unsigned short*>(logits), ld, vocab,
                       dtype, state, counts);
    LS_CHECK_LAUNCH("sample_count_kernel");
    hipLaunchKernelGGL(sample_band_kernel, dim3(rows), dim3(BAND_THREADS), 0, s, dtype, temperature, typical_p, state, counts,
                       prefix);
    LS_CHECK_LAUNCH("sample_band_kernel");
    return LS_OK;
}
