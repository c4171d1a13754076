// sample_cut.hip -- the top_n_sigma and XTC cuts of ls_sample_rows_cut (gfx950 / CDNA4).  Like the band filters of
// sample_band.hip they leave the row's kept set as a band lower <= key <= upper of ordered 16-bit keys in its RowState, which
// sample_key_kernel then draws from.  No counterpart in the reference.
//
// top_n_sigma = n   keep x_j >= m - n sigma, m the row maximum, sigma the population deviation of the row's finite raw 16-bit
//                   logits (not divided by the temperature).  A threshold set that holds the maximum: it runs behind the top-k
//                   levels and in front of the top-p levels, whose mass is then taken over what both kept.
//   sample_sigma_part_kernel    grid (chunks, rows): (count, sum y, sum y^2) of the chunk's finite logits, y = x - m, in double.
//                               Fixed order: a thread's 32 elements in element order, the xor butterfly of the wave (both
//                               operands of every addition are the same pair on both lanes), the four waves in wave order;
//                               one record per chunk, plain stores.
//   sample_sigma_finish_kernel  one thread per row: the chunk records summed in chunk order, sigma = sqrt(S2 / N - (S1 / N)^2),
//                               the smallest key whose value v has v - m >= -n sigma by bisection, lower = max(lower, key).
//
// xtc = (P, theta)  the row's coin: Philox4x32-10, key = the seed's halves, counter (0xFFFFFFFF, position lo, position hi,
//                   stream) -- token noise has counter word 0 = column >> 2 < 2^22 --, u = ((w0 >> 9) + 0.5) 2^-23, the cut
//                   happens iff u < P in fp32.  S = the band kept so far, F(v) = floor(2^40 exp((v - m) / T)) as top-p,
//                   Z = sum_S F; v* = the smallest value occurring in S with F(v*) >= ceil(theta Z); upper = key(v*): every
//                   token of S above v* goes, the ties at v* stay.  No such value, or v* the largest of S: nothing changes.
//   sample_xtc_sum_kernel    grid (chunks, rows): the chunk's integer sum of F over S (plain store)
//   sample_xtc_cut_kernel    one thread per row: Z, the target, the smallest KEY with F >= target by bisection -> pad[0]
//                            (0 = no cut), pad[1] = 0xffffffff
//   sample_xtc_find_kernel   grid (chunks, rows): the smallest occupied key of S that is >= pad[0]: integer atomic minimum on
//                            pad[1]
//   sample_xtc_store_kernel  one thread per row: upper = pad[1] where one was found
// A row whose coin does not fire (and with P = 0 every row) leaves the two grid kernels in front of the chunk load: every
// workgroup forms the coin itself from the row's position and stream.  Every cross-workgroup quantity is an integer or is summed
// in a fixed order; nothing here uses a floating-point atomic.  The partial records live in the histogram area of sample.hip's
// workspace, which is free between two of its passes.
#include "sample_common.h"

namespace {

constexpr int SIGMA_REC = 3;            // doubles per (row, chunk): count, sum y, sum y^2
constexpr unsigned XTC_NONE = 0xffffffffu;

__device__ __forceinline__ double shfl_xor_f64(double v, int off) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = __shfl_xor((unsigned)b, off), hi = __shfl_xor((unsigned)(b >> 32), off);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int off) {
    const unsigned lo = __shfl_xor((unsigned)v, off), hi = __shfl_xor((unsigned)(v >> 32), off);
    return ((unsigned long long)hi << 32) | lo;
}
// ordered key of the row maximum (a value of the 16-bit format), clamped to the finite range (as sample_band.hip)
__device__ __forceinline__ unsigned max_key(float m, int dtype) {
    const unsigned bits = dtype == LS_F16 ? (unsigned)__builtin_bit_cast(unsigned short, (_Float16)m) : __float_as_uint(m) >> 16;
    const unsigned k = order_key(bits);
    return k < max_finite_key(dtype) ? k : max_finite_key(dtype);
}
__device__ __forceinline__ bool finite_f32(float x) { return fabsf(x) < INFINITY; }      // false for NaN too

template <typename E>
__global__ __launch_bounds__(SM_THREADS) void sample_sigma_part_kernel(const typename E::T* __restrict__ logits, long ld, int V,
                                                                       const RowState* __restrict__ state,
                                                                       double* __restrict__ part) {
    __shared__ double s_r[4][SIGMA_REC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, row = blockIdx.y, nchunks = gridDim.x;
    const float mf = state[row].m;
    if (!finite_f32(mf)) return;                         // no finite logit: the finish leaves the row alone too
    Chunk<E> ck;
    ck.load(logits + (long)row * ld, chunk * SM_CHUNK, V, tid);
    const double m = (double)mf;
    double n = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int e = 0; e < 32; ++e) {
        const float x = ck.val(e);
        if (!ck.valid(e) || !finite_f32(x)) continue;
        const double y = (double)x - m;
        n += 1.0;
        s1 += y;
        s2 += y * y;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        n += shfl_xor_f64(n, off);
        s1 += shfl_xor_f64(s1, off);
        s2 += shfl_xor_f64(s2, off);
    }
    if (lane == 0) { s_r[wave][0] = n; s_r[wave][1] = s1; s_r[wave][2] = s2; }
    __syncthreads();
    if (tid < SIGMA_REC)
        part[((long)row * nchunks + chunk) * SIGMA_REC + tid] = ((s_r[0][tid] + s_r[1][tid]) + s_r[2][tid]) + s_r[3][tid];
}

__global__ __launch_bounds__(SM_THREADS) void sample_sigma_finish_kernel(int rows, int nchunks, int dtype, float n_sigma,
                                                                         RowState* __restrict__ state,
                                                                         const double* __restrict__ part) {
    const int row = blockIdx.x * SM_THREADS + threadIdx.x;
    if (row >= rows) return;
    const float mf = state[row].m;
    if (!finite_f32(mf)) return;
    double n = 0.0, s1 = 0.0, s2 = 0.0;
    for (int c = 0; c < nchunks; ++c) {                  // chunk order
        const double* r = part + ((long)row * nchunks + c) * SIGMA_REC;
        n += r[0]; s1 += r[1]; s2 += r[2];
    }
    if (!(n > 0.0)) return;
    const double mean = s1 / n;
    double var = s2 / n - mean * mean;
    if (!(var > 0.0)) var = 0.0;
    const double cut = -((double)n_sigma * sqrt(var));   // keep y >= cut
    const double m = (double)mf;
    unsigned lo = min_finite_key(dtype), hi = max_key(mf, dtype);       // y(m) = 0 >= cut: hi passes
    while (lo < hi) {                                    // the first key that passes
        const unsigned mid = (lo + hi) >> 1;
        if ((double)order_key_value(mid, dtype) - m >= cut) hi = mid;
        else lo = mid + 1;
    }
    if (lo > state[row].lower) state[row].lower = lo;
}

// the row's coin; the same words in every kernel that asks
__device__ __forceinline__ bool xtc_fires(const int64_t* positions, const int32_t* streams, int row, unsigned seed_lo, unsigned seed_hi,
                                          float P) {
    const unsigned long long pos = (unsigned long long)positions[row];
    const unsigned strm = streams ? (unsigned)streams[row] : 0u;
    const Philox r = philox4x32_10(0xFFFFFFFFu, (unsigned)pos, (unsigned)(pos >> 32), strm, seed_lo, seed_hi);
    const float u = ((float)(r.w[0] >> 9) + 0.5f) * 1.1920928955078125e-07f;               // 2^-23: exact, in (0, 1)
    return u < P;
}
__device__ __forceinline__ unsigned long long xtc_weight(double v, double m, double T) {
    return (unsigned long long)(exp((v - m) / T) * 1099511627776.0);                      // 2^40, as top-p; v <= m
}

template <typename E>
__global__ __launch_bounds__(SM_THREADS) void sample_xtc_sum_kernel(const typename E::T* __restrict__ logits, long ld, int V, float T,
                                                                    float P, const int64_t* __restrict__ positions,
                                                                    const int32_t* __restrict__ streams, unsigned seed_lo,
                                                                    unsigned seed_hi, const RowState* __restrict__ state,
                                                                    unsigned long long* __restrict__ part) {
    __shared__ unsigned long long s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, row = blockIdx.y, nchunks = gridDim.x;
    if (!xtc_fires(positions, streams, row, seed_lo, seed_hi, P)) return;                 // (the whole workgroup)
    const float mf = state[row].m;
    if (!finite_f32(mf)) return;
    Chunk<E> ck;
    ck.load(logits + (long)row * ld, chunk * SM_CHUNK, V, tid);
    const unsigned lower = state[row].lower, upper = state[row].upper;
    const double m = (double)mf, Td = (double)T;
    unsigned long long z = 0ull;
#pragma unroll
    for (int e = 0; e < 32; ++e) {
        const unsigned key = order_key(ck.bits(e));
        const float x = ck.val(e);
        if (!ck.valid(e) || !finite_f32(x) || key < lower || key > upper) continue;
        z += xtc_weight((double)x, m, Td);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) z += shfl_xor_u64(z, off);
    if (lane == 0) s_w[wave] = z;
    __syncthreads();
    if (tid == 0) part[(long)row * nchunks + chunk] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

__global__ __launch_bounds__(SM_THREADS) void sample_xtc_cut_kernel(int rows, int nchunks, int dtype, float T, float P, float theta,
                                                                    const int64_t* __restrict__ positions,
                                                                    const int32_t* __restrict__ streams, unsigned seed_lo,
                                                                    unsigned seed_hi, RowState* __restrict__ state,
                                                                    const unsigned long long* __restrict__ part) {
    const int row = blockIdx.x * SM_THREADS + threadIdx.x;
    if (row >= rows) return;
    state[row].pad[0] = 0u;                              // no cut
    state[row].pad[1] = XTC_NONE;
    if (!xtc_fires(positions, streams, row, seed_lo, seed_hi, P)) return;
    const float mf = state[row].m;
    if (!finite_f32(mf)) return;
    unsigned long long Z = 0ull;
    for (int c = 0; c < nchunks; ++c) Z += part[(long)row * nchunks + c];
    // Z = 0: typical_p has moved S so far below m (more than 40 ln 2 T) that every F floors to 0.  Taken literally the rule would
    // let every value qualify (ceil(theta 0) = 0) and keep the smallest alone; a set without measurable mass has no top
    // choices, and the row is left as it is (stated in longspec_hip.h).
    if (Z == 0ull) return;
    unsigned long long target = (unsigned long long)ceil((double)theta * (double)Z);
    if (target < 1ull) target = 1ull;
    const double m = (double)mf, Td = (double)T;
    unsigned lo = state[row].lower > min_finite_key(dtype) ? state[row].lower : min_finite_key(dtype);
    unsigned hi = state[row].upper < max_key(mf, dtype) ? state[row].upper : max_key(mf, dtype);
    if (lo > hi || xtc_weight((double)order_key_value(hi, dtype), m, Td) < target) return;      // nothing qualifies
    while (lo < hi) {                                    // the first key whose weight reaches the target (F rises with the key)
        const unsigned mid = (lo + hi) >> 1;
        if (xtc_weight((double)order_key_value(mid, dtype), m, Td) >= target) hi = mid;
        else lo = mid + 1;
    }
    state[row].pad[0] = lo;                              // >= min_finite_key > 0
}

template <typename E>
__global__ __launch_bounds__(SM_THREADS) void sample_xtc_find_kernel(const typename E::T* __restrict__ logits, long ld, int V,
                                                                     RowState* __restrict__ state) {
    __shared__ unsigned s_k[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, row = blockIdx.y;
    const unsigned cut = state[row].pad[0];
    if (cut == 0u) return;                               // the coin did not fire, or nothing qualifies (the whole workgroup)
    Chunk<E> ck;
    ck.load(logits + (long)row * ld, chunk * SM_CHUNK, V, tid);
    const unsigned lower = state[row].lower > cut ? state[row].lower : cut, upper = state[row].upper;
    unsigned best = XTC_NONE;
#pragma unroll
    for (int e = 0; e < 32; ++e) {
        const unsigned key = order_key(ck.bits(e));
        if (!ck.valid(e) || !finite_f32(ck.val(e)) || key < lower || key > upper) continue;
        best = key < best ? key : best;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned o = __shfl_xor(best, off);
        best = o < best ? o : best;
    }
    if (lane == 0) s_k[wave] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) best = s_k[w] < best ? s_k[w] : best;
        if (best != XTC_NONE) atomicMin(&state[row].pad[1], best);
    }
}

__global__ __launch_bounds__(SM_THREADS) void sample_xtc_store_kernel(int rows, RowState* __restrict__ state) {
    const int row = blockIdx.x * SM_THREADS + threadIdx.x;
    if (row >= rows) return;
    const unsigned found = state[row].pad[1];
    if (state[row].pad[0] != 0u && found != XTC_NONE && found < state[row].upper) state[row].upper = found;
}

}  // namespace

size_t ls_sample_cut_scratch_bytes(int rows, int vocab) {
    const size_t nchunks = ((size_t)vocab + SM_CHUNK - 1) / SM_CHUNK;
    return (size_t)rows * nchunks * SIGMA_REC * sizeof(double);          // the larger of the two records
}

int ls_sample_sigma_launch(const void* logits, int rows, int vocab, long ld, int dtype, float n_sigma, RowState* state, void* scratch,
                           hipStream_t s) {
    const int nchunks = (vocab + SM_CHUNK - 1) / SM_CHUNK;
    const dim3 grid(nchunks, rows), block(SM_THREADS);
    double* part = static_cast<double*>(scratch);
    if (dtype == LS_F16)
        hipLaunchKernelGGL(sample_sigma_part_kernel<ElemF16>, grid, block, 0, s, static_cast<const _Float16*>(logits), ld, vocab, state,
                           part);
    else
        hipLaunchKernelGGL(sample_sigma_part_kernel<ElemBF16>, grid, block, 0, s, static_cast<const __bf16*>(logits), ld, vocab, state,
                           part);
    LS_CHECK_LAUNCH("sample_sigma_part_kernel");
    hipLaunchKernelGGL(sample_sigma_finish_kernel, dim3((rows + SM_THREADS - 1) / SM_THREADS), block, 0, s, rows, nchunks, dtype,
                       n_sigma, state, part);
    LS_CHECK_LAUNCH("sample_sigma_finish_kernel");
    return LS_OK;
}

int ls_sample_xtc_launch(const void* logits, int rows, int vocab, long ld, int dtype, float temperature, float probability,
                         float threshold, const int64_t* positions, const int32_t* streams, unsigned seed_lo, unsigned seed_hi,
                         RowState* state, void* scratch, hipStream_t s) {
    const int nchunks = (vocab + SM_CHUNK - 1) / SM_CHUNK;
    const dim3 grid(nchunks, rows), block(SM_THREADS), per_row((rows + SM_THREADS - 1) / SM_THREADS);
    unsigned long long* part = static_cast<unsigned long long*>(scratch);
    if (dtype == LS_F16)
        hipLaunchKernelGGL(sample_xtc_sum_kernel<ElemF16>, grid, block, 0, s, static_cast<const _Float16*>(logits), ld, vocab,
                           temperature, probability, positions, streams, seed_lo, seed_hi, state, part);
    else
        hipLaunchKernelGGL(sample_xtc_sum_kernel<ElemBF16>, grid, block, 0, s, static_cast<const __bf16*>(logits), ld, vocab,
                           temperature, probability, positions, streams, seed_lo, seed_hi, state, part);
    LS_CHECK_LAUNCH("sample_xtc_sum_kernel");
    hipLaunchKernelGGL(sample_xtc_cut_kernel, per_row, block, 0, s, rows, nchunks, dtype, temperature, probability, threshold,
                       positions, streams, seed_lo, seed_hi, state, part);
    LS_CHECK_LAUNCH("sample_xtc_cut_kernel");
    if (dtype == LS_F16)
        hipLaunchKernelGGL(sample_xtc_find_kernel<ElemF16>, grid, block, 0, s, static_cast<const _Float16*>(logits), ld, vocab, state);
    else
        hipLaunchKernelGGL(sample_xtc_find_kernel<ElemBF16>, grid, block, 0, s, static_cast<const __bf16*>(logits), ld, vocab, state);
    LS_CHECK_LAUNCH("sample_xtc_find_kernel");
    hipLaunchKernelGGL(sample_xtc_store_kernel, per_row, block, 0, s, rows, state);
    LS_CHECK_LAUNCH("sample_xtc_store_kernel");
    return LS_OK;
}
