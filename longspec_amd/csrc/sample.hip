// sample.hip -- one draw per row from the tempered, top-k / top-p filtered distribution of the lm_head logits
// (gfx950 / CDNA4).  No counterpart in the reference: its temperature > 0 paths stay in tree.hip / ops.py as they are.
//
// A row's draw is the Gumbel-max of its kept logits, with noise keyed by (seed, stream, position, column) through
// Philox4x32-10: key_j = x_j / T - ln(-ln u_j), the result is the kept column with the largest key (ties to the smaller
// column).  Nothing of a row's result depends on the other rows, the row count, the grid or the run: every cross-workgroup
// quantity is an integer sum (order-free) or a maximum of unique 64-bit keys.
//
// The kept set is a threshold set {x_j >= t}.  t comes from a weighted rank selection on the ordered 16-bit pattern of the
// logits, two 256-bin radix levels, run once per filter:
//   top-k   weight 1 per logit, target min(k, finite logits): t_k = the k-th largest value (ties all kept);
//   top-p   weight F(x) = floor(2^40 * exp((x - x_max) / T)) (double precision exp, unsigned 64-bit fixed point) per logit
//           >= t_k, target ceil(p * sum F): t_p = the largest value v with sum_{x >= v} F >= target.
// Integer weights make the sum over the tokens of a value EQUAL n(v) * F(v), and the coarse level consistent with the fine
// one, whatever the order of the additions.  A -inf logit carries no weight and is never kept while the row has a finite one.
//
//   sample_hist_kernel    grid (chunks of 8192 logits, rows): 256-bin weight histogram of the chunk at one radix level
//                         (LDS integer atomics), chunk maximum
//   sample_select_kernel  grid (rows): bin sums over the chunks, the bin that holds the target, the residual target
//   sample_key_kernel     grid (chunks, rows): Philox + Gumbel keys of the kept logits, the chunk's two best, kept count,
//                         smallest kept value
//   sample_merge_kernel   one thread per row: the row's two best over its chunks, outputs
// Filters off: the last two launches only.  top-k: + 4.  top-p: + 6 (the first pair finds x_max).
//
// ls_sample_rows_ex adds min_p (one more lower bound) and typical_p (a band [lower, upper] of values that may exclude the
// maximum): their kernels are in sample_band.hip and run between the selections above and the key pass, which honours
// `upper` as well as `lower` and reports the largest kept value.  With both off the launches are the ones listed here.
//
// ls_sample_rows_cut adds top_n_sigma (a lower bound from the raw logits, behind the top-k levels and in front of the top-p
// levels) and xtc (an upper bound on the rows whose coin fires, last in front of the key pass): sample_cut.hip.  With both off,
// again, the launches are the ones listed here.
#include "sample_common.h"

namespace {

constexpr int SM_REC_WORDS = 8;         // candidate record of (row, chunk), 32-bit words: best (2), second (2), finite kept, -inf kept, min kept, max kept

__device__ __forceinline__ unsigned order_key32(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key32_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// mode 0: weight 1; mode 1: weight F(x).  level 0: bin = high byte; level 1: low byte of the logits whose high byte is st.bin
template <typename E>
__global__ __launch_bounds__(SM_THREADS) void sample_hist_kernel(const typename E::T* __restrict__ logits, long ld, int V, int level,
                                                                 int mode, float T, const RowState* __restrict__ state,
                                                                 unsigned long long* __restrict__ hist, float* __restrict__ chunk_max) {
    __shared__ unsigned long long s_hist[256];
    __shared__ float s_red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, row = blockIdx.y, nchunks = gridDim.x;
    Chunk<E> ck;
    ck.load(logits + (long)row * ld, chunk * SM_CHUNK, V, tid);
    s_hist[tid] = 0ull;
    const bool first = level == 0 && mode == 0;          // the launch that nothing precedes: the state is not read
    const unsigned lower = first ? 0u : state[row].lower;
    const unsigned prefix = level ? state[row].bin : 0u;
    const double m = mode ? (double)state[row].m : 0.0;
    if (first) {
        float cm = -INFINITY;
#pragma unroll
        for (int e = 0; e < 32; ++e)
            if (ck.valid(e)) cm = fmaxf(cm, ck.val(e));
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cm = fmaxf(cm, __shfl_xor(cm, off));
        if (lane == 0) s_red[wave] = cm;
    }
    __syncthreads();
    if (first && tid == 0) chunk_max[(long)row * nchunks + chunk] = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
#pragma unroll
    for (int e = 0; e < 32; ++e) {
        const unsigned key = order_key(ck.bits(e));
        const float x = ck.val(e);
        if (!ck.valid(e) || x == -INFINITY || key < lower) continue;
        if (level && (key >> 8) != prefix) continue;
        unsigned long long w = 1ull;
        if (mode) w = (unsigned long long)(exp(((double)x - m) / (double)T) * 1099511627776.0);     // 2^40; x <= m
        atomicAdd(&s_hist[level ? (key & 255u) : (key >> 8)], w);
    }
    __syncthreads();
    hist[((long)row * nchunks + chunk) * 256 + tid] = s_hist[tid];
}

__device__ __forceinline__ unsigned long long shfl_down64(unsigned long long v, int off) {
    const unsigned lo = __shfl_down((unsigned)v, off), hi = __shfl_down((unsigned)(v >> 32), off);
    return ((unsigned long long)hi << 32) | lo;
}

// One workgroup per row, one thread per bin.  Level 0 fixes the target and the high byte; level 1 the threshold key, which
// becomes the row's `lower`.  A row without weight (all -inf) keeps lower = 0: everything is kept.
__global__ __launch_bounds__(SM_THREADS) void sample_select_kernel(int level, int mode, int k, float p, int nchunks,
                                                                   RowState* __restrict__ state,
                                                                   const unsigned long long* __restrict__ hist,
                                                                   const float* __restrict__ chunk_max) {
    __shared__ unsigned long long s_wave[4];
    __shared__ float s_cm[4];
    const int tid = threadIdx.x, row = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long w = 0ull;
#pragma unroll 8
    for (int c = 0; c < nchunks; ++c) w += hist[((long)row * nchunks + c) * 256 + tid];
    float cm = -INFINITY;                                // the row maximum, from the chunk maxima (first launch only)
    if (level == 0 && mode == 0)
        for (int c = tid; c < nchunks; c += SM_THREADS) cm = fmaxf(cm, chunk_max[(long)row * nchunks + c]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cm = fmaxf(cm, __shfl_xor(cm, off));
    if (lane == 0) s_cm[wave] = cm;
    // weight of this bin and the bins beyond it: suffix sums inside the wave, then the totals of the waves above
    unsigned long long incl = w;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = shfl_down64(incl, off);
        if (lane + off < 64) incl += o;
    }
    if (lane == 0) s_wave[wave] = incl;
    __syncthreads();
    for (int q = wave + 1; q < 4; ++q) incl += s_wave[q];
    const unsigned long long above = incl - w;
    const unsigned long long total = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
    unsigned long long target;
    if (level) {
        target = state[row].target;
    } else if (mode == 0) {
        target = (unsigned long long)k < total ? (unsigned long long)k : total;
    } else {
        target = (unsigned long long)ceil((double)p * (double)total);
        if (target < 1ull) target = 1ull;
        if (target > total) target = total;
    }
    if (level == 0 && mode == 0 && tid == 0) {
        state[row].m = fmaxf(fmaxf(s_cm[0], s_cm[1]), fmaxf(s_cm[2], s_cm[3]));
        state[row].lower = 0u;
        state[row].upper = 0xffffu;
    }
    if (total == 0ull) {
        if (tid == 0 && level == 0) { state[row].bin = 0u; state[row].target = 0ull; }
        return;
    }
    if (incl >= target && above < target) {              // exactly one bin
        if (level == 0) {
            state[row].bin = (unsigned)tid;
            state[row].target = target - above;
        } else {
            state[row].lower = (state[row].bin << 8) | (unsigned)tid;
        }
    }
}

__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int off) {
    const unsigned lo = __shfl_xor((unsigned)v, off), hi = __shfl_xor((unsigned)(v >> 32), off);
    return ((unsigned long long)hi << 32) | lo;
}
// two best of the union of two (best, second) pairs; keys are unique or 0 (= none)
__device__ __forceinline__ void top2_merge(unsigned long long& a1, unsigned long long& a2, unsigned long long b1, unsigned long long b2) {
    const unsigned long long hi = a1 > b1 ? a1 : b1, lo = a1 > b1 ? b1 : a1;
    const unsigned long long s = a2 > b2 ? a2 : b2;
    a1 = hi;
    a2 = lo > s ? lo : s;
}

template <typename E>
__global__ __launch_bounds__(SM_THREADS) void sample_key_kernel(const typename E::T* __restrict__ logits, long ld, int V,
                                                                const int64_t* __restrict__ positions,
                                                                const int32_t* __restrict__ streams, unsigned seed_lo,
                                                                unsigned seed_hi, float T, int filtered,
                                                                const RowState* __restrict__ state, unsigned* __restrict__ cand) {
    __shared__ unsigned long long s_b[8];
    __shared__ int s_n[8];
    __shared__ float s_min[4], s_max[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, row = blockIdx.y, nchunks = gridDim.x;
    Chunk<E> ck;
    ck.load(logits + (long)row * ld, chunk * SM_CHUNK, V, tid);
    const unsigned lower = filtered ? state[row].lower : 0u;
    const unsigned upper = filtered ? state[row].upper : 0xffffu;
    const unsigned long long pos = (unsigned long long)positions[row];
    const unsigned strm = streams ? (unsigned)streams[row] : 0u;
    unsigned long long b1 = 0ull, b2 = 0ull;             // (ordered fp32 key << 32) | ~column
    int n_fin = 0, n_inf = 0;
    float vmin = INFINITY, vmax = -INFINITY;
#pragma unroll
    for (int q = 0; q < 8; ++q) {                        // 4 consecutive columns share one Philox block
        const int c = ck.col0[q >> 1] + (q & 1) * 4;
        if (c >= V) continue;
        const Philox r = philox4x32_10((unsigned)c >> 2, (unsigned)pos, (unsigned)(pos >> 32), strm, seed_lo, seed_hi);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = q * 4 + i;
            const unsigned k16 = order_key(ck.bits(e));
            if (k16 < lower || k16 > upper) continue;
            const float x = ck.val(e);
            const float u = ((float)(r.w[i] >> 9) + 0.5f) * 1.1920928955078125e-07f;       // 2^-23: exact, in (0, 1)
            const float key = x / T - logf(-logf(u));
            const unsigned long long pk = ((unsigned long long)order_key32(key) << 32) | (0xffffffffu - (unsigned)(c + i));
            if (pk > b1) { b2 = b1; b1 = pk; }
            else if (pk > b2) b2 = pk;
            if (x == -INFINITY) ++n_inf;
            else { ++n_fin; vmin = fminf(vmin, x); vmax = fmaxf(vmax, x); }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        top2_merge(b1, b2, shfl_xor64(b1, off), shfl_xor64(b2, off));
        n_fin += __shfl_xor(n_fin, off);
        n_inf += __shfl_xor(n_inf, off);
        vmin = fminf(vmin, __shfl_xor(vmin, off));
        vmax = fmaxf(vmax, __shfl_xor(vmax, off));
    }
    if (lane == 0) {
        s_b[wave * 2] = b1; s_b[wave * 2 + 1] = b2;
        s_n[wave * 2] = n_fin; s_n[wave * 2 + 1] = n_inf;
        s_min[wave] = vmin;
        s_max[wave] = vmax;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) {
            top2_merge(b1, b2, s_b[w * 2], s_b[w * 2 + 1]);
            n_fin += s_n[w * 2];
            n_inf += s_n[w * 2 + 1];
            vmin = fminf(vmin, s_min[w]);
            vmax = fmaxf(vmax, s_max[w]);
        }
        unsigned* rec = cand + ((long)row * nchunks + chunk) * SM_REC_WORDS;
        rec[0] = (unsigned)b1; rec[1] = (unsigned)(b1 >> 32);
        rec[2] = (unsigned)b2; rec[3] = (unsigned)(b2 >> 32);
        rec[4] = (unsigned)n_fin; rec[5] = (unsigned)n_inf;
        rec[6] = __float_as_uint(vmin); rec[7] = __float_as_uint(vmax);
    }
}

__global__ __launch_bounds__(SM_THREADS) void sample_merge_kernel(const unsigned* __restrict__ cand, int rows, int nchunks,
                                                                  int64_t* __restrict__ out_idx, int64_t* __restrict__ top2_idx,
                                                                  float* __restrict__ top2_key, int32_t* __restrict__ out_kept,
                                                                  float* __restrict__ out_thr, float* __restrict__ out_upper) {
    const int row = blockIdx.x * SM_THREADS + threadIdx.x;
    if (row >= rows) return;
    unsigned long long b1 = 0ull, b2 = 0ull;
    long n_fin = 0, n_inf = 0;
    float vmin = INFINITY, vmax = -INFINITY;
    for (int c = 0; c < nchunks; ++c) {
        const unsigned* rec = cand + ((long)row * nchunks + c) * SM_REC_WORDS;
        top2_merge(b1, b2, ((unsigned long long)rec[1] << 32) | rec[0], ((unsigned long long)rec[3] << 32) | rec[2]);
        n_fin += rec[4];
        n_inf += rec[5];
        vmin = fminf(vmin, __uint_as_float(rec[6]));
        vmax = fmaxf(vmax, __uint_as_float(rec[7]));
    }
    // -inf logits (key -inf) only count while the row has no finite logit at all
    const long kept = n_fin > 0 ? n_fin : n_inf;
    if (kept < 2) b2 = 0ull;
    out_idx[row] = (int64_t)(0xffffffffu - (unsigned)b1);
    if (top2_idx) {
        top2_idx[row * 2] = (int64_t)(0xffffffffu - (unsigned)b1);
        top2_idx[row * 2 + 1] = b2 ? (int64_t)(0xffffffffu - (unsigned)b2) : -1;
    }
    if (top2_key) {
        top2_key[row * 2] = key32_value((unsigned)(b1 >> 32));
        top2_key[row * 2 + 1] = b2 ? key32_value((unsigned)(b2 >> 32)) : -INFINITY;
    }
    if (out_kept) out_kept[row] = (int32_t)kept;
    if (out_thr) out_thr[row] = n_fin > 0 ? vmin : -INFINITY;
    if (out_upper) out_upper[row] = vmax;                // -inf for a row without a finite logit
}

struct SampleWs {
    size_t state, cmax, hist, cand, total;
};
SampleWs sample_ws(int rows, int vocab) {
    const size_t nchunks = ((size_t)vocab + SM_CHUNK - 1) / SM_CHUNK;
    SampleWs w;
    w.state = 0;
    w.hist = (size_t)rows * sizeof(RowState);
    w.cand = w.hist + (size_t)rows * nchunks * 256 * sizeof(unsigned long long);
    w.cmax = w.cand + (size_t)rows * nchunks * SM_REC_WORDS * sizeof(unsigned);
    w.total = w.cmax + ((size_t)rows * nchunks * sizeof(float) + 15) / 16 * 16;
    return w;
}

// All three entry points: d.min_p = 0 and d.typical_p = 1 issue the launches of ls_sample_rows and nothing else, and so does a
// `cut` that is NULL or has both of its filters off.
int sample_run(const ls_sample_desc& d, const ls_sample_cut* cut, void* workspace, size_t workspace_bytes, void* stream,
               const char* who) {
    const void* logits = d.logits;
    const int rows = d.rows, vocab = d.vocab, dtype = d.dtype, top_k = d.top_k;
    const int64_t ld = d.ld;
    const float temperature = d.temperature, top_p = d.top_p;
    if (!logits || !d.positions || !d.out_idx || !workspace) LS_FAIL(LS_ERR_INVALID_ARG, "%s: null pointer", who);
    if (dtype != LS_F16 && dtype != LS_BF16) LS_FAIL(LS_ERR_INVALID_ARG, "%s: dtype", who);
    if (rows < 1 || rows > 65535 || vocab < 8 || vocab > (1 << 24) || vocab % 8 != 0 || ld < vocab || ld % 8 != 0)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: rows=%d vocab=%d ld=%ld (vocab and ld must be multiples of 8, rows <= 65535, "
                "vocab <= 2^24)", who, rows, vocab, (long)ld);
    if (!(temperature > 0.f) || top_k < 0 || !(top_p > 0.f) || !(top_p <= 1.f))
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: temperature=%g (> 0), top_k=%d (>= 0), top_p=%g (0 < p <= 1)", who, (double)temperature,
                top_k, (double)top_p);
    if (!(d.min_p >= 0.f) || !(d.min_p <= 1.f) || !(d.typical_p > 0.f) || !(d.typical_p <= 1.f))
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: min_p=%g (0 <= min_p <= 1), typical_p=%g (0 < typical_p <= 1)", who, (double)d.min_p,
                (double)d.typical_p);
    if (reinterpret_cast<uintptr_t>(logits) % 16 != 0 || reinterpret_cast<uintptr_t>(workspace) % 16 != 0)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: logits and workspace must be 16-byte aligned", who);
    if (cut && (!(cut->top_n_sigma >= 0.f) || !(cut->top_n_sigma < INFINITY) || !(cut->xtc_probability >= 0.f) ||
                !(cut->xtc_probability <= 1.f) || !(cut->xtc_threshold > 0.f) || !(cut->xtc_threshold <= 1.f) || cut->reserved != 0))
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: top_n_sigma=%g (finite, >= 0), xtc_probability=%g (0 <= P <= 1), xtc_threshold=%g "
                "(0 < theta <= 1), reserved=%d (0)", who, (double)cut->top_n_sigma, (double)cut->xtc_probability,
                (double)cut->xtc_threshold, (int)cut->reserved);
    const SampleWs w = sample_ws(rows, vocab);
    const bool use_k = top_k > 0 && top_k < vocab, use_p = top_p < 1.f, use_m = d.min_p > 0.f, use_t = d.typical_p < 1.f;
    const bool use_s = cut && cut->top_n_sigma > 0.f, use_x = cut && cut->xtc_probability > 0.f;
    if (workspace_bytes < w.total + (use_t ? ls_sample_band_bytes(rows) : 0)) LS_FAIL(LS_ERR_WORKSPACE, "%s: workspace too small", who);
    if ((use_s || use_x) && ls_sample_cut_scratch_bytes(rows, vocab) > w.cand - w.hist)      // the cuts' records live in `hist`
        LS_FAIL(LS_ERR_WORKSPACE, "%s: the histogram area does not hold the partial records of the cuts", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(workspace);
    RowState* state = reinterpret_cast<RowState*>(base + w.state);
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(base + w.hist);
    unsigned* cand = reinterpret_cast<unsigned*>(base + w.cand);
    float* cmax = reinterpret_cast<float*>(base + w.cmax);
    const int nchunks = (vocab + SM_CHUNK - 1) / SM_CHUNK;
    const dim3 grid(nchunks, rows), block(SM_THREADS);
    auto hist_pass = [&](int level, int mode) -> int {
        if (dtype == LS_F16)
            hipLaunchKernelGGL(sample_hist_kernel<ElemF16>, grid, block, 0, s, static_cast<const _Float16*>(logits), (long)ld, vocab,
                               level, mode, temperature, state, hist, cmax);
        else
            hipLaunchKernelGGL(sample_hist_kernel<ElemBF16>, grid, block, 0, s, static_cast<const __bf16*>(logits), (long)ld, vocab,
                               level, mode, temperature, state, hist, cmax);
        LS_CHECK_LAUNCH("sample_hist_kernel");
        hipLaunchKernelGGL(sample_select_kernel, dim3(rows), block, 0, s, level, mode, use_k ? top_k : vocab, top_p, nchunks, state,
                           hist, cmax);
        LS_CHECK_LAUNCH("sample_select_kernel");
        return LS_OK;
    };
    int rc;
    const int filtered = (use_k || use_p || use_m || use_t || use_s || use_x) ? 1 : 0;
    const unsigned seed_lo = (unsigned)d.seed, seed_hi = (unsigned)(d.seed >> 32);
    if (filtered) {
        if ((rc = hist_pass(0, 0))) return rc;           // also the row maximum, lower = 0 and upper = 0xffff
        if (use_k && (rc = hist_pass(1, 0))) return rc;
        // (the partial records of the cuts live in `hist`: no pass of this function has it in use across them)
        if (use_s && (rc = ls_sample_sigma_launch(logits, rows, vocab, (long)ld, dtype, cut->top_n_sigma, state, hist, s))) return rc;
        if (use_p) {
            if ((rc = hist_pass(0, 1))) return rc;
            if ((rc = hist_pass(1, 1))) return rc;
        }
        if (use_m && (rc = ls_sample_minp_launch(rows, dtype, temperature, d.min_p, state, s))) return rc;
        if (use_t && (rc = ls_sample_band_launch(logits, rows, vocab, (long)ld, dtype, temperature, d.typical_p, state,
                                                 base + w.total, s)))
            return rc;
        if (use_x && (rc = ls_sample_xtc_launch(logits, rows, vocab, (long)ld, dtype, temperature, cut->xtc_probability,
                                                cut->xtc_threshold, d.positions, d.streams, seed_lo, seed_hi, state, hist, s)))
            return rc;
    }
    if (dtype == LS_F16)
        hipLaunchKernelGGL(sample_key_kernel<ElemF16>, grid, block, 0, s, static_cast<const _Float16*>(logits), (long)ld, vocab,
                           d.positions, d.streams, seed_lo, seed_hi, temperature, filtered, state, cand);
    else
        hipLaunchKernelGGL(sample_key_kernel<ElemBF16>, grid, block, 0, s, static_cast<const __bf16*>(logits), (long)ld, vocab,
                           d.positions, d.streams, seed_lo, seed_hi, temperature, filtered, state, cand);
    LS_CHECK_LAUNCH("sample_key_kernel");
    hipLaunchKernelGGL(sample_merge_kernel, dim3((rows + SM_THREADS - 1) / SM_THREADS), block, 0, s, cand, rows, nchunks, d.out_idx,
                       d.out_top2_idx, d.out_top2_key, d.out_kept, d.out_threshold, d.out_upper);
    LS_CHECK_LAUNCH("sample_merge_kernel");
    return LS_OK;
}

}  // namespace

extern "C" {

size_t ls_sample_workspace_bytes(int rows, int vocab) {
    if (rows < 1 || vocab < 8) return 0;
    return sample_ws(rows, vocab).total;
}

size_t ls_sample_ex_workspace_bytes(const ls_sample_desc* d) {
    if (!d || d->rows < 1 || d->vocab < 8) return 0;
    return sample_ws(d->rows, d->vocab).total + (d->typical_p < 1.f ? ls_sample_band_bytes(d->rows) : 0);
}

int ls_sample_rows(const void* logits, int rows, int vocab, int64_t ld, int dtype, const int64_t* positions, const int32_t* streams,
                   uint64_t seed, float temperature, int top_k, float top_p, int64_t* out_idx, int64_t* out_top2_idx,
                   float* out_top2_key, int32_t* out_kept, float* out_threshold, void* workspace, size_t workspace_bytes,
                   void* stream) {
    ls_sample_desc d = {};
    d.logits = logits; d.positions = positions; d.streams = streams;
    d.out_idx = out_idx; d.out_top2_idx = out_top2_idx; d.out_top2_key = out_top2_key;
    d.out_kept = out_kept; d.out_threshold = out_threshold; d.out_upper = nullptr;
    d.ld = ld; d.seed = seed;
    d.rows = rows; d.vocab = vocab; d.dtype = dtype; d.top_k = top_k;
    d.temperature = temperature; d.top_p = top_p; d.min_p = 0.f; d.typical_p = 1.f;
    return sample_run(d, nullptr, workspace, workspace_bytes, stream, "ls_sample_rows");
}

int ls_sample_rows_ex(const ls_sample_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    if (!d) LS_FAIL(LS_ERR_INVALID_ARG, "ls_sample_rows_ex: null descriptor");
    return sample_run(*d, nullptr, workspace, workspace_bytes, stream, "ls_sample_rows_ex");
}

size_t ls_sample_cut_workspace_bytes(const ls_sample_desc* d, const ls_sample_cut* cut) {
    (void)cut;                                           // the cuts keep their partial records in the histogram area
    return ls_sample_ex_workspace_bytes(d);
}

int ls_sample_rows_cut(const ls_sample_desc* d, const ls_sample_cut* cut, void* workspace, size_t workspace_bytes, void* stream) {
    if (!d) LS_FAIL(LS_ERR_INVALID_ARG, "ls_sample_rows_cut: null descriptor");
    return sample_run(*d, cut, workspace, workspace_bytes, stream, "ls_sample_rows_cut");
}

}  // extern "C"
