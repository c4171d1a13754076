// gemm_w8.hip -- the skinny GEMM of gemm.hip with OCP e4m3fn (FP8) weights: half the bytes of the weight stream (gfx950 / CDNA4).
//
// Everything a decode pass spends in the projections is the read of W, so W is stored as one byte per element plus one
// fp32 scale per output row, W[n, k] = q[n, k] * s[n].  The activations are NOT quantised: a byte is converted, exactly, to the
// activation dtype on its way into the MFMA A operand (v_cvt_scalef32_pk_{f16,bf16}_fp8 with scale 1.0) and the multiply is
// the same v_mfma_f32_16x16x32_{f16,bf16} as in gemm.hip.  The row scale is applied to the fp32 sum AFTER the 4-wave and
// split-K reductions and BEFORE bias, rounding, SiLU, RoPE or the residual add:  y = round(acc * s[n] (+ bias[n])).
//
// The kernel is the body of the 16-bit one (skinny_gemm.h::skinny_gemm_body) with the weight-format policy W8 below; this file
// holds only what is FP8-specific: the policy, the conversion, the quantiser, the packer and the C entry points.
//
// Exactness.  Launch plan (ls_common.h::GemmPlan), k order of every accumulator, reductions and rounding points are the
// 16-bit launch's because the code is the same.  With s[n] a power of two,
// q * s[n] is a value of the activation dtype, every product and every fp32 partial sum of the 16-bit launch on the
// de-quantised weight is 2^e times the one computed here, and the final multiply is exact: the two launches agree bit for
// bit.  (A general fp32 scale costs one more fp32 rounding.)
//
// Layout (ls_linear_w8_pack).  The 1 KB block of (16-row tile, 64-k chunk c) holds lane l's 16 bytes at byte 16 l:
//     bytes 0..7   q[row0 + (l & 15)][64 c      + 8 (l >> 4) ...]      the A operand of k-step 2c
//     bytes 8..15  q[row0 + (l & 15)][64 c + 32 + 8 (l >> 4) ...]      the A operand of k-step 2c + 1
// and the 4 tiles of a 64-row group are adjacent: block (group g, chunk c, tile t) sits at ((g * K/64 + c) * 4 + t) * 1024.
// One wave-wide non-temporal global_load_dwordx4 per tile feeds the two MFMAs of a chunk; a group streams 4 KB per chunk
// (gemm.hip: 8 KB).  Gate/up and rope packing permute the 16-row tiles exactly as the 16-bit packers do.
//
// Not on this path (no model file uses them with 8-bit weights): the folded RMSNorm (norm_weight / ssq_in / ssq_out) and
// ls_linear_prefetch -- LS_ERR_UNSUPPORTED.
//
// Serves the same reference seams as gemm.hip (longspec/test): llama.py:361-363,390, LlamaMLP.forward (vendored
// qwen2.py:218-230), llama_glide.py:248-250,268,285-287,305, lm_head at llama_glide.py:960,1019,1046,1091.
#include <math.h>
#include <stdlib.h>

#include "skinny_gemm.h"

namespace {

struct GemmK8 : GemmK {          // (the norm / ssq / prefetch fields of GemmK travel along unused: W8::FOLDED_NORM is false)
    const float* scale[3];       // fp32 [n_i] row scales (SILU: scale[0] = gate rows, scale[1] = up rows)
};

// 8 e4m3 bytes (two dwords, k ascending) -> the 8 elements of an MFMA A operand.  Exact: every e4m3 value is an f16 and a
// bf16 value; the scale operand is 1.0.
template <typename E>
__device__ __forceinline__ typename E::V8 cvt8(unsigned lo, unsigned hi);
template <>
__device__ __forceinline__ f16x8 cvt8<ElemF16>(unsigned lo, unsigned hi) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, false);
    const h2 b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, true);
    const h2 c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, false);
    const h2 d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, true);
    return f16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
template <>
__device__ __forceinline__ bf16x8 cvt8<ElemBF16>(unsigned lo, unsigned hi) {
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    const b2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false);
    const b2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
    const b2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false);
    const b2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
    return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// The e4m3 weight format of skinny_gemm_body: a chunk is 4 tiles of 1 KB, one dwordx4 per lane and tile -- half the bytes of
// the 16-bit chunk.  The look-ahead is twice as many chunks, i.e. the same bytes in flight per wave.
struct W8 {
    using Args = GemmK8;
    static constexpr bool SCALED = true;
    static constexpr bool FOLDED_NORM = false;
    static constexpr int CHUNK_BYTES = 4096;
    static constexpr int TILE_BYTES = 1024, LANE_BYTES = 16;
    static constexpr int lac(int MT, int NT) { return NT == 8 ? 2 : MT == 1 ? 8 : 6; }
    template <typename E, int NT>
    struct Set {
        u32x4 q[NT];                         // [tile]: .xy = k-step 0 of the chunk, .zw = k-step 1
    };
    template <typename E, int NT>
    static __device__ __forceinline__ void issue(Set<E, NT>& s, const char* const (&wtile)[NT], int ks0) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
            s.q[t] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wtile[t] + (long)(ks0 >> 1) * CHUNK_BYTES));
    }
    template <typename E, int NT>
    static __device__ __forceinline__ typename E::V8 a_operand(const Set<E, NT>& s, int ks, int t) {
        return cvt8<E>(s.q[t][2 * ks], s.q[t][2 * ks + 1]);
    }
    // (`n` % 4 == 0 and the arrays are 16-byte aligned: ls_linear_w8_fwd)
    static __device__ __forceinline__ f32x4 scale4(const Args& p, int i, int n, bool valid) {
        return valid ? *reinterpret_cast<const f32x4*>(p.scale[i] + n) : f32x4{1.f, 1.f, 1.f, 1.f};
    }
};

template <typename E, int MT, int NT, int EPI>
__global__ __launch_bounds__(GEMM_THREADS, MT >= 5 ? 1 : 2) void skinny_gemm_w8_kernel(const GemmK8 p) {
    skinny_gemm_body<E, W8, MT, NT, EPI, false>(p);
}

struct SkinnyGemmW8 {            // host: the kernel family launch_skinny_gemm dispatches over
    using W = W8;
    static constexpr const char* NAME = "skinny_gemm_w8_kernel";
    template <typename E, int MT, int NT, int EPI, bool NORM>
    static auto kernel() {
        return skinny_gemm_w8_kernel<E, MT, NT, EPI>;
    }
};

// ---- quantiser ---------------------------------------------------------------------------
// fp32 -> OCP e4m3fn, round to nearest even, saturating at +-448 (never the NaN encoding 0x7f / 0xff).  Written out in
// integer arithmetic so that it is, bit for bit, what longspec_amd/quant.py computes with torch's cast on the host.
__device__ __forceinline__ unsigned e4m3_rne(float x) {
    const unsigned sign = (__float_as_uint(x) >> 24) & 0x80u;
    const float a = fminf(fabsf(x), 448.0f);                 // (fminf drops a NaN: it saturates too)
    if (a < 0.015625f) return sign | (unsigned)rintf(a * 512.0f);          // subnormals, step 2^-9; 8 = the smallest normal
    unsigned b = __float_as_uint(a);
    b += 0x7FFFFu + ((b >> 20) & 1u);                        // RNE at mantissa bit 20
    return sign | (((b >> 23) - 120u) << 3) | ((b >> 20) & 7u);
}

// s = 2^ceil(log2(amax / 448)) by exponent arithmetic: amax = m 2^ex with m in [0.5, 1), 448 = 0.875 * 2^9
__device__ __forceinline__ float pow2_scale(float amax) {
    int ex;
    const float m = frexpf(amax, &ex);
    int e = ex - 9 + (m > 0.875f ? 1 : 0);
    e = e < -120 ? -120 : e;                                 // q * s stays a (sub)normal bf16 / a normal fp32
    return __uint_as_float((unsigned)(e + 127) << 23);
}

// one workgroup per row: amax, the scale, then the bytes.  K % 8 == 0.
template <typename E>
__global__ __launch_bounds__(256) void quantize_rows_kernel(const char* __restrict__ w, uint8_t* __restrict__ q,
                                                            float* __restrict__ scale, int K, int pow2) {
    using V8 = typename E::V8;
    __shared__ float red[4];
    const long row = blockIdx.x;
    const char* src = w + row * K * 2;
    float amax = 0.f;
    for (int k = threadIdx.x * 8; k < K; k += 256 * 8) {
        const V8 v = *reinterpret_cast<const V8*>(src + (long)k * 2);
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(E::to_f32(v[e])));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float s = amax == 0.f ? 1.0f : pow2 ? pow2_scale(amax) : amax / 448.0f;
    if (threadIdx.x == 0) scale[row] = s;
    for (int k = threadIdx.x * 8; k < K; k += 256 * 8) {
        const V8 v = *reinterpret_cast<const V8*>(src + (long)k * 2);
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            lo |= e4m3_rne(E::to_f32(v[e]) / s) << (8 * e);
            hi |= e4m3_rne(E::to_f32(v[4 + e]) / s) << (8 * e);
        }
        *reinterpret_cast<uint2*>(q + row * K + k) = make_uint2(lo, hi);
    }
}

// ---- packing: q [N, K] bytes -> the streamed layout (header comment); rows >= N are zero.  The tile permutations (`q_up`,
// `rope`) are the 16-bit packers': skinny_gemm.h::packed_tile_source.
__global__ __launch_bounds__(256) void pack_w8_kernel(const uint8_t* __restrict__ q, const uint8_t* __restrict__ q_up,
                                                      uint8_t* __restrict__ out, int N, int K, long nblocks, int rope) {
    const int nch = K >> 6;
    for (long blk = (long)blockIdx.x * 4 + (threadIdx.x >> 6); blk < nblocks; blk += (long)gridDim.x * 4) {
        const int t = (int)(blk & 3);
        const long gc = blk >> 2;
        const int g = (int)(gc / nch), c = (int)(gc % nch);
        const int l = threadIdx.x & 63;
        int row;
        const uint8_t* src = packed_tile_source(g * 4 + t, l, q, q_up, rope, row);
        uint2 a = make_uint2(0u, 0u), b = make_uint2(0u, 0u);
        if (row < N) {
            const uint8_t* s = src + (long)row * K + c * 64 + (l >> 4) * 8;
            a = *reinterpret_cast<const uint2*>(s);
            b = *reinterpret_cast<const uint2*>(s + 32);
        }
        *reinterpret_cast<uint4*>(out + blk * 1024 + l * 16) = make_uint4(a.x, a.y, b.x, b.y);
    }
}

// ---- host side ---------------------------------------------------------------------------
int make_plan_w8(const ls_linear_desc* d, GemmPlan& pl) {
    if (d && (d->norm_weight || d->ssq_in || d->ssq_out))
        LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear_w8: the folded RMSNorm (norm_weight / ssq_in / ssq_out) is not available with 8-bit weights");
    return gemm_make_plan(d, pl);
}

}  // namespace

extern "C" {

size_t ls_linear_w8_packed_bytes(int N, int K) {
    if (N < 1 || K < 64 || K % 64 != 0) return 0;
    return (size_t)((N + 63) / 64) * (64 * (size_t)K);
}

int ls_linear_w8_quantize(const void* weight, int N, int K, int dtype, int pow2_scale_flag, uint8_t* q, float* scale, void* stream) {
    if (!weight || !q || !scale) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear_w8_quantize: null pointer");
    if (dtype != LS_F16 && dtype != LS_BF16) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear_w8_quantize: dtype");
    if (N < 1 || K < 8 || K % 8 != 0) LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear_w8_quantize: K=%d must be a multiple of 8", K);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == LS_F16)
        hipLaunchKernelGGL(quantize_rows_kernel<ElemF16>, dim3((unsigned)N), dim3(256), 0, s, static_cast<const char*>(weight), q,
                           scale, K, pow2_scale_flag);
    else
        hipLaunchKernelGGL(quantize_rows_kernel<ElemBF16>, dim3((unsigned)N), dim3(256), 0, s, static_cast<const char*>(weight), q,
                           scale, K, pow2_scale_flag);
    LS_CHECK_LAUNCH("quantize_rows_kernel");
    return LS_OK;
}

int ls_linear_w8_pack(const uint8_t* q, const uint8_t* q_up, void* packed, int N, int K, int rope, void* stream) {
    if (!q || !packed) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear_w8_pack: null pointer");
    if (N < 1 || K < 64 || K % 64 != 0) LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear_w8_pack: K=%d must be a multiple of 64", K);
    if (q_up && rope) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear_w8_pack: a gate/up pair has no rope layout");
    if (q_up && N % 16 != 0) LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear_w8_pack: gate/up needs N %% 16 == 0");
    if (rope && N % 128 != 0) LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear_w8_pack: rope layout needs N = heads x 128 rows");
    const int rows = q_up ? 2 * N : N;
    const long nblocks = (long)((rows + 63) / 64) * 4 * (K / 64);
    long grid = (nblocks + 3) / 4;
    if (grid > 65535 * 4) grid = 65535 * 4;
    hipLaunchKernelGGL(pack_w8_kernel, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), q, q_up,
                       static_cast<uint8_t*>(packed), N, K, nblocks, rope);
    LS_CHECK_LAUNCH("pack_w8_kernel");
    return LS_OK;
}

size_t ls_linear_w8_workspace_bytes(const ls_linear_desc* d) {
    GemmPlan pl;
    if (make_plan_w8(d, pl) != LS_OK) return 0;
    return pl.counter_bytes + pl.part_bytes;
}

int ls_linear_w8_fwd(const ls_linear_desc* d, const float* const scale[3], void* workspace, size_t workspace_bytes, void* stream) {
    GemmPlan pl;
    int rc = make_plan_w8(d, pl);
    if (rc != LS_OK) return rc;
    if (!scale) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear_w8_fwd: null scale array");
    const int n_scale = d->epilogue == LS_EPI_SILU_MUL ? 2 : d->n_seg;
    for (int i = 0; i < n_scale; ++i)
        if (!scale[i] || (reinterpret_cast<uintptr_t>(scale[i]) & 15) != 0)
            LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear_w8_fwd: scale[%d] must be a 16-byte aligned fp32 array", i);
    if (!workspace || workspace_bytes < pl.counter_bytes + pl.part_bytes)
        LS_FAIL(LS_ERR_WORKSPACE, "ls_linear_w8_fwd: workspace %zu < %zu bytes", workspace_bytes, pl.counter_bytes + pl.part_bytes);
    GemmK8 k{};
    fill_gemm_args(k, d, pl, workspace);
    for (int i = 0; i < n_scale; ++i) k.scale[i] = scale[i];
    return launch_skinny_gemm<SkinnyGemmW8>(d, k, pl, static_cast<hipStream_t>(stream));
}

}  // extern "C"
