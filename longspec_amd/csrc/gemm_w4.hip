// gemm_w4.hip -- the skinny GEMM of gemm.hip with OCP MX FP4 (e2m1 elements, e8m0 block scales) weights: a quarter of the
// bytes of the 16-bit weight stream, plus one scale byte per 32 elements (gfx950 / CDNA4).
//
// W[n, k] = e2m1(q[n, k]) * 2^(e[n, k / 32] - 127): a 4-bit element {+-0, 0.5, 1, 1.5, 2, 3, 4, 6}, two per byte (lower k in
// the low nibble), and one e8m0 byte per 32 consecutive k of a row.  The activations are NOT quantised: a dword of 8 nibbles
// is converted, exactly, to the activation dtype on its way into the MFMA A operand by four
// v_cvt_scalef32_pk_{f16,bf16}_fp4 (byte selects 0..3) whose scale operand is the block's 2^(e - 127), and the multiply is the
// same v_mfma_f32_16x16x32_{f16,bf16} as in gemm.hip.  The converted operand IS the de-quantised weight: there is no row
// scale behind the reductions (W4::SCALED is false).
//
// The kernel is skinny_gemm.h::skinny_gemm_body with the weight-format policy W4 below; this file holds only what is
// MXFP4-specific: the policy, the conversion, the quantiser, the packer and the C entry points.
//
// Exactness.  Launch plan (ls_common.h::GemmPlan), k order of every accumulator, reductions and rounding points are the
// 16-bit launch's because the code is the same.  The block exponent is kept in [-13, 13] (quantiser: clamped; packer: anything
// else is LS_ERR_UNSUPPORTED), so every non-zero element times its scale lies in [2^-14, 6 * 2^13]: a NORMAL fp16 value and a
// bf16 value, which the conversion produces without rounding and whatever it does with fp16 subnormal results.  The MFMA
// therefore sees the operands of the 16-bit launch on the de-quantised weight, and the two launches agree bit for bit.
//
// Layout (ls_linear_w4_pack).  The 64-k chunk c of the 64-row group g is CHUNK_BYTES = 2176 bytes at (g * K/64 + c) * 2176:
//     bytes 512 t + 8 l .. + 3      (tile t = 0..3, lane l = 0..63)  the 8 nibbles of row 16 t + (l & 15),
//                                   k = 64 c + 8 (l >> 4) .. + 7        -- the A operand of k-step 2c
//     bytes 512 t + 8 l + 4 .. + 7  the same row, k = 64 c + 32 + 8 (l >> 4) .. + 7   -- the A operand of k-step 2c + 1
//     bytes 2048 + 8 r + 2 t + ks   (r = 0..15, ks = 0, 1)  the scale byte of row 16 t + r, block 2 c + ks
// One wave-wide non-temporal global_load_dwordx2 per tile plus ONE per 64-row group for the scales (lane l reads the 8 bytes
// of row-in-tile l & 15: its scale for every tile and k-step of the chunk) feed the 2 x 4 MFMAs of a chunk.  Each scale byte
// is stored once; a group streams 2176 bytes per chunk (gemm_w8.hip: 4096, gemm.hip: 8192), 0.5 + 1/32 bytes per element.
// (A 32-byte table behind every tile's 512 bytes would be the same bytes but four 2-byte loads per chunk instead of one
// 8-byte load: 8 instead of 5 entries of the 63-deep load counter per chunk, and 4 registers instead of 2.)
// Gate/up and rope packing permute the 16-row tiles exactly as the other packers do.
//
// Not on this path: the folded RMSNorm (norm_weight / ssq_in / ssq_out) and ls_linear_prefetch -- LS_ERR_UNSUPPORTED.
//
// Serves the same reference seams as gemm.hip (longspec/test): llama.py:361-363,390, LlamaMLP.forward (vendored
// qwen2.py:218-230), llama_glide.py:248-250,268,285-287,305, lm_head at llama_glide.py:960,1019,1046,1091.
#include <math.h>
#include <stdlib.h>

#include <mutex>

#include "skinny_gemm.h"

namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int W4_EXP_MIN = 127 - 13, W4_EXP_MAX = 127 + 13;      // the e8m0 bytes this path takes

// 8 e2m1 nibbles (one dword, k ascending from the low nibble) times `scale` -> the 8 elements of an MFMA A operand
template <typename E>
__device__ __forceinline__ typename E::V8 cvt8_fp4(unsigned q, float scale);
template <>
__device__ __forceinline__ f16x8 cvt8_fp4<ElemF16>(unsigned q, float scale) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(q, scale, 0);
    const h2 b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(q, scale, 1);
    const h2 c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(q, scale, 2);
    const h2 d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(q, scale, 3);
    return f16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
template <>
__device__ __forceinline__ bf16x8 cvt8_fp4<ElemBF16>(unsigned q, float scale) {
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    const b2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 0);
    const b2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 1);
    const b2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 2);
    const b2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 3);
    return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// The MXFP4 weight format of skinny_gemm_body: per chunk and tile one dwordx2 per lane (k-step 0, k-step 1), per chunk and
// 64-row group one dwordx2 of scale bytes.  A set is 2176 bytes per group, about half of W8's.  The look-ahead is W8's in
// CHUNKS (8 / 6 / 3 against 8 / 6 / 2), i.e. about half its bytes in flight per wave, not the same bytes: MEASURED
// (profiles/w4_lac_ab.txt, two box visits, the tool of the per-launch table) against 11 / 10 / 4 and against 16 / 12 / 5 (equal bytes; 80 loads in flight,
// beyond the 63 the wave's load counter tells apart), the short look-ahead is the fastest -- lm_head at M <= 16: 57-61 us
// against 64-66 us for both longer ones, gate|up 19.3-19.4 against 20.3 / 20.8 us, the rest within 1.2 us and never behind.  At 156 registers the
// M <= 16 variant runs 3 waves per SIMD instead of 2, which hides more latency than the registers spent on deeper sets did.
struct W4 {
    using Args = GemmK;
    static constexpr bool SCALED = false;
    static constexpr bool FOLDED_NORM = false;
    static constexpr int CHUNK_BYTES = 2176;
    static constexpr int TILE_BYTES = 512, LANE_BYTES = 8;
    static constexpr int SCALE_OFF = 2048;
    static constexpr int lac(int MT, int NT) { return NT == 8 ? 3 : MT == 1 ? 8 : 6; }
    template <typename E, int NT>
    struct Set {
        u32x2 q[NT];                         // [tile]: .x = the nibbles of k-step 0 of the chunk, .y = k-step 1
        u32x2 s[NT / 4];                     // [group]: scale byte 2 t + ks of the lane's row-in-tile
    };
    template <typename E, int NT>
    static __device__ __forceinline__ void issue(Set<E, NT>& s, const char* const (&wtile)[NT], int ks0) {
        const long off = (long)(ks0 >> 1) * CHUNK_BYTES;
#pragma unroll
        for (int t = 0; t < NT; ++t) s.q[t] = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(wtile[t] + off));
        // wtile[4j] = chunk 0 of the group + lane * 8; the scale row of lane l is row l & 15: 8 * (l & 15) = 8 l - 128 (l >> 4)
        const int back = SCALE_OFF - (int)(threadIdx.x & 48) * 8;
#pragma unroll
        for (int j = 0; j < NT / 4; ++j)
            s.s[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(wtile[4 * j] + off + back));
    }
    template <typename E, int NT>
    static __device__ __forceinline__ typename E::V8 a_operand(const Set<E, NT>& s, int ks, int t) {
        const unsigned b = (s.s[t >> 2][(t & 3) >> 1] >> (((t & 1) * 2 + ks) * 8)) & 0xffu;
        return cvt8_fp4<E>(s.q[t][ks], __uint_as_float(b << 23));
    }
};

template <typename E, int MT, int NT, int EPI>
__global__ __launch_bounds__(GEMM_THREADS, MT >= 5 ? 1 : 2) void skinny_gemm_w4_kernel(const GemmK p) {
    skinny_gemm_body<E, W4, MT, NT, EPI, false>(p);
}

struct SkinnyGemmW4 {            // host: the kernel family launch_skinny_gemm dispatches over
    using W = W4;
    static constexpr const char* NAME = "skinny_gemm_w4_kernel";
    template <typename E, int MT, int NT, int EPI, bool NORM>
    static auto kernel() {
        return skinny_gemm_w4_kernel<E, MT, NT, EPI>;
    }
};

// ---- quantiser ---------------------------------------------------------------------------
// |x| <= 6 -> the e2m1 magnitude code 0..7 (0, 0.5, 1, 1.5, 2, 3, 4, 6), round to nearest, ties to the even mantissa bit,
// saturating at 6.  Written out in integer arithmetic so that it is, bit for bit, what longspec_amd/quant.py computes.
__device__ __forceinline__ unsigned e2m1_rne(float x) {
    const float a = fminf(fabsf(x), 6.0f);                   // (fminf drops a NaN: it saturates too)
    if (a < 1.0f) return (unsigned)rintf(a * 2.0f);          // the subnormal step 0.5; 2 = the smallest normal
    unsigned b = __float_as_uint(a);
    b += 0x1FFFFFu + ((b >> 22) & 1u);                       // RNE at mantissa bit 22
    return (((b >> 23) - 126u) << 1) | ((b >> 22) & 1u);
}

// E = ceil(log2(amax / 6)) by exponent arithmetic, clamped: amax = m 2^ex with m in [0.5, 1), 6 = 0.75 * 2^3
__device__ __forceinline__ int mx_block_exp(float amax) {
    if ((__float_as_uint(amax) & 0x7fffffffu) == 0u) return 0;
    int ex;
    const float m = frexpf(amax, &ex);
    const int e = ex - 3 + (m > 0.75f ? 1 : 0);
    return e < -13 ? -13 : e > 13 ? 13 : e;
}

// 4 lanes per 32-k block, 8 elements each: amax over the block, the exponent byte, then one dword of nibbles per lane.
// K % 32 == 0; `nunits` = N * K / 8.
template <typename E>
__global__ __launch_bounds__(256) void quantize_blocks_kernel(const char* __restrict__ w, uint8_t* __restrict__ q,
                                                              uint8_t* __restrict__ eb, long nunits) {
    using V8 = typename E::V8;
    // (nunits % 4 == 0 and the stride is a multiple of 4: the 4 lanes of a block enter and leave the loop together)
    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < nunits; u += (long)gridDim.x * 256) {
        const V8 v = *reinterpret_cast<const V8*>(w + u * 16);
        float f[8];
        float amax = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            f[i] = E::to_f32(v[i]);
            amax = fmaxf(amax, fabsf(f[i]));
        }
        amax = fmaxf(amax, __shfl_xor(amax, 1));
        amax = fmaxf(amax, __shfl_xor(amax, 2));
        const int ex = mx_block_exp(amax);
        const float inv = __uint_as_float((unsigned)(127 - ex) << 23);        // 2^-E: the division is exact
        unsigned d = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) d |= (((__float_as_uint(f[i]) >> 28) & 8u) | e2m1_rne(f[i] * inv)) << (4 * i);
        *reinterpret_cast<unsigned*>(q + u * 4) = d;
        if ((u & 3) == 0) eb[u >> 2] = (uint8_t)(ex + 127);
    }
}

// ---- packing: q [N, K/2] nibble bytes, e [N, K/32] -> the streamed layout (header comment); rows >= N are zero with scale
// 2^0.  The tile permutations (`q_up`, `rope`) are the other packers': skinny_gemm.h::packed_tile_source.  `bad` is set when
// a scale byte of a real row lies outside [W4_EXP_MIN, W4_EXP_MAX].
__global__ __launch_bounds__(256) void pack_w4_kernel(const uint8_t* __restrict__ q, const uint8_t* __restrict__ q_up,
                                                      const uint8_t* __restrict__ e, const uint8_t* __restrict__ e_up,
                                                      uint8_t* __restrict__ out, int N, int K, long nblocks, int rope,
                                                      unsigned* __restrict__ bad) {
    const int nch = K >> 6;
    for (long blk = (long)blockIdx.x * 4 + (threadIdx.x >> 6); blk < nblocks; blk += (long)gridDim.x * 4) {
        const int t = (int)(blk & 3);
        const long gc = blk >> 2;
        const int g = (int)(gc / nch), c = (int)(gc % nch);
        const int l = threadIdx.x & 63;
        int row;
        const uint8_t* src = packed_tile_source(g * 4 + t, l, q, q_up, rope, row);
        const uint8_t* esrc = packed_tile_source(g * 4 + t, l, e, e_up, rope, row);
        uint8_t* chunk = out + gc * W4::CHUNK_BYTES;
        unsigned a = 0u, b = 0u;
        if (row < N) {
            const uint8_t* s = src + (long)row * (K >> 1) + c * 32 + (l >> 4) * 4;
            a = *reinterpret_cast<const unsigned*>(s);
            b = *reinterpret_cast<const unsigned*>(s + 16);
        }
        *reinterpret_cast<uint2*>(chunk + t * W4::TILE_BYTES + l * W4::LANE_BYTES) = make_uint2(a, b);
        if (l < 16) {
            unsigned s0 = 127u, s1 = 127u;
            if (row < N) {
                s0 = esrc[(long)row * (K >> 5) + c * 2];
                s1 = esrc[(long)row * (K >> 5) + c * 2 + 1];
                if (s0 < (unsigned)W4_EXP_MIN || s0 > (unsigned)W4_EXP_MAX || s1 < (unsigned)W4_EXP_MIN || s1 > (unsigned)W4_EXP_MAX)
                    *bad = 1u;
            }
            *reinterpret_cast<unsigned short*>(chunk + W4::SCALE_OFF + l * 8 + t * 2) = (unsigned short)(s0 | (s1 << 8));
        }
    }
}

// ---- host side ---------------------------------------------------------------------------
int make_plan_w4(const ls_linear_desc* d, GemmPlan& pl) {
    if (d && (d->norm_weight || d->ssq_in || d->ssq_out))
        LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear_w4: the folded RMSNorm (norm_weight / ssq_in / ssq_out) is not available with 4-bit weights");
    if (d && (d->K < 128 || d->K % 64 != 0))
        LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear_w4: K=%d must be a multiple of 64, at least 128", d->K);
    return gemm_make_plan(d, pl);
}

}  // namespace

extern "C" {

size_t ls_linear_w4_packed_bytes(int N, int K) {
    if (N < 1 || K < 64 || K % 64 != 0) return 0;
    return (size_t)((N + 63) / 64) * (size_t)(K / 64) * W4::CHUNK_BYTES;
}

int ls_linear_w4_quantize(const void* weight, int N, int K, int dtype, uint8_t* q, uint8_t* e, void* stream) {
    if (!weight || !q || !e) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear_w4_quantize: null pointer");
    if (dtype != LS_F16 && dtype != LS_BF16) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear_w4_quantize: dtype");
    if (N < 1 || K < 32 || K % 32 != 0) LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear_w4_quantize: K=%d must be a multiple of 32", K);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long nunits = (long)N * K / 8;
    long grid = (nunits + 255) / 256;
    if (grid > 65536) grid = 65536;
    if (dtype == LS_F16)
        hipLaunchKernelGGL(quantize_blocks_kernel<ElemF16>, dim3((unsigned)grid), dim3(256), 0, s, static_cast<const char*>(weight), q, e,
                           nunits);
    else
        hipLaunchKernelGGL(quantize_blocks_kernel<ElemBF16>, dim3((unsigned)grid), dim3(256), 0, s, static_cast<const char*>(weight), q, e,
                           nunits);
    LS_CHECK_LAUNCH("quantize_blocks_kernel");
    return LS_OK;
}

int ls_linear_w4_pack(const uint8_t* q, const uint8_t* e, const uint8_t* q_up, const uint8_t* e_up, void* packed, int N, int K,
                      int rope, void* stream) {
    if (!q || !e || !packed) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear_w4_pack: null pointer");
    if ((q_up == nullptr) != (e_up == nullptr)) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear_w4_pack: q_up and e_up go together");
    if (N < 1 || K < 64 || K % 64 != 0) LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear_w4_pack: K=%d must be a multiple of 64", K);
    if (q_up && rope) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear_w4_pack: a gate/up pair has no rope layout");
    if (q_up && N % 16 != 0) LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear_w4_pack: gate/up needs N %% 16 == 0");
    if (rope && N % 128 != 0) LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear_w4_pack: rope layout needs N = heads x 128 rows");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rows = q_up ? 2 * N : N;
    const long nblocks = (long)((rows + 63) / 64) * 4 * (K / 64);
    long grid = (nblocks + 3) / 4;
    if (grid > 65535 * 4) grid = 65535 * 4;
    // The exponent check needs one word back from the device: packing is a set-up call, it waits for its own kernel.  The
    // word lives in one allocation per device, made at the first call and kept (no allocation or free per call); calls are
    // serialised around it.  A capturing stream cannot be waited for: refused.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear_w4_pack: the stream is capturing; pack before the capture");
    static std::mutex mu;
    static unsigned* flags[64] = {};
    std::lock_guard<std::mutex> lock(mu);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) LS_FAIL(LS_ERR_LAUNCH, "ls_linear_w4_pack: hipGetDevice");
    if (!flags[dev] && hipMalloc(reinterpret_cast<void**>(&flags[dev]), sizeof(unsigned)) != hipSuccess) {
        flags[dev] = nullptr;
        LS_FAIL(LS_ERR_LAUNCH, "ls_linear_w4_pack: hipMalloc");
    }
    unsigned* bad = flags[dev];
    unsigned host_bad = 0;
    hipError_t err = hipMemsetAsync(bad, 0, sizeof(unsigned), s);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(pack_w4_kernel, dim3((unsigned)grid), dim3(256), 0, s, q, q_up, e, e_up, static_cast<uint8_t*>(packed), N, K,
                           nblocks, rope, bad);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipMemcpyAsync(&host_bad, bad, sizeof(unsigned), hipMemcpyDeviceToHost, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) LS_FAIL(LS_ERR_LAUNCH, "pack_w4_kernel: %s", hipGetErrorString(err));
    if (host_bad)
        LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear_w4_pack: a block exponent byte lies outside [%d, %d] (2^-13 .. 2^13), the range this path converts exactly",
                W4_EXP_MIN, W4_EXP_MAX);
    return LS_OK;
}

size_t ls_linear_w4_workspace_bytes(const ls_linear_desc* d) {
    GemmPlan pl;
    if (make_plan_w4(d, pl) != LS_OK) return 0;
    return pl.counter_bytes + pl.part_bytes;
}

int ls_linear_w4_fwd(const ls_linear_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    GemmPlan pl;
    int rc = make_plan_w4(d, pl);
    if (rc != LS_OK) return rc;
    if (!workspace || workspace_bytes < pl.counter_bytes + pl.part_bytes)
        LS_FAIL(LS_ERR_WORKSPACE, "ls_linear_w4_fwd: workspace %zu < %zu bytes", workspace_bytes, pl.counter_bytes + pl.part_bytes);
    GemmK k{};
    fill_gemm_args(k, d, pl, workspace);
    return launch_skinny_gemm<SkinnyGemmW4>(d, k, pl, static_cast<hipStream_t>(stream));
}

}  // extern "C"
