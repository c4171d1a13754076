// gemm_w8.hip -- the skinny GEMM of gemm.hip with OCP e4m3fn (FP8) weights: half the bytes of the weight stream (gfx950 / CDNA4).
//
// Everything a decode pass spends in the projections is the read of W, so W is stored as one byte per element plus one
// fp32 scale per output row, W[n, k] = q[n, k] * s[n].  The activations are NOT quantised: a byte is converted, exactly, to the
// activation dtype on its way into the MFMA A operand (v_cvt_scalef32_pk_{f16,bf16}_fp8 with scale 1.0) and the multiply is
// the same v_mfma_f32_16x16x32_{f16,bf16} as in gemm.hip.  The row scale is applied to the fp32 sum AFTER the 4-wave and
// split-K reductions and BEFORE bias, rounding, SiLU, RoPE or the residual add:  y = round(acc * s[n] (+ bias[n])).
//
// Exactness.  The launch plan (slab height, split-K factor: ls_common.h::GemmPlan) is the 16-bit kernel's, a wave owns the
// same quarter of the same k range, and every accumulator sees its k-steps in the same order.  With s[n] a power of two,
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

#include "ls_common.h"

namespace {

constexpr int GEMM_THREADS = 256;

struct GemmK8 {
    const char* x;
    long ldx;                    // elements
    const char* w[3];            // packed e4m3 segments (SILU: w[0] = the gate/up pair)
    const char* bias[3];         // or null
    const float* scale[3];       // fp32 [n_i] row scales (SILU: scale[0] = gate rows, scale[1] = up rows)
    int n[3];
    char* y;
    long ldy;
    float* part;                 // split-K partials
    unsigned* counters;          // one per slab, zero between launches
    int M, K, N;
    int nch, S, nslabs;          // nch = K / 64 chunks
    int flag_off;                // byte offset of the last-arriver flag in dynamic LDS
    const char* rope_cos;
    const char* rope_sin;
    int rope_segs;
    const char* residual;
    long ldr;
};

enum { EPI_NONE = 0, EPI_SILU_MUL = 1, EPI_QKV_ROPE = 2 };

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t part_rsrc(const float* base, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, bytes, 0x00020000);
}
// agent-coherent (sc1, aux 16) 16-byte accesses of the split-K partials, as in gemm.hip
__device__ __forceinline__ void st_coherent4(__amdgpu_buffer_rsrc_t r, unsigned byte_off, f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, byte_off, 0, 16);
}
__device__ __forceinline__ f32x4 ld_coherent4(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 16));
}

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

// 4 row scales of output columns n .. n+3 (`sc` is indexable by that column; n % 4 == 0, the array is 16-byte aligned)
__device__ __forceinline__ f32x4 load_scale4(const float* sc, int n, bool valid) {
    return valid ? *reinterpret_cast<const f32x4*>(sc + n) : f32x4{1.f, 1.f, 1.f, 1.f};
}

// MT = 16-row tiles of x (M <= 16*MT); NT = 16-row weight tiles per workgroup (4: one packed group, 8: two)
template <typename E, int MT, int NT, int EPI>
__global__ __launch_bounds__(GEMM_THREADS, MT >= 5 ? 1 : 2) void skinny_gemm_w8_kernel(const GemmK8 p) {
    using V8 = typename E::V8;
    using V4 = typename E::V4;
    // A W register set holds one 64-k chunk of the workgroup's NT tiles: NT dwordx4 per lane, half of gemm.hip's.  The
    // look-ahead is twice as many chunks, i.e. the same bytes in flight per wave.
    constexpr int LAC = NT == 8 ? 2 : MT == 1 ? 8 : 6;      // chunks of look-ahead
    constexpr int NCS = LAC + 1;             // W register sets, one per chunk in flight
    constexpr int XL = 2 * MT;               // 1 KB pieces (8 rows x 128 B) of one x chunk
    constexpr int XSLAB = MT * 16 * 128;     // bytes of a wave's x slab
    constexpr int NPASS = NT / 4;            // the 4-wave reduction handles 4 tiles per pass (LDS budget)
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g4 = lane >> 4;
    const int slab = blockIdx.x, split = blockIdx.y;
    const int ch_begin = (int)(((long)p.nch * split) / p.S);
    const int ch_end = (int)(((long)p.nch * (split + 1)) / p.S);

    // ---- the NT weight tiles of this workgroup (tile order of the packed matrix as in gemm.hip: gate/up alternate for
    // EPI_SILU_MUL, rotary pairs neighbour each other in the q and k segments of EPI_QKV_ROPE)
    const char* wtile[NT];
    const char* bias_p = nullptr;
    int n_lim;                   // end of the valid output columns of this slab's segment (global column)
    int n_tile0;                 // global output column of tile 0
    int seg_base = 0, seg = 0;
    const long group_b = (long)p.nch * 4096;
    {
        const int row0 = slab * NT * 16;                 // first packed row of the workgroup (global over segments)
        if (EPI != EPI_SILU_MUL) {
            if (row0 >= p.n[0]) { seg_base = p.n[0]; seg = 1; }
            if (seg == 1 && row0 >= p.n[0] + p.n[1]) { seg_base = p.n[0] + p.n[1]; seg = 2; }
            bias_p = p.bias[seg] ? p.bias[seg] - (long)seg_base * 2 : nullptr;   // indexable by global column
            n_tile0 = row0;
            n_lim = seg_base + p.n[seg];
        } else {
            n_tile0 = row0 >> 1;
            n_lim = p.n[0];
        }
        const int ngroups = EPI != EPI_SILU_MUL ? (p.n[seg] + 63) >> 6 : (2 * p.n[0] + 63) >> 6;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int g = min(((row0 - seg_base) >> 6) + (t >> 2), ngroups - 1);    // clamp: tiles past the end are never stored
            wtile[t] = p.w[seg] + (long)g * group_b + (t & 3) * 1024 + lane * 16;
        }
    }

    f32x4 acc[NT][MT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // wave w takes the w-th contiguous quarter of the workgroup's chunk range
    const int quarter = (ch_end - ch_begin + 3) >> 2;
    const int ch0 = ch_begin + wave * quarter;
    const int nch = max(0, min(ch_end - ch0, quarter));

    u32x4 wa[NCS][NT];           // [set][tile]: .xy = k-step 0 of the chunk, .zw = k-step 1
    V8 xs[XL];                   // x staging: piece i = rows 8i .. 8i+7, lane -> (row 8i + lane/8, 16 B slot lane%8)
    char* xlds = smem + wave * XSLAB;
    const int xr_in = lane >> 3, xslot = lane & 7;

    unsigned xoff[XL];           // 32-bit byte offsets of this lane's 16 B in each piece (x is far below 4 GB)
#pragma unroll
    for (int i = 0; i < XL; ++i) xoff[i] = (unsigned)(((long)min(i * 8 + xr_in, p.M - 1) * p.ldx + xslot * 8) * 2);
    auto load_x = [&](int ch) {
        const char* xc = p.x + (long)ch * 128;            // wave-uniform
#pragma unroll
        for (int i = 0; i < XL; ++i) xs[i] = *reinterpret_cast<const V8*>(xc + xoff[i]);
    };
    auto store_x = [&]() {       // slot ^ ((row >> 1) & 7): 16 rows x one slot hit 16 distinct 16 B bank groups
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const int row = i * 8 + xr_in;
            *reinterpret_cast<V8*>(xlds + row * 128 + ((xslot ^ ((row >> 1) & 7)) << 4)) = xs[i];
        }
    };
    // chunk `un` of this wave: every byte is read once per launch by one workgroup -> non-temporal
    auto issue_w = [&](int un, int set) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
            wa[set][t] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wtile[t] + (long)(ch0 + un) * 4096));
    };
    auto mma_unit = [&](int set) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {                     // k-step inside the 64-k chunk staged in LDS
            V8 bx[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int row = mt * 16 + l15;
                bx[mt] = *reinterpret_cast<const V8*>(xlds + row * 128 + (((ks * 4 + g4) ^ ((row >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const V8 a = cvt8<E>(wa[set][t][2 * ks], wa[set][t][2 * ks + 1]);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[t][mt] = E::mfma(a, bx[mt], acc[t][mt]);
            }
        }
    };

    if (nch > 0) load_x(ch0);
#pragma unroll
    for (int i = 0; i < LAC; ++i)
        if (i < nch) issue_w(i, i);
    int c = 0;
    // steady state: no control flow inside, so the compiler's in-order vmcnt counts stay exact;
    // sched_barrier(0) keeps the loads of the chunks ahead in front of the MFMAs of the current one
    for (; c + NCS - 1 + LAC < nch; c += NCS) {
#pragma unroll
        for (int u = 0; u < NCS; ++u) {
            store_x();                                   // chunk c+u: staging registers -> the wave's LDS slab
            load_x(ch0 + c + u + 1);                     // (the last chunk of the wave is never in this loop: LAC >= 1)
            issue_w(c + u + LAC, (u + LAC) % NCS);
            __builtin_amdgcn_sched_barrier(0);
            mma_unit(u);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int u = 0; u < NCS + LAC - 1; ++u) {            // drain
        if (c + u < nch) {
            store_x();
            if (c + u + 1 < nch) load_x(ch0 + c + u + 1);
            if (c + u + LAC < nch) issue_w(c + u + LAC, (u + LAC) % NCS);
            __builtin_amdgcn_sched_barrier(0);
            mma_unit(u % NCS);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // ---- reduce the 4 waves (fixed order) through LDS, 4 tiles per pass.  EPI_NONE: wave w finishes tile
    // 4h + w of pass h.  EPI_SILU_MUL / EPI_QKV_ROPE: waves 0,1 finish the tile pair 4h + 2w, 4h + 2w + 1
    // (gate, up) / (rotary low half, high half).
    constexpr bool PAIRED = EPI != EPI_NONE;
    constexpr int NT_OUT = PAIRED ? 2 : 1;                   // tiles per finishing wave per pass
    const bool finisher = PAIRED ? wave < 2 : true;
    float* red = reinterpret_cast<float*>(smem);
    f32x4 r[NPASS][NT_OUT][MT];
#pragma unroll
    for (int h = 0; h < NPASS; ++h) {
        __syncthreads();         // x slabs / previous pass no longer read
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                *reinterpret_cast<f32x4*>(red + (((wave * 4 + t) * MT + mt) * 64 + lane) * 4) = acc[h * 4 + t][mt];
        __syncthreads();
        if (finisher) {
#pragma unroll
            for (int q = 0; q < NT_OUT; ++q) {
                const int t = PAIRED ? 2 * wave + q : wave;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    f32x4 v = *reinterpret_cast<const f32x4*>(red + (((0 * 4 + t) * MT + mt) * 64 + lane) * 4);
#pragma unroll
                    for (int w2 = 1; w2 < 4; ++w2)
                        v += *reinterpret_cast<const f32x4*>(red + (((w2 * 4 + t) * MT + mt) * 64 + lane) * 4);
                    r[h][q][mt] = v;
                }
            }
        }
    }

    // ---- split-K: deterministic last-arriver reduction (gemm.hip)
    if (p.S > 1) {
        constexpr int TILE_F = MT * 4 * 64;                  // floats of one tile's accumulators
        auto tile_of = [&](int h, int q) { return h * 4 + (PAIRED ? 2 * wave + q : wave); };
        if (finisher) {
#pragma unroll
            for (int h = 0; h < NPASS; ++h)
#pragma unroll
                for (int q = 0; q < NT_OUT; ++q) {
                    const __amdgpu_buffer_rsrc_t mine =
                        part_rsrc(p.part + (((long)split * p.nslabs + slab) * NT + tile_of(h, q)) * TILE_F, TILE_F * 4);
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) st_coherent4(mine, (mt * 64 + lane) * 16, r[h][q][mt]);
                }
        }
        // every thread drains its OWN write-through partial stores before the barrier; only then may thread 0 bump the
        // slab counter (the asm wait is invisible to the compiler's waitcnt elision, see gemm.hip)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        volatile unsigned& s_last = *reinterpret_cast<volatile unsigned*>(smem + p.flag_off);
        if (tid == 0) {
            const unsigned prev = __hip_atomic_fetch_add(p.counters + slab, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = (prev == (unsigned)p.S - 1u);
            if (prev == (unsigned)p.S - 1u) __hip_atomic_store(p.counters + slab, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (!s_last) return;
        if (finisher) {
#pragma unroll
            for (int h = 0; h < NPASS; ++h)
#pragma unroll
                for (int q = 0; q < NT_OUT; ++q)
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) r[h][q][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int s = 0; s < p.S; ++s) {
#pragma unroll
                for (int h = 0; h < NPASS; ++h)
#pragma unroll
                    for (int q = 0; q < NT_OUT; ++q) {
                        const __amdgpu_buffer_rsrc_t src =
                            part_rsrc(p.part + (((long)s * p.nslabs + slab) * NT + tile_of(h, q)) * TILE_F, TILE_F * 4);
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) r[h][q][mt] += ld_coherent4(src, (mt * 64 + lane) * 16);
                    }
            }
        }
    }
    if (!finisher) return;

    // ---- epilogue: lane holds the fp32 sums of y[m = mt*16 + l15][n .. n+3]; the row scales come first
#pragma unroll
    for (int h = 0; h < NPASS; ++h) {
        if (EPI == EPI_SILU_MUL) {
            const int nn = n_tile0 + (h * 2 + wave) * 16 + g4 * 4;
            const f32x4 sg4 = load_scale4(p.scale[0], nn, nn < n_lim), su4 = load_scale4(p.scale[1], nn, nn < n_lim);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int m = mt * 16 + l15;
                V4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float g = round_to<E>(r[h][0][mt][e] * sg4[e]);     // gate_proj output in the storage dtype
                    const float u = round_to<E>(r[h][1][mt][e] * su4[e]);     // up_proj output
                    const float sg = round_to<E>(g / (1.0f + expf(-g)));      // act_fn (SiLU), fp32 math, rounded
                    o[e] = E::from_f32(sg * u);
                }
                if (m < p.M && nn < n_lim) *reinterpret_cast<V4*>(p.y + ((long)m * p.ldy + nn) * 2) = o;
            }
        } else if (EPI == EPI_QKV_ROPE) {
            // tiles (2u, 2u+1) of the slab, u = 2h + wave.  Rotated segment: they are rows d.. and 64+d.. of one head;
            // apply_rotary_pos_emb on the rounded projections exactly as rope_apply_kernel does (misc.hip).
            const int tl = ((n_tile0 - seg_base) >> 4) + (h * 2 + wave) * 2;          // packed tile index in the segment
            const bool rot = seg < p.rope_segs;
            const int d = ((tl & 7) >> 1) * 16 + g4 * 4;                              // dimension of the low half
            const int n_lo = rot ? seg_base + (tl >> 3) * 128 + d : seg_base + tl * 16 + g4 * 4;
            const int n_hi = rot ? n_lo + 64 : n_lo + 16;
            const float* sc = p.scale[seg] - seg_base;                                // indexable by global column
            const f32x4 sl4 = load_scale4(sc, n_lo, n_lo < n_lim), sh4 = load_scale4(sc, n_hi, n_hi < n_lim);
            float bl[4] = {0.f, 0.f, 0.f, 0.f}, bh[4] = {0.f, 0.f, 0.f, 0.f};
            if (bias_p != nullptr) {
                if (n_lo < n_lim) {
                    const V4 b4 = *reinterpret_cast<const V4*>(bias_p + (long)n_lo * 2);
#pragma unroll
                    for (int e = 0; e < 4; ++e) bl[e] = E::to_f32(b4[e]);
                }
                if (n_hi < n_lim) {
                    const V4 b4 = *reinterpret_cast<const V4*>(bias_p + (long)n_hi * 2);
#pragma unroll
                    for (int e = 0; e < 4; ++e) bh[e] = E::to_f32(b4[e]);
                }
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int m = mt * 16 + l15;
                if (m >= p.M) continue;
                V4 lo, hi;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    lo[e] = E::from_f32(r[h][0][mt][e] * sl4[e] + bl[e]);
                    hi[e] = E::from_f32(r[h][1][mt][e] * sh4[e] + bh[e]);
                }
                if (rot) {
                    const V4 cl = *reinterpret_cast<const V4*>(p.rope_cos + ((long)m * 128 + d) * 2);
                    const V4 ch = *reinterpret_cast<const V4*>(p.rope_cos + ((long)m * 128 + 64 + d) * 2);
                    const V4 sl = *reinterpret_cast<const V4*>(p.rope_sin + ((long)m * 128 + d) * 2);
                    const V4 sh = *reinterpret_cast<const V4*>(p.rope_sin + ((long)m * 128 + 64 + d) * 2);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float xl = E::to_f32(lo[e]), xh = E::to_f32(hi[e]);
                        lo[e] = E::from_f32(round_to<E>(xl * E::to_f32(cl[e])) + round_to<E>(-xh * E::to_f32(sl[e])));
                        hi[e] = E::from_f32(round_to<E>(xh * E::to_f32(ch[e])) + round_to<E>(xl * E::to_f32(sh[e])));
                    }
                }
                if (n_lo < n_lim) *reinterpret_cast<V4*>(p.y + ((long)m * p.ldy + n_lo) * 2) = lo;
                if (n_hi < n_lim) *reinterpret_cast<V4*>(p.y + ((long)m * p.ldy + n_hi) * 2) = hi;
            }
        } else {
            const int nn = n_tile0 + (h * 4 + wave) * 16 + g4 * 4;
            const f32x4 sc4 = load_scale4(p.scale[seg] - seg_base, nn, nn < n_lim);
            float bv[4] = {0.f, 0.f, 0.f, 0.f};
            if (bias_p != nullptr && nn < n_lim) {
                const V4 b4 = *reinterpret_cast<const V4*>(bias_p + (long)nn * 2);
#pragma unroll
                for (int e = 0; e < 4; ++e) bv[e] = E::to_f32(b4[e]);
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int m = mt * 16 + l15;
                V4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = E::from_f32(r[h][0][mt][e] * sc4[e] + bv[e]);
                if (m < p.M && nn < n_lim) {
                    if (p.residual != nullptr) {           // the projection is rounded first, then added (llama_glide.py:466)
                        const V4 r4 = *reinterpret_cast<const V4*>(p.residual + ((long)m * p.ldr + nn) * 2);
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = E::from_f32(E::to_f32(o[e]) + E::to_f32(r4[e]));
                    }
                    *reinterpret_cast<V4*>(p.y + ((long)m * p.ldy + nn) * 2) = o;
                }
            }
        }
    }
}

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

// ---- packing: q [N, K] bytes -> the streamed layout (header comment); rows >= N are zero.  Tile permutations as
// gemm.hip::pack_weight_kernel: `q_up` alternates gate and up tiles, `rope` stores the 8 tiles of a head as 0,4,1,5,2,6,3,7.
__global__ __launch_bounds__(256) void pack_w8_kernel(const uint8_t* __restrict__ q, const uint8_t* __restrict__ q_up,
                                                      uint8_t* __restrict__ out, int N, int K, long nblocks, int rope) {
    const int nch = K >> 6;
    for (long blk = (long)blockIdx.x * 4 + (threadIdx.x >> 6); blk < nblocks; blk += (long)gridDim.x * 4) {
        const int t = (int)(blk & 3);
        const long gc = blk >> 2;
        const int g = (int)(gc / nch), c = (int)(gc % nch);
        const int l = threadIdx.x & 63;
        const int T = g * 4 + t;                           // 16-row tile of the packed matrix
        const uint8_t* src = q;
        int row = T * 16 + (l & 15);
        if (q_up != nullptr) {
            src = (T & 1) ? q_up : q;
            row = (T >> 1) * 16 + (l & 15);
        } else if (rope) {
            row = ((T & ~7) + ((T & 7) >> 1) + 4 * (T & 1)) * 16 + (l & 15);
        }
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
template <typename E, int MT, int NT, int EPI>
int launch(const GemmK8& k, const GemmPlan& pl, hipStream_t s) {
    auto kern = skinny_gemm_w8_kernel<E, MT, NT, EPI>;
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_done = true;
    }
    hipLaunchKernelGGL(kern, dim3(pl.nslabs, pl.S), dim3(GEMM_THREADS), pl.lds, s, k);
    LS_CHECK_LAUNCH("skinny_gemm_w8_kernel");
    return LS_OK;
}

template <typename E, int EPI>
int launch_mt(const GemmK8& k, const GemmPlan& pl, hipStream_t s) {
    switch (pl.MT) {
        case 1: return launch<E, 1, 4, EPI>(k, pl, s);
        case 2: return launch<E, 2, 4, EPI>(k, pl, s);
        default: return pl.NT == 8 ? launch<E, 5, 8, EPI>(k, pl, s) : launch<E, 5, 4, EPI>(k, pl, s);
    }
}

template <typename E, int EPI>
int launch_mt4(const GemmK8& k, const GemmPlan& pl, hipStream_t s) {      // epilogues that only exist with 4-tile slabs
    switch (pl.MT) {
        case 1: return launch<E, 1, 4, EPI>(k, pl, s);
        case 2: return launch<E, 2, 4, EPI>(k, pl, s);
        default: return launch<E, 5, 4, EPI>(k, pl, s);
    }
}

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
    k.x = static_cast<const char*>(d->x);
    k.ldx = d->ldx;
    for (int i = 0; i < 3; ++i) {
        k.w[i] = i < d->n_seg ? static_cast<const char*>(d->w[i]) : nullptr;
        k.bias[i] = i < d->n_seg ? static_cast<const char*>(d->bias[i]) : nullptr;
        k.scale[i] = i < n_scale ? scale[i] : nullptr;
        k.n[i] = i < d->n_seg ? d->n[i] : 0;
    }
    k.y = static_cast<char*>(d->y);
    k.ldy = d->ldy;
    k.counters = static_cast<unsigned*>(workspace);
    k.part = reinterpret_cast<float*>(static_cast<char*>(workspace) + pl.counter_bytes);
    k.M = d->M;
    k.K = d->K;
    k.N = pl.N;
    k.nch = pl.nks / 2;
    k.S = pl.S;
    k.nslabs = pl.nslabs;
    k.flag_off = pl.flag_off;
    k.rope_cos = static_cast<const char*>(d->rope_cos);
    k.rope_sin = static_cast<const char*>(d->rope_sin);
    k.rope_segs = d->n_seg < 2 ? d->n_seg : 2;
    k.residual = static_cast<const char*>(d->residual);
    k.ldr = d->ldr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (d->ev_start) (void)hipEventRecord(static_cast<hipEvent_t>(d->ev_start), s);
    if (d->dtype == LS_F16)
        rc = d->epilogue == LS_EPI_SILU_MUL   ? launch_mt<ElemF16, EPI_SILU_MUL>(k, pl, s)
             : d->epilogue == LS_EPI_QKV_ROPE ? launch_mt4<ElemF16, EPI_QKV_ROPE>(k, pl, s)
                                              : launch_mt<ElemF16, EPI_NONE>(k, pl, s);
    else
        rc = d->epilogue == LS_EPI_SILU_MUL   ? launch_mt<ElemBF16, EPI_SILU_MUL>(k, pl, s)
             : d->epilogue == LS_EPI_QKV_ROPE ? launch_mt4<ElemBF16, EPI_QKV_ROPE>(k, pl, s)
                                              : launch_mt<ElemBF16, EPI_NONE>(k, pl, s);
    if (d->ev_stop) (void)hipEventRecord(static_cast<hipEvent_t>(d->ev_stop), s);
    return rc;
}

}  // extern "C"
