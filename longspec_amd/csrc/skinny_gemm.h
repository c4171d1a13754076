// skinny_gemm.h -- the ONE body of the weight-streaming skinny GEMM, shared by its three translation units:
//   gemm.hip     16-bit weights (policy W16, kernel skinny_gemm_kernel)     -- the design is described in its header comment
//   gemm_w8.hip  e4m3 weights   (policy W8,  kernel skinny_gemm_w8_kernel)
//   gemm_w4.hip  MXFP4 weights  (policy W4,  kernel skinny_gemm_w4_kernel)
// A weight-format policy `W` supplies exactly what the format changes; the segment / tile set-up, the x staging, the
// steady-state and drain loops, the 4-wave reduction, the split-K last-arriver protocol and the epilogues exist once, so
// "same plan, same k order, same rounding points in both formats" holds by construction.
//
//   W::Args                     kernel argument struct: GemmK, or GemmK with the row scales appended
//   W::CHUNK_BYTES              bytes of one 64-k chunk of a 64-row group, the stride of the weight stream
//   W::TILE_BYTES, LANE_BYTES   inside a chunk: tile t's block starts at t * TILE_BYTES, lane l's bytes at l * LANE_BYTES
//   W::lac(MT, NT)              chunks of look-ahead per wave
//   W::Set<E, NT>               the registers of one chunk of the workgroup's NT tiles
//   W::issue<E, NT>(set, wtile, ks0)          request the chunk that starts at k-step ks0 (non-temporal in both formats)
//   W::a_operand<E, NT>(set, ks, t)           MFMA A operand of k-step ks (0, 1) of tile t
//   W::SCALED, W::scale4(p, i, n, valid)      fp32 row scales i of output columns n .. n+3 of that segment, applied to the
//                                             reduced sums in front of bias / rounding
//   W::FOLDED_NORM              the format has the folded RMSNorm, ssq_out and ls_linear_prefetch (W::prefetch_chunk)
// The host side launches through a kernel family F next to each wrapper: F::W, F::NAME, F::kernel<E, MT, NT, EPI, NORM>().
#pragma once
#include "ls_common.h"

// (An anonymous namespace in a header, on purpose: this header is the shared part of exactly three translation units whose
// own contents are anonymous too, and the kernels' mangled names -- which tools and tests match -- contain it.)
namespace {

constexpr int GEMM_THREADS = 256;

struct GemmK {
    const char* x;
    long ldx;                    // elements
    const char* w[3];            // segment weights [n_i, K]  (SILU: w[0] = gate, w[1] = up)
    const char* bias[3];         // or null
    int n[3];                    // segment rows
    char* y;
    long ldy;                    // elements
    float* part;                 // split-K partials
    unsigned* counters;          // one per slab, zero between launches
    int M, K, N;                 // N = total output columns
    int nks, S, nslabs;          // nks = K / 32 k-steps
    int flag_off;                // byte offset of the last-arriver flag in dynamic LDS
    const char* rope_cos;        // EPI_QKV_ROPE: [M, 128] dtype tables of the rows' positions
    const char* rope_sin;
    int rope_segs;               // leading segments (q, k) that are rotated; the rest (v) are plain
    const char* residual;        // EPI_NONE: [M, N] dtype added to the rounded output (`residual + mlp(x)`), or null
    long ldr;
    // RMSNorm folded into the launch (NORM): x is the UN-normalised residual stream; its rows' sums of squares arrive
    // as `ssq_parts` partials per row (one per 64 columns, written by the launch that produced x), the norm weight is
    // applied while x is staged.  `ssq_out` (EPI_NONE): this launch is such a producer.
    const float* ssq_in;         // [M, ssq_parts]
    int ssq_parts;
    const char* norm_w;          // [K] dtype
    float norm_eps;
    float* ssq_out;              // [M, N / 64] or null
    int prefetch_units;          // > 0: ls_linear_prefetch -- every wave only REQUESTS its first chunks (default cache policy) and exits
};

enum { EPI_NONE = 0, EPI_SILU_MUL = 1, EPI_QKV_ROPE = 2 };

// agent-coherent accesses (sc1: write-through / cache-bypassing), so that partials written by a workgroup
// on one XCD are read correctly by the reducing workgroup on another without an L2 write-back + invalidate
// 16 bytes per lane (one accumulator quad): scalar sc1 stores are one fabric write EACH -- a dword costs ~6x the time per
// byte of a dwordx4 (MI355X_MICROARCH, visibility table) -- so a partial tile travels as `buffer_store_dwordx4 ... sc1` of
// the lane's f32x4, 1 KB contiguous per wave-instruction.  aux 16 = sc1 on gfx950.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t part_rsrc(const float* base, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ void st_coherent4(__amdgpu_buffer_rsrc_t r, unsigned byte_off, f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, byte_off, 0, 16);
}
__device__ __forceinline__ f32x4 ld_coherent4(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 16));
}

// MT = 16-row tiles of x (M <= 16*MT); NT = 16-row weight tiles per workgroup (4: one packed slab, 8: two)
// NORM: `x` is normalised on the way into LDS -- LlamaRMSNorm's arithmetic (misc.hip::rmsnorm_rows_kernel), with the row
// sums of squares taken from the producer's 64-column partials in the canonical order (ls_common.h::ssq_*).
template <typename E, typename W, int MT, int NT, int EPI, bool NORM>
__device__ __forceinline__ void skinny_gemm_body(const typename W::Args& args) {
    // A local copy, as a by-value kernel parameter is: every field becomes one scalar load at the head of the kernel and
    // lives in SGPRs.  Read through the reference, the loops re-request fields (p.x in every drain step) and wait for them.
    const typename W::Args p = args;
    static_assert(W::FOLDED_NORM || !NORM, "the folded RMSNorm exists for 16-bit weights only");
    using V8 = typename E::V8;
    using V4 = typename E::V4;
    // A W register set holds one 64-k chunk (2 k-steps) of the workgroup's NT tiles, and the look-ahead is counted in
    // chunks.  M <= 32: 2 waves per SIMD (256 registers each); above: 1 wave per SIMD with the full 512.  (Round 4 gave the
    // 128-row 16-bit variant k-step-granular sets instead, 24 KB per wave in flight instead of one 16 KB chunk of look-ahead:
    // lm_head 202 vs 207 us, gate|up+SiLU 47.0 vs 45.4 us, GEMM per round 5.57-5.72 vs 5.60-5.65 ms -- no gain, the 128-row
    // launches are not limited by their look-ahead; profiles/r4_ab_kstep8_*.json.)
    constexpr int LAC = W::lac(MT, NT);
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
    const int nch_all = p.nks >> 1;          // 64-k chunks of K
    const int ch_begin = (int)(((long)nch_all * split) / p.S);
    const int ch_end = (int)(((long)nch_all * (split + 1)) / p.S);

    // ---- the NT weight tiles of this workgroup.  The 64-k chunk c of 64-row group g starts at (g * K/64 + c) * CHUNK_BYTES
    // and is made of TILE_BYTES blocks, those of the group's 4 tiles adjacent (which blocks: the policy's translation unit).
    // EPI_SILU_MUL: the packed matrix alternates gate and up tiles (tile 2j = gate rows 16j.., tile 2j+1 = up rows
    // 16j..), so tiles (2j, 2j+1) make output columns 16j..16j+15.
    // EPI_QKV_ROPE: like EPI_NONE, but the q and k segments are packed in rope order (within each 128-row
    // head, tile 2j = rows 16j.., tile 2j+1 = rows 64+16j..: a rotary pair sits in neighbouring tiles).
    const char* wtile[NT];
    const char* bias_p = nullptr;
    int n_lim;                   // end of the valid output columns of this slab's segment (global column)
    int n_tile0;                 // global output column of tile 0
    int seg_base = 0, seg = 0;
    const long group_b = (long)p.nks * (W::CHUNK_BYTES / 2);
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
            wtile[t] = p.w[seg] + (long)g * group_b + (t & 3) * W::TILE_BYTES + lane * W::LANE_BYTES;
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

    typename W::template Set<E, NT> wa[NCS];
    V8 xs[XL];                   // x staging: piece i = rows 8i .. 8i+7, lane -> (row 8i + lane/8, 16 B slot lane%8)
    char* xlds = smem + wave * XSLAB;
    const int xr_in = lane >> 3, xslot = lane & 7;

    unsigned xoff[XL];           // 32-bit byte offsets of this lane's 16 B in each piece (x is far below 4 GB)
#pragma unroll
    for (int i = 0; i < XL; ++i) xoff[i] = (unsigned)(((long)min(i * 8 + xr_in, p.M - 1) * p.ldx + xslot * 8) * 2);
    // NORM: behind the last-arriver flag the launch keeps 1 / rms of every row (fp32 [MT * 16]) and the norm weight
    // (dtype [K]) in LDS; both are read back per piece / per chunk rather than held in registers (the 128-row variant
    // has none to spare)
    const float* rs = reinterpret_cast<const float*>(smem + p.flag_off + 16);
    const char* nwl = smem + p.flag_off + 16 + MT * 64;
    int x_ch = 0;                // the chunk in `xs`
    auto load_x = [&](int ch) {
        const char* xc = p.x + (long)ch * 128;            // wave-uniform
#pragma unroll
        for (int i = 0; i < XL; ++i) xs[i] = *reinterpret_cast<const V8*>(xc + xoff[i]);
        if (NORM) x_ch = ch;
    };
    auto store_x = [&]() {       // slot ^ ((row >> 1) & 7): 16 rows x one slot hit 16 distinct 16 B bank groups
        V8 nw;
        if (NORM) nw = *reinterpret_cast<const V8*>(nwl + x_ch * 128 + xslot * 16);
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const int row = i * 8 + xr_in;
            V8 v = xs[i];
            if (NORM) {
                const float rstd = rs[row];
#pragma unroll
                for (int e = 0; e < 8; ++e) {             // weight * dtype(x32 * rsqrt(mean(x32^2) + eps))
                    const float n = round_to<E>(E::to_f32(v[e]) * rstd);
                    v[e] = E::from_f32(E::to_f32(nw[e]) * n);
                }
            }
            *reinterpret_cast<V8*>(xlds + row * 128 + ((xslot ^ ((row >> 1) & 7)) << 4)) = v;
        }
    };
    // chunk `c` of this wave = k-steps ch0 * 2 + c * 2, + 1 of the slab
    auto issue_w = [&](int c, int set) { W::template issue<E, NT>(wa[set], wtile, ch0 * 2 + c * 2); };
    auto mma_chunk = [&](int set) {
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
                const V8 a = W::template a_operand<E, NT>(wa[set], ks, t);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[t][mt] = E::mfma(a, bx[mt], acc[t][mt]);
            }
        }
    };

    if constexpr (W::FOLDED_NORM) {
        if (p.prefetch_units > 0) {
            // ls_linear_prefetch: pull the first chunks of every wave's weight stream into the L2 of the XCD that the matching
            // workgroup of the real launch will run on (same grid, block b -> XCD b % 8 as observed; speed only), with the
            // DEFAULT cache policy -- the later nt loads hit those lines
            const int n = min(nch, p.prefetch_units);
            for (int i = 0; i < n; ++i) W::template prefetch_chunk<E, NT>(wtile, ch0 * 2 + i * 2);
            return;
        }
    }
    if (nch > 0) load_x(ch0);
#pragma unroll
    for (int i = 0; i < LAC; ++i)
        if (i < nch) issue_w(i, i);
    if (NORM) {
        // behind the first weight requests: thread r sums row r's partials in slab order (the canonical order)
        float* rsw = reinterpret_cast<float*>(smem + p.flag_off + 16);
        for (int i = tid * 16; i < p.K * 2; i += GEMM_THREADS * 16)
            *reinterpret_cast<uint4*>(smem + p.flag_off + 16 + MT * 64 + i) = *reinterpret_cast<const uint4*>(p.norm_w + i);
        if (tid < MT * 16) {
            const float tot = ssq_row(p.ssq_in + (long)min(tid, p.M - 1) * p.ssq_parts, p.ssq_parts);
            rsw[tid] = rsqrtf(tot / (float)p.K + p.norm_eps);
        }
        __syncthreads();
    }
    int c = 0;
    // steady state: no control flow inside, so the compiler's in-order vmcnt counts stay exact;
    // sched_barrier(0) keeps the loads of the chunks ahead in front of the MFMAs of the current one
    for (; c + NCS - 1 + LAC < nch; c += NCS) {
#pragma unroll
        for (int u = 0; u < NCS; ++u) {
            store_x();                                   // chunk c+u: staging registers -> the wave's LDS slab
            load_x(ch0 + (c + u) + 1);                   // (the last chunk of the wave is never in this loop: LAC >= 1)
            issue_w(c + u + LAC, (u + LAC) % NCS);
            __builtin_amdgcn_sched_barrier(0);
            mma_chunk(u);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int u = 0; u < NCS + LAC - 1; ++u) {            // drain
        if (c + u < nch) {
            store_x();
            if (c + u + 1 < nch) load_x(ch0 + (c + u) + 1);
            if (c + u + LAC < nch) issue_w(c + u + LAC, (u + LAC) % NCS);
            __builtin_amdgcn_sched_barrier(0);
            mma_chunk(u % NCS);
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

    // ---- split-K: deterministic last-arriver reduction
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
        // Every thread drains its OWN write-through (sc1) partial stores before the barrier: only then may thread 0
        // bump the slab counter.  (A workgroup-scope fence does not emit the wait -- the compiler left vmcnt(63)
        // in front of the barrier -- so the last arriver, possibly on another XCD, could sum partials still in
        // flight.  The asm wait is invisible to the waitcnt-elision pass: MI355X_MICROARCH, "Compiler hazard".)
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

    // ---- epilogue: lane holds the fp32 sums of y[m = mt*16 + l15][n .. n+3].  SCALED: the row scales come first, in front
    // of bias, rounding, SiLU, RoPE and the residual add.
    // MODIFIES the reduced sums in place: v *= row scales i of the global columns n .. n+3 (no-op unless W::SCALED)
    auto scale_rows = [&](f32x4 (&v)[MT], int i, int n) {
        if constexpr (W::SCALED) {
            const f32x4 s = W::scale4(p, i, n - seg_base, n < n_lim);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) v[mt] *= s;
        }
    };
#pragma unroll
    for (int h = 0; h < NPASS; ++h) {
        if (EPI == EPI_SILU_MUL) {
            const int nn = n_tile0 + (h * 2 + wave) * 16 + g4 * 4;
            scale_rows(r[h][0], 0, nn);
            scale_rows(r[h][NT_OUT - 1], 1, nn);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int m = mt * 16 + l15;
                V4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float g = round_to<E>(r[h][0][mt][e]);              // gate_proj output in the storage dtype
                    const float u = round_to<E>(r[h][NT_OUT - 1][mt][e]);     // up_proj output
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
            scale_rows(r[h][0], seg, n_lo);
            scale_rows(r[h][NT_OUT - 1], seg, n_hi);
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
                    lo[e] = E::from_f32(r[h][0][mt][e] + bl[e]);
                    hi[e] = E::from_f32(r[h][1][mt][e] + bh[e]);
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
            scale_rows(r[h][0], seg, nn);
            float bv[4] = {0.f, 0.f, 0.f, 0.f};
            float tsq[MT];
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
                for (int e = 0; e < 4; ++e) o[e] = E::from_f32(r[h][0][mt][e] + bv[e]);
                if (m < p.M && nn < n_lim) {
                    if (p.residual != nullptr) {           // the projection is rounded first, then added (llama_glide.py:466)
                        const V4 r4 = *reinterpret_cast<const V4*>(p.residual + ((long)m * p.ldr + nn) * 2);
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = E::from_f32(E::to_f32(o[e]) + E::to_f32(r4[e]));
                    }
                    *reinterpret_cast<V4*>(p.y + ((long)m * p.ldy + nn) * 2) = o;
                }
                // this tile's 16 columns of row m in the canonical order (every lane takes part in the shuffles)
                if constexpr (W::FOLDED_NORM)
                    if (p.ssq_out != nullptr) tsq[mt] = ssq_tile16(ssq_quad(E::to_f32(o[0]), E::to_f32(o[1]), E::to_f32(o[2]), E::to_f32(o[3])));
            }
            if (W::FOLDED_NORM && p.ssq_out != nullptr) {  // (uniform) the slab's 64 columns: tiles in wave order
                __syncthreads();                           // the 4-wave reduction no longer reads `red`
                if (g4 == 0) {
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) red[wave * (MT * 16) + mt * 16 + l15] = tsq[mt];
                }
                __syncthreads();
                if (tid < MT * 16 && tid < p.M) {
                    const int R = MT * 16;
                    p.ssq_out[(long)tid * (p.N >> 6) + slab * NPASS + h] = ssq_slab64(red[tid], red[R + tid], red[2 * R + tid], red[3 * R + tid]);
                }
                __syncthreads();
            }
        }
    }
}

// ---- weight packing: the tile permutation all packers share.  Packed 16-row tile T, lane l holds a row of `w`, or of
// `w_up`: a gate/up pair is packed as ONE matrix of 2N rows whose tiles alternate (tile 2j = gate rows 16j.., tile 2j+1 =
// up rows 16j..: the silu(gate)*up epilogue pairs neighbouring tiles).  `rope` packs a q/k projection for EPI_QKV_ROPE:
// within every 128-row head the 8 tiles are stored in the order 0,4,1,5,2,6,3,7, so that rows d.. and 64+d.. (a rotary
// pair) are neighbouring tiles of one workgroup.  Returns the source matrix and sets `row`.
template <typename B>
__device__ __forceinline__ const B* packed_tile_source(int T, int l, const B* w, const B* w_up, int rope, int& row) {
    const B* src = w;
    row = T * 16 + (l & 15);
    if (w_up != nullptr) {
        src = (T & 1) ? w_up : w;
        row = (T >> 1) * 16 + (l & 15);
    } else if (rope) {
        row = ((T & ~7) + ((T & 7) >> 1) + 4 * (T & 1)) * 16 + (l & 15);
    }
    return src;
}

// ---- host side: the kernel arguments of a planned launch, and the dtype x epilogue x (MT, NT) ladder -----------------------
// (the norm / ssq fields are copied for every format: a format without FOLDED_NORM has rejected descriptors that set them
// before it plans -- gemm_w8.hip::make_plan_w8 -- so they are null there)
inline void fill_gemm_args(GemmK& k, const ls_linear_desc* d, const GemmPlan& pl, void* workspace) {
    k.x = static_cast<const char*>(d->x);
    k.ldx = d->ldx;
    for (int i = 0; i < 3; ++i) {
        k.w[i] = i < d->n_seg ? static_cast<const char*>(d->w[i]) : nullptr;
        k.bias[i] = i < d->n_seg ? static_cast<const char*>(d->bias[i]) : nullptr;
        k.n[i] = i < d->n_seg ? d->n[i] : 0;
    }
    k.y = static_cast<char*>(d->y);
    k.ldy = d->ldy;
    k.counters = static_cast<unsigned*>(workspace);
    k.part = reinterpret_cast<float*>(static_cast<char*>(workspace) + pl.counter_bytes);
    k.M = d->M;
    k.K = d->K;
    k.N = pl.N;
    k.nks = pl.nks;
    k.S = pl.S;
    k.nslabs = pl.nslabs;
    k.flag_off = pl.flag_off;
    k.rope_cos = static_cast<const char*>(d->rope_cos);
    k.rope_sin = static_cast<const char*>(d->rope_sin);
    k.rope_segs = d->n_seg < 2 ? d->n_seg : 2;
    k.residual = static_cast<const char*>(d->residual);
    k.ldr = d->ldr;
    k.norm_w = static_cast<const char*>(d->norm_weight);
    k.norm_eps = d->norm_eps;
    k.ssq_in = d->ssq_in;
    k.ssq_parts = d->ssq_parts;
    k.ssq_out = d->ssq_out;
}

template <typename F, typename E, int MT, int NT, int EPI, bool NORM>
int launch_kernel(const typename F::W::Args& k, const GemmPlan& pl, hipStream_t s) {
    auto kern = F::template kernel<E, MT, NT, EPI, NORM>();
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_done = true;
    }
    hipLaunchKernelGGL(kern, dim3(pl.nslabs, pl.S), dim3(GEMM_THREADS), pl.lds, s, k);
    LS_CHECK_LAUNCH(F::NAME);
    return LS_OK;
}

template <typename F, typename E, int MT, int NT, int EPI>
int launch_norm(const typename F::W::Args& k, const GemmPlan& pl, hipStream_t s) {
    if constexpr (F::W::FOLDED_NORM)
        if (k.norm_w != nullptr) return launch_kernel<F, E, MT, NT, EPI, true>(k, pl, s);
    return launch_kernel<F, E, MT, NT, EPI, false>(k, pl, s);
}

template <typename F, typename E, int EPI>
int launch_tiles(const typename F::W::Args& k, const GemmPlan& pl, hipStream_t s) {
    switch (pl.MT) {
        case 1: return launch_norm<F, E, 1, 4, EPI>(k, pl, s);
        case 2: return launch_norm<F, E, 2, 4, EPI>(k, pl, s);
    }
    if constexpr (EPI != EPI_QKV_ROPE)                   // (the plan gives the rope epilogue 4-tile slabs only)
        if (pl.NT == 8) return launch_norm<F, E, 5, 8, EPI>(k, pl, s);
    return launch_norm<F, E, 5, 4, EPI>(k, pl, s);
}

template <typename F, typename E>
int launch_epilogue(int epilogue, const typename F::W::Args& k, const GemmPlan& pl, hipStream_t s) {
    return epilogue == LS_EPI_SILU_MUL   ? launch_tiles<F, E, EPI_SILU_MUL>(k, pl, s)
           : epilogue == LS_EPI_QKV_ROPE ? launch_tiles<F, E, EPI_QKV_ROPE>(k, pl, s)
                                         : launch_tiles<F, E, EPI_NONE>(k, pl, s);
}

// `d` has passed gemm_make_plan (dtype and epilogue are valid); records the descriptor's timing events around the kernel
template <typename F>
int launch_skinny_gemm(const ls_linear_desc* d, const typename F::W::Args& k, const GemmPlan& pl, hipStream_t s) {
    if (d->ev_start) (void)hipEventRecord(static_cast<hipEvent_t>(d->ev_start), s);
    const int rc = d->dtype == LS_F16 ? launch_epilogue<F, ElemF16>(d->epilogue, k, pl, s) : launch_epilogue<F, ElemBF16>(d->epilogue, k, pl, s);
    if (d->ev_stop) (void)hipEventRecord(static_cast<hipEvent_t>(d->ev_stop), s);
    return rc;
}

}  // namespace
