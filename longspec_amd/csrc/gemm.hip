// gemm.hip -- weight-streaming "skinny" linear layers for the decode round (gfx950 / CDNA4).
//
// Every projection of a draft or verify pass multiplies a handful of token rows (M = 1 ... 80:
// 74 verification rows, 4/16 tree-level rows, 1 vanilla row) by a weight matrix that has to be read
// from HBM in full: y[M,N] = x[M,K] . W[N,K]^T.  The flops are negligible next to the bytes of W, so
// the kernel is organised around the weight stream, not around an output tile:
//
//   * Weights are PRE-PACKED once (ls_linear_pack_weight) into the A-operand layout of
//     v_mfma_f32_16x16x32: the 1 KB block of (16-row tile, k-step s) holds lane l's 16 bytes
//     W[row0 + (l&15)][32s + 8(l>>4) ...] at byte 16*l, and the 4 tiles of a 64-row slab are adjacent.
//     A wave-wide global_load_dwordx4 of a block is one fully coalesced 1 KB read (8 full 128 B lines)
//     that lands directly in MFMA operand registers: W never touches LDS, and a wave walking the
//     k-steps of its slab streams contiguous memory, 4 KB per k-step.  (Loading
//     the row-major nn.Linear layout in MFMA lane order instead costs 64 separate 16 B L1 accesses per
//     instruction -- measured: 4x the TCP accesses and 2x the L2 requests of hipBLASLt, ~2.5 TB/s.)
//   * x (the few token rows; L2 resident) is the B operand.  Each wave stages the 64-k chunk it is
//     about to multiply through a wave-private LDS slab: coalesced loads (8 lanes = one 128 B line of a
//     row), XOR-swizzled ds_write_b128, conflict-free ds_read_b128 in MFMA lane order.  No workgroup
//     barrier is involved: LDS operations of one wave execute in order.
//   * A wave owns 64 output columns (4 MFMA tiles) x one quarter of the workgroup's k-range, so every x
//     fragment feeds 4 MFMAs; the next chunk of W (and of x) is in flight while the current one is
//     multiplied.  The 4 waves are reduced through LDS in a fixed order.
//   * Split-K across workgroups (needed to fill 256 CUs when N/64 < 256) is reduced in the SAME launch,
//     deterministically: partials go to a workspace with agent-coherent (write-through) stores, the
//     last workgroup to arrive at the slab's counter sums all S partials in split order -- the result
//     does not depend on arrival order -- and runs the epilogue.  No L2 write-back / invalidate is needed.
//     The k order of a row's dot product depends on (N, K) only, never on M: a token gets bit-identical
//     logits whether it is verified in a 74-row pass or decoded alone (vanilla).
//
// Epilogues: bias (q/k/v of the draft layer and of Qwen2), up to three weight segments sharing one x
// (q|k|v in one launch), and silu(gate) * up for the MLP -- with the reference's rounding points kept:
// each linear's output is rounded to the storage dtype before the next op uses it.
//
// Replaces, on the decode path (reference = longspec/test): llama.py:361-363,390 (q/k/v/o_proj),
// LlamaMLP.forward (transformers; vendored qwen2.py:218-230), llama_glide.py:248-250,268,285-287,305
// (draft projections), lm_head at llama_glide.py:960,1019,1046,1091.
#include <math.h>
#include <stdlib.h>

#include "skinny_gemm.h"

namespace {

// (The 64-row groups of a packed weight lie nks * 4 KB apart -- 512 KB for K = 4096 -- and the workgroups of a launch walk
// them at the same pace.  An 8 MB stride between the splits costs the attention 9 % (tools/sweep_cross_attn_128k.py); here
// 256 B, 4 KB and 36 KB of padding between the groups all measured within +-2 us of the unpadded layout on every projection,
// round 3, profiles/r3_gemm_group_pad.txt.)
constexpr int COUNTER_BYTES = 64 * 1024;   // fixed counter region at the head of the workspace (16384 slabs)

// The 16-bit weight format of skinny_gemm_body (skinny_gemm.h): a chunk is 2 k-steps x 4 tiles of 1 KB MFMA-ready blocks.
struct W16 {
    using Args = GemmK;
    static constexpr bool SCALED = false;
    static constexpr bool FOLDED_NORM = true;
    static constexpr int CHUNK_BYTES = 2 * 4096;
    static constexpr int TILE_BYTES = 1024, LANE_BYTES = 16;
    // M <= 16 / <= 32 / above with 64-row slabs: 4 / 3 / 3 chunks in flight per wave; 128-row slabs: 1 (16 KB)
    static constexpr int lac(int MT, int NT) { return NT == 8 ? 1 : MT == 1 ? 4 : 3; }
    template <typename E, int NT>
    struct Set {
        typename E::V8 a[2][NT];             // [k-step in chunk][tile]
    };
    // The weight stream: every byte is read ONCE per launch by ONE workgroup, so it is requested non-temporally
    // (`global_load_dwordx4 ... nt`: no allocation priority in L2 / MALL -- the x rows, the partials and the next kernel's
    // operands keep the cache).  MI355X_MICROARCH "nt-weights": issue -> landed -18 %, 5-10 % per decode layer against the
    // default policy.
    template <typename E, int NT>
    static __device__ __forceinline__ void issue(Set<E, NT>& s, const char* const (&wtile)[NT], int ks0) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int t = 0; t < NT; ++t)
                s.a[kk][t] = __builtin_nontemporal_load(reinterpret_cast<const typename E::V8*>(wtile[t] + (long)(ks0 + kk) * 4096));
    }
    template <typename E, int NT>
    static __device__ __forceinline__ void prefetch_chunk(const char* const (&wtile)[NT], int ks0) {      // default cache policy
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const typename E::V8 v = *reinterpret_cast<const typename E::V8*>(wtile[t] + (long)(ks0 + kk) * 4096);
                asm volatile("" : : "v"(v));
            }
    }
    template <typename E, int NT>
    static __device__ __forceinline__ typename E::V8 a_operand(const Set<E, NT>& s, int ks, int t) {
        return s.a[ks][t];
    }
};

template <typename E, int MT, int NT, int EPI, bool NORM>
__global__ __launch_bounds__(GEMM_THREADS, MT >= 5 ? 1 : 2) void skinny_gemm_kernel(const GemmK p) {
    skinny_gemm_body<E, W16, MT, NT, EPI, NORM>(p);
}

struct SkinnyGemm16 {            // host: the kernel family launch_skinny_gemm dispatches over
    using W = W16;
    static constexpr const char* NAME = "skinny_gemm_kernel";
    template <typename E, int MT, int NT, int EPI, bool NORM>
    static auto kernel() {
        return skinny_gemm_kernel<E, MT, NT, EPI, NORM>;
    }
};

// (Round 4's persistent layer-tail launch measured not faster: profiles/r4_tail_*.json.)

// ---- weight packing ---------------------------------------------------------------------
// The 64 rows of slab g at k-step s form one contiguous 4 KB block of 4 tiles:
// packed[((g * nks + s) * 4 + t) * 512 + l * 8 + e] = W[64 g + 16 t + (l & 15)][32 s + 8 (l >> 4) + e]
// (16-bit elements; rows >= N are zero).  A wave multiplying a slab reads 4 KB contiguous per k-step.
// Gate/up pairs (`w_up` != null) and `rope` permute the 16-row tiles: skinny_gemm.h::packed_tile_source.
__global__ __launch_bounds__(256) void pack_weight_kernel(const uint16_t* __restrict__ w, const uint16_t* __restrict__ w_up,
                                                          uint16_t* __restrict__ out, int N, int K, long nblocks, int rope) {
    const int nks = K >> 5;
    for (long blk = (long)blockIdx.x * 4 + (threadIdx.x >> 6); blk < nblocks; blk += (long)gridDim.x * 4) {
        const int t = (int)(blk & 3);
        const long gs = blk >> 2;
        const int g = (int)(gs / nks), ks = (int)(gs % nks);
        const int l = threadIdx.x & 63;
        int row;
        const uint16_t* src = packed_tile_source(g * 4 + t, l, w, w_up, rope, row);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (row < N) v = *reinterpret_cast<const uint4*>(src + (long)row * K + ks * 32 + (l >> 4) * 8);
        *reinterpret_cast<uint4*>(out + blk * 512 + l * 8) = v;
    }
}

// ---- host side ---------------------------------------------------------------------------
int num_cus_gemm() {
    static int n = 0;
    if (n == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
        if (n <= 0) n = 256;
    }
    return n;
}

using Plan = GemmPlan;       // ls_common.h: gemm_w8.hip launches the same plan

int pick_mt(int M) { return M <= 16 ? 1 : M <= 32 ? 2 : M <= 80 ? 5 : 0; }

// The split count is a function of (N, K, epilogue) ONLY -- never of M -- so that a row's
// summation order is the same in every pass (see the header comment).  `groups` = 64-row groups of W.
int pick_splits(int groups, int nks, int forced) {
    const int smax = nks / 16 > 0 ? nks / 16 : 1;     // at least 512 k (8 chunks) per split
    if (forced > 0) return forced < smax ? forced : smax;
    const int cus = 256;
    if (groups >= cus) return 1;                      // a weight that already fills the chip is never split
    // Measured model of a launch (rocprofv3, M = 74, K = 4096 / 14336; fits within ~1 us):
    //   t = rounds x (bytes per workgroup / stream rate + 3 us of ramp) + 0.4 us x S of partial traffic,
    //   stream rate per workgroup = min(27 GB/s, 6 TB/s / resident workgroups), rounds = ceil(groups x S / 256).
    const double bytes_per_group = 64.0 * nks * 32 * 2;
    int best = 1;
    double best_t = 1e30;
    for (int S = 1; S <= smax && S <= 32; ++S) {
        const int wgs = groups * S;
        const int rounds = (wgs + cus - 1) / cus;
        const double rate = fmin(27e9, 6e12 / (wgs < cus ? wgs : cus));
        const double t = rounds * (bytes_per_group / S / rate + 3e-6) + 0.4e-6 * S;
        if (t < best_t - 1e-9) { best_t = t; best = S; }
    }
    return best;
}

int make_plan(const ls_linear_desc* d, Plan& pl) {
    if (!d || !d->x || !d->y || !d->w[0]) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear: null pointer");
    if (d->dtype != LS_F16 && d->dtype != LS_BF16) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear: dtype");
    if (d->M < 1 || d->K < 128 || d->K % 64 != 0)
        LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear: K=%d must be a multiple of 64, >= 128", d->K);
    pl.MT = pick_mt(d->M);
    if (pl.MT == 0) LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear: M=%d > 80 rows is a plain library GEMM, not this kernel", d->M);
    if (d->n_seg < 1 || d->n_seg > 3) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear: n_seg");
    if (d->ldx < d->K) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear: ldx < K");
    if ((d->ldx % 8) != 0 || (d->ldy % 4) != 0) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear: ldx must be a multiple of 8, ldy of 4");
    int rows;                                           // rows of the packed matrix the grid covers
    if (d->epilogue == LS_EPI_SILU_MUL) {
        if (d->n_seg != 1) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear: silu_mul takes ONE weight packed by ls_linear_pack_gate_up");
        if (d->n[0] < 1 || d->n[0] % 16 != 0) LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear: silu_mul needs N %% 16 == 0");
        pl.N = d->n[0];
        rows = 2 * d->n[0];
    } else if (d->epilogue == LS_EPI_NONE || d->epilogue == LS_EPI_QKV_ROPE) {
        if (d->epilogue == LS_EPI_QKV_ROPE) {
            if (!d->rope_cos || !d->rope_sin) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear: qkv_rope needs the cos/sin tables");
            for (int i = 0; i < d->n_seg; ++i)
                if (d->n[i] % 128 != 0) LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear: qkv_rope segments are heads x 128 rows");
        }
        int N = 0;
        for (int i = 0; i < d->n_seg; ++i) {
            if (!d->w[i] || d->n[i] < 1) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear: segment %d", i);
            if (d->n_seg > 1 && d->n[i] % 128 != 0) LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear: multi-segment rows must be multiples of 128");
            if (d->n[i] % 4 != 0) LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear: N %% 4");
            N += d->n[i];
        }
        pl.N = N;
        rows = N;
    } else {
        LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear: epilogue");
    }
    if (d->ldy < pl.N) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear: ldy < N");
    if (d->residual && (d->epilogue != LS_EPI_NONE || d->ldr < pl.N || (d->ldr % 4) != 0))
        LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear: residual goes with LS_EPI_NONE, ldr >= N, ldr %% 4 == 0");
    if (d->norm_weight && (!d->ssq_in || d->ssq_parts < 1))
        LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear: norm_weight needs the rows' sum-of-squares partials (ssq_in, ssq_parts)");
    if (d->ssq_out && (d->epilogue != LS_EPI_NONE || d->n_seg != 1 || pl.N % 64 != 0))
        LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear: ssq_out goes with LS_EPI_NONE, one segment, N %% 64 == 0");
    const int groups = (rows + 63) / 64;
    // more than 32 token rows run ONE workgroup per CU (512 registers per wave): give it 128 weight rows when that
    // still fills the chip -- half the x staging traffic, half the workgroups (measured: lm_head 230 -> 209 us)
    pl.NT = (pl.MT >= 5 && groups >= 2 * 224 && d->epilogue != LS_EPI_QKV_ROPE) ? 8 : 4;
    pl.nslabs = (rows + pl.NT * 16 - 1) / (pl.NT * 16);
    pl.nks = d->K / 32;
    pl.S = pick_splits(groups, pl.nks, d->n_splits);
    if (pl.NT == 8) pl.S = d->n_splits > 0 ? pl.S : 1;
    if ((size_t)pl.nslabs * 4 > COUNTER_BYTES) LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear: N too large (%d slabs)", pl.nslabs);
    pl.lds = (size_t)16 * 4 * pl.MT * 64 * 4 + 16;     // 4 waves x 4 tiles x MT accumulators (>= the 4 x-slabs) + the last-arriver flag
    pl.flag_off = (int)pl.lds - 16;
    if (d->norm_weight) pl.lds += (size_t)pl.MT * 64 + (size_t)d->K * 2;      // + 1 / rms of the rows + the norm weight
    if (pl.lds > 160 * 1024) LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear: K=%d too large for a folded norm", d->K);
    pl.counter_bytes = COUNTER_BYTES;
    pl.part_bytes = pl.S > 1 ? (size_t)pl.S * pl.nslabs * pl.NT * pl.MT * 4 * 64 * 4 : 0;
    return LS_OK;
}

}  // namespace

int gemm_make_plan(const ls_linear_desc* d, GemmPlan& pl) { return make_plan(d, pl); }

extern "C" {

size_t ls_linear_packed_bytes(int N, int K) {
    if (N < 1 || K < 32 || K % 32 != 0) return 0;
    return (size_t)((N + 63) / 64) * (64 * (size_t)K * 2);
}

static int pack_impl(const void* w, const void* w_up, void* packed, int N, int K, int dtype, void* stream, const char* what,
                     int rope = 0) {
    if (!w || !packed) LS_FAIL(LS_ERR_INVALID_ARG, "%s: null pointer", what);
    if (dtype != LS_F16 && dtype != LS_BF16) LS_FAIL(LS_ERR_INVALID_ARG, "%s: dtype", what);
    if (N < 1 || K < 32 || K % 32 != 0) LS_FAIL(LS_ERR_UNSUPPORTED, "%s: K=%d must be a multiple of 32", what, K);
    const int rows = w_up ? 2 * N : N;
    const long nblocks = (long)((rows + 63) / 64) * 4 * (K / 32);
    long grid = (nblocks + 3) / 4;
    if (grid > 65535 * 4) grid = 65535 * 4;
    hipLaunchKernelGGL(pack_weight_kernel, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t*>(w), static_cast<const uint16_t*>(w_up), static_cast<uint16_t*>(packed), N, K,
                       nblocks, rope);
    LS_CHECK_LAUNCH("pack_weight_kernel");
    return LS_OK;
}

int ls_linear_pack_weight(const void* weight, void* packed, int N, int K, int dtype, void* stream) {
    return pack_impl(weight, nullptr, packed, N, K, dtype, stream, "ls_linear_pack_weight");
}

int ls_linear_pack_gate_up(const void* gate_weight, const void* up_weight, void* packed, int N, int K, int dtype, void* stream) {
    if (!up_weight) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear_pack_gate_up: null pointer");
    if (N % 16 != 0) LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear_pack_gate_up: N %% 16");
    return pack_impl(gate_weight, up_weight, packed, N, K, dtype, stream, "ls_linear_pack_gate_up");
}

int ls_linear_pack_rope(const void* weight, void* packed, int N, int K, int dtype, void* stream) {
    if (N % 128 != 0) LS_FAIL(LS_ERR_UNSUPPORTED, "ls_linear_pack_rope: N must be heads x 128 rows");
    return pack_impl(weight, nullptr, packed, N, K, dtype, stream, "ls_linear_pack_rope", 1);
}

size_t ls_linear_workspace_bytes(const ls_linear_desc* d) {
    Plan pl;
    if (make_plan(d, pl) != LS_OK) return 0;
    return pl.counter_bytes + pl.part_bytes;
}

static int linear_launch(const ls_linear_desc* d, void* workspace, size_t workspace_bytes, void* stream, int prefetch_units) {
    Plan pl;
    int rc = make_plan(d, pl);
    if (rc != LS_OK) return rc;
    if (!workspace || workspace_bytes < pl.counter_bytes + pl.part_bytes)
        LS_FAIL(LS_ERR_WORKSPACE, "ls_linear_fwd: workspace %zu < %zu bytes", workspace_bytes, pl.counter_bytes + pl.part_bytes);
    GemmK k{};
    fill_gemm_args(k, d, pl, workspace);
    k.prefetch_units = prefetch_units;
    return launch_skinny_gemm<SkinnyGemm16>(d, k, pl, static_cast<hipStream_t>(stream));
}

int ls_linear_fwd(const ls_linear_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    return linear_launch(d, workspace, workspace_bytes, stream, 0);
}

int ls_linear_prefetch(const ls_linear_desc* d, int units, void* workspace, size_t workspace_bytes, void* stream) {
    if (units < 1) LS_FAIL(LS_ERR_INVALID_ARG, "ls_linear_prefetch: units");
    return linear_launch(d, workspace, workspace_bytes, stream, units);
}

}  // extern "C"
