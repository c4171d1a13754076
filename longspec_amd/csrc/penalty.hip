// penalty.hip -- repetition / presence / frequency penalties and a logit bias on the TARGET's lm_head logits, per row, and the
// per-(batch row, token) state they read (gfx950 / CDNA4).  No counterpart in the reference.
//
// State word (int32, one per batch row and token): bits 0-30 = times the token was generated, bit 31 = the token occurs in the
// prompt.  A row's history is that state plus the row's own selected "extras": the draft tokens on its path of the beam tree
// (mask row of the tree mask) or in front of it in the chain (a triangular mask).  Per element, fp32, one rounding per
// operation, no contraction (include/longspec_hip.h has the contract):
//   c = count(state) + extras equal to the column
//   c > 0 or prompt:  x = x > 0 ? x / repetition : x * repetition
//   c > 0:            x = x - frequency * float(c);  x = x - presence
//   bias:             x = x + bias[column]
// and x goes back to the 16-bit type, round to nearest even.
//
//   penalize_rows_kernel    grid (chunks of 8192 logits, rows, batch): the workgroup compacts its row's selected extras into
//                           LDS (ballot + prefix, no atomics), then every lane streams 4 x 8 columns with 16-byte accesses and
//                           counts the extras that fall into them
//   token_state_add_kernel  grid (ids / 256, batch): one integer atomic per id (add 1, or OR bit 31)
#include "rule_rows.h"

namespace {

constexpr int PN_THREADS = 256;
constexpr int PN_CHUNK = 8192;          // logits per workgroup: 4 x 8 per thread
constexpr int PN_MAX_EXTRA = 1024;

struct PenaltyArgs {
    const void* logits;
    void* out;
    const int32_t* state;
    const float* bias;
    long in_sb, in_sr, out_sb, out_sr, state_sb;
    RowExtras ex;            // C <= PN_MAX_EXTRA
    int V;
    float repetition, presence, frequency;
};

template <typename E>
__global__ __launch_bounds__(PN_THREADS) void penalize_rows_kernel(const PenaltyArgs a) {
    __shared__ int s_ids[PN_MAX_EXTRA];
    __shared__ int s_wave[4];
    using T = typename E::T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, row = blockIdx.y, z = blockIdx.z;
    const int V = a.V;
    // ---- the row's selected extras, compacted: order is free (only counts matter), the set is not
    int n_extra = 0;
    if (a.ex.C > 0) {
        const int C = a.ex.C;
        const int64_t* ids = a.ex.ids + (long)z * a.ex.ids_sb;
        const int64_t* mask = a.ex.mask + (long)z * a.ex.mask_sb + (long)row * a.ex.mask_sr;
        for (int base = 0; base < C; base += PN_THREADS) {                // (uniform trip count: barriers inside)
            const int c = base + tid;
            int64_t id = -1;
            if (c < C && mask[c] != 0) id = ids[c];
            const bool sel = id >= 0 && id < (int64_t)V;
            const unsigned long long bal = __ballot(sel);
            const int before = __popcll(bal & ((1ull << lane) - 1ull));
            if (lane == 0) s_wave[wave] = __popcll(bal);
            __syncthreads();
            int off = n_extra;
            for (int w = 0; w < wave; ++w) off += s_wave[w];
            if (sel) s_ids[off + before] = (int)id;
            n_extra += (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
            __syncthreads();
        }
    }
    const T* src = static_cast<const T*>(a.logits) + (long)z * a.in_sb + (long)row * a.in_sr;
    T* dst = static_cast<T*>(a.out) + (long)z * a.out_sb + (long)row * a.out_sr;
    const int32_t* state = a.state + (long)z * a.state_sb;
    // ---- loads first (four independent 16-byte requests per lane), then the extras, then the arithmetic
    uint4 raw[4];
    int col0[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        col0[j] = chunk * PN_CHUNK + (j * PN_THREADS + tid) * 8;
        raw[j] = make_uint4(0u, 0u, 0u, 0u);
        if (col0[j] < V) raw[j] = *reinterpret_cast<const uint4*>(src + col0[j]);         // V % 8 == 0: all-in or all-out
    }
    // extras per column, 16 bits each (a count is at most PN_MAX_EXTRA): columns 0-3 in lo, 4-7 in hi
    unsigned long long lo[4] = {0ull, 0ull, 0ull, 0ull}, hi[4] = {0ull, 0ull, 0ull, 0ull};
    for (int e = 0; e < n_extra; ++e) {
        const int id = s_ids[e];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned d = (unsigned)(id - col0[j]);
            const unsigned long long inc = d < 8u ? 1ull << ((d & 3u) * 16u) : 0ull;
            lo[j] += (d & 4u) ? 0ull : inc;
            hi[j] += (d & 4u) ? inc : 0ull;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (col0[j] >= V) continue;
        const uint4 w0 = *reinterpret_cast<const uint4*>(state + col0[j]);
        const uint4 w1 = *reinterpret_cast<const uint4*>(state + col0[j] + 4);
        const unsigned word[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
        float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (a.bias) {
            const float4 b0 = *reinterpret_cast<const float4*>(a.bias + col0[j]);
            const float4 b1 = *reinterpret_cast<const float4*>(a.bias + col0[j] + 4);
            bv[0] = b0.x; bv[1] = b0.y; bv[2] = b0.z; bv[3] = b0.w;
            bv[4] = b1.x; bv[5] = b1.y; bv[6] = b1.z; bv[7] = b1.w;
        }
        const unsigned in[4] = {raw[j].x, raw[j].y, raw[j].z, raw[j].w};
        unsigned res[4];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned short h = (unsigned short)((in[i >> 1] >> ((i & 1) * 16)) & 0xffffu);
            float x = E::to_f32(__builtin_bit_cast(T, h));
            const unsigned extra = (unsigned)(((i < 4 ? lo[j] : hi[j]) >> ((i & 3) * 16)) & 0xffffull);
            const unsigned c = (word[i] & 0x7fffffffu) + extra;
            if (c > 0u || (word[i] >> 31)) x = x > 0.f ? __fdiv_rn(x, a.repetition) : x * a.repetition;
            if (c > 0u) {
                const float t = a.frequency * (float)c;
                x = x - t;
                x = x - a.presence;
            }
            if (a.bias) x = x + bv[i];
            const unsigned short o = __builtin_bit_cast(unsigned short, E::from_f32(x));
            if (i & 1) res[i >> 1] |= (unsigned)o << 16;
            else res[i >> 1] = (unsigned)o;
        }
        *reinterpret_cast<uint4*>(dst + col0[j]) = make_uint4(res[0], res[1], res[2], res[3]);
    }
}

__global__ __launch_bounds__(PN_THREADS) void token_state_add_kernel(int32_t* __restrict__ state, long state_sb, int V,
                                                                     const int64_t* __restrict__ ids, long ids_sb, int n,
                                                                     const int64_t* __restrict__ num, long num_stride, int prompt) {
    const int j = blockIdx.x * PN_THREADS + threadIdx.x, z = blockIdx.y;
    if (j >= n) return;
    if (num && (int64_t)j >= num[(long)z * num_stride]) return;
    const int64_t id = ids[(long)z * ids_sb + j];
    if (id < 0 || id >= (int64_t)V) return;
    unsigned* word = reinterpret_cast<unsigned*>(state + (long)z * state_sb + id);
    if (prompt) atomicOr(word, 0x80000000u);
    else atomicAdd(word, 1u);
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" {

int ls_penalize_rows(const void* logits, void* out, int b, int rows, int vocab, int dtype, int64_t in_stride_b, int64_t in_stride_r,
                     int64_t out_stride_b, int64_t out_stride_r, const int32_t* state, int64_t state_stride_b,
                     const int64_t* extra_ids, int64_t ids_stride_b, const int64_t* extra_mask, int64_t mask_stride_b,
                     int64_t mask_stride_r, int n_extra, float repetition, float presence, float frequency, const float* bias,
                     void* stream) {
    if (!logits || !out || !state) LS_FAIL(LS_ERR_INVALID_ARG, "ls_penalize_rows: null pointer");
    if (dtype != LS_F16 && dtype != LS_BF16) LS_FAIL(LS_ERR_INVALID_ARG, "ls_penalize_rows: dtype");
    if (b < 1 || b > 65535 || rows < 1 || rows > 65535 || vocab < 8 || vocab > (1 << 24) || vocab % 8 != 0)
        LS_FAIL(LS_ERR_INVALID_ARG, "ls_penalize_rows: b=%d rows=%d vocab=%d (vocab a multiple of 8, <= 2^24; b, rows <= 65535)", b, rows,
                vocab);
    if (in_stride_r < vocab || out_stride_r < vocab || state_stride_b < vocab || in_stride_b < 0 || out_stride_b < 0 ||
        in_stride_b % 8 != 0 || in_stride_r % 8 != 0 || out_stride_b % 8 != 0 || out_stride_r % 8 != 0 || state_stride_b % 8 != 0)
        LS_FAIL(LS_ERR_INVALID_ARG, "ls_penalize_rows: row strides must be >= vocab and all strides multiples of 8 (in %ld/%ld, out "
                "%ld/%ld, state %ld)", (long)in_stride_b, (long)in_stride_r, (long)out_stride_b, (long)out_stride_r, (long)state_stride_b);
    if (!aligned16(logits) || !aligned16(out) || !aligned16(state) || (bias && !aligned16(bias)))
        LS_FAIL(LS_ERR_INVALID_ARG, "ls_penalize_rows: logits, out, state and bias must be 16-byte aligned");
    if (!(repetition > 0.f)) LS_FAIL(LS_ERR_INVALID_ARG, "ls_penalize_rows: repetition=%g must be > 0", (double)repetition);
    PenaltyArgs a;
    if (int rc = row_extras_check("ls_penalize_rows", extra_ids, ids_stride_b, extra_mask, mask_stride_b, mask_stride_r, n_extra,
                                  PN_MAX_EXTRA, a.ex))
        return rc;
    a.logits = logits; a.out = out; a.state = state; a.bias = bias;
    a.in_sb = (long)in_stride_b; a.in_sr = (long)in_stride_r; a.out_sb = (long)out_stride_b; a.out_sr = (long)out_stride_r;
    a.state_sb = (long)state_stride_b;
    a.V = vocab;
    a.repetition = repetition; a.presence = presence; a.frequency = frequency;
    const dim3 grid((vocab + PN_CHUNK - 1) / PN_CHUNK, rows, b), block(PN_THREADS);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == LS_F16) hipLaunchKernelGGL(penalize_rows_kernel<ElemF16>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(penalize_rows_kernel<ElemBF16>, grid, block, 0, s, a);
    LS_CHECK_LAUNCH("penalize_rows_kernel");
    return LS_OK;
}

int ls_token_state_add(int32_t* state, int b, int vocab, int64_t state_stride_b, const int64_t* ids, int n, int64_t ids_stride_b,
                       const int64_t* num, int64_t num_stride, int prompt, void* stream) {
    if (!state || !ids) LS_FAIL(LS_ERR_INVALID_ARG, "ls_token_state_add: null pointer");
    if (b < 1 || b > 65535 || vocab < 1 || state_stride_b < vocab || n < 0 || ids_stride_b < 0 || num_stride < 0)
        LS_FAIL(LS_ERR_INVALID_ARG, "ls_token_state_add: b=%d vocab=%d n=%d strides %ld/%ld/%ld", b, vocab, n, (long)state_stride_b,
                (long)ids_stride_b, (long)num_stride);
    if (n == 0) return LS_OK;
    const dim3 grid((n + PN_THREADS - 1) / PN_THREADS, b), block(PN_THREADS);
    hipLaunchKernelGGL(token_state_add_kernel, grid, block, 0, static_cast<hipStream_t>(stream), state, (long)state_stride_b, vocab, ids,
                       (long)ids_stride_b, n, num, (long)num_stride, prompt ? 1 : 0);
    LS_CHECK_LAUNCH("token_state_add_kernel");
    return LS_OK;
}

}  // extern "C"
