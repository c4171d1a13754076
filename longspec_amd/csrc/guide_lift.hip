// guide_lift.hip -- the lift of a byte-level DFA to the tokens of a vocabulary (Guide.from_byte_dfa / Guide.from_regex with a
// device; gfx950 / CDNA4).  No counterpart in the reference.
//
// A token's behaviour is the vector state -> state of running its bytes through the DFA.  The operands:
//   step     16-bit [256, S + 1], BYTE-major: step[c, s] = the state behind byte c in state s, S = the dead state (column S maps to
//            S).  A wave whose lanes hold different states of one token gathers from ONE contiguous (S + 1) * 2-byte row per byte.
//   blob     the bytes of all tokens, back to back; offsets int32 [T + 1]: token t is blob[offsets[t] : offsets[t + 1]]
// Lanes run across states.  W = the smallest power of two >= min(S, 64) lanes hold one token's states s, s + 64, s + 128, ...;
// for S < 64 a wave holds 64 / W tokens, so that lanes do not idle; beyond 64 states a wave takes LS_K slices of 64 states per pass
// over the token's bytes (K independent gathers in flight) and as many passes as S needs.  A token's bytes are uniform across its
// lanes: no divergence but the ends of tokens of different lengths within a packed wave.  Everything read is clamped: an offset
// pair that does not lie in the blob counts as an empty token, a step entry beyond S as S, a token id outside [0, T) as empty.
//
//   MODE_HASH   per token two independent 64-bit hashes of its vector (wrap-around sums over s of a mix of (s, end state of s),
//               reduced across the token's lanes with shuffles) and its alive flag (non-empty and some state survives)
//   MODE_COLS   the exact vectors of a list of token ids, int32 [n, S], -1 = dead
//   MODE_CHECK  every token with group[t] >= 0 recomputes its vector and compares it with reps[group[t]]; one mismatch byte per token
// No scratch, no LDS, no atomics, no floating point.  Every output element is written by every call.
#include "ls_common.h"

namespace {

constexpr int GL_THREADS = 256, GL_WAVE = 64;
enum { MODE_HASH = 0, MODE_COLS = 1, MODE_CHECK = 2 };

struct LiftArgs {
    const unsigned short* step;      // [256, S + 1]
    const unsigned char* blob;
    const int32_t* offsets;          // [T + 1]
    long blob_bytes;
    int T, S;
    int n;                           // items: T (hash, check) or the length of ids (cols)
    int logw;                        // W = 1 << logw lanes per token
    const int32_t* ids;              // cols: [n]
    unsigned long long* hashes;      // hash: [T, 2]
    unsigned char* alive;            // hash: [T]
    int32_t* cols;                   // cols: [n, S]
    const int32_t* reps;             // check: [C, S]
    const int32_t* group;            // check: [T]
    int C;
    unsigned char* mismatch;         // check: [T]
};

__device__ __forceinline__ unsigned long long mix(unsigned s, unsigned e, unsigned long long k1, unsigned long long k2) {
    unsigned long long x = (((unsigned long long)s << 32) | e) + k1;
    x ^= x >> 30; x *= k2;
    x ^= x >> 27; x *= k1 | 1ull;
    x ^= x >> 31;
    return x;
}

template <int MODE, int K>
__global__ __launch_bounds__(GL_THREADS) void guide_lift_kernel(const LiftArgs a) {
    const int lane = threadIdx.x & (GL_WAVE - 1);
    const long wave = (long)blockIdx.x * (GL_THREADS / GL_WAVE) + (threadIdx.x >> 6);
    const int W = 1 << a.logw, s_lo = lane & (W - 1), S = a.S;
    const long item = (wave << (6 - a.logw)) + (lane >> a.logw);
    const bool have = item < (long)a.n;
    int tok = -1;
    if (have) tok = MODE == MODE_COLS ? a.ids[item] : (int)item;
    if (tok < 0 || tok >= a.T) tok = -1;
    int grp = -1;
    if (MODE == MODE_CHECK && tok >= 0) grp = a.group[tok];
    long beg = 0;
    int len = 0;
    if (tok >= 0 && (MODE != MODE_CHECK || grp >= 0)) {
        const long b0 = a.offsets[tok], b1 = a.offsets[tok + 1];
        if (b0 >= 0 && b1 >= b0 && b1 <= a.blob_bytes) { beg = b0; len = (int)(b1 - b0); }
    }
    const unsigned char* bytes = a.blob + beg;
    const int row = S + 1;

    unsigned long long h1 = 0, h2 = 0;
    int any = 0, bad = 0;
    for (int s0 = s_lo; s0 < S; s0 += GL_WAVE * K) {                // (W < 64: S <= W, one pass, K = 1)
        int cur[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int s = s0 + GL_WAVE * k;
            cur[k] = s < S ? s : S;                                // beyond S: the dead state, which stays where it is
        }
        unsigned c = len > 0 ? bytes[0] : 0u;
        for (int p = 0; p < len; ++p) {
            const unsigned short* r = a.step + c * row;
            if (p + 1 < len) c = bytes[p + 1];                     // the next byte is on its way while the gathers run
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int nx = r[cur[k]];
                cur[k] = nx < S ? nx : S;
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int s = s0 + GL_WAVE * k;
            if (s >= S) continue;
            const int e = len > 0 ? cur[k] : S;                    // an empty token is dead from every state
            if (MODE == MODE_HASH) {
                h1 += mix((unsigned)s, (unsigned)e, 0x9E3779B97F4A7C15ull, 0xBF58476D1CE4E5B9ull);
                h2 += mix((unsigned)e, (unsigned)s, 0xD6E8FEB86659FD93ull, 0x94D049BB133111EBull);
                any |= e < S;
            } else if (MODE == MODE_COLS) {
                if (have) a.cols[item * S + s] = e < S ? e : -1;
            } else if (grp >= 0) {
                bad |= grp >= a.C || a.reps[(long)grp * S + s] != (e < S ? e : -1);
            }
        }
    }
    if (MODE == MODE_COLS) return;

    // ---- across the token's W lanes (lanes without a state or a token hold zeros)
    for (int d = 1; d < W; d <<= 1) {
        if (MODE == MODE_HASH) {
            h1 += __shfl_xor(h1, d);
            h2 += __shfl_xor(h2, d);
            any |= __shfl_xor(any, d);
        } else {
            bad |= __shfl_xor(bad, d);
        }
    }
    if (!have || s_lo != 0) return;
    if (MODE == MODE_HASH) {
        a.hashes[2 * item] = h1;
        a.hashes[2 * item + 1] = h2;
        a.alive[item] = (unsigned char)(any != 0);
    } else {
        a.mismatch[item] = (unsigned char)(bad != 0);
    }
}

int lift_check(const char* what, const void* step, const void* blob, const void* offsets, int64_t blob_bytes, int T, int S, int n,
               bool outputs, LiftArgs& a) {
    if (!step || !blob || !offsets || !outputs) LS_FAIL(LS_ERR_INVALID_ARG, "%s: null pointer", what);
    if (S < 1 || S > LS_GUIDE_LIFT_MAX_STATES || T < 1 || n < 1 || blob_bytes < 0)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: S=%d (1..%d) T=%d n=%d (>= 1) blob_bytes=%ld (>= 0)", what, S, LS_GUIDE_LIFT_MAX_STATES, T, n,
                (long)blob_bytes);
    a = LiftArgs{};
    a.step = static_cast<const unsigned short*>(step);
    a.blob = static_cast<const unsigned char*>(blob);
    a.offsets = static_cast<const int32_t*>(offsets);
    a.blob_bytes = (long)blob_bytes; a.T = T; a.S = S; a.n = n;
    a.logw = 0;
    while ((1 << a.logw) < S && a.logw < 6) ++a.logw;
    return LS_OK;
}

template <int MODE>
int lift_launch(const char* name, const LiftArgs& a, void* stream) {
    const long per_wave = 64 >> a.logw, waves = ((long)a.n + per_wave - 1) / per_wave;
    const dim3 grid((unsigned)((waves + GL_THREADS / GL_WAVE - 1) / (GL_THREADS / GL_WAVE))), block(GL_THREADS);
    if (a.S <= 2 * GL_WAVE)
        hipLaunchKernelGGL((guide_lift_kernel<MODE, 1>), grid, block, 0, static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL((guide_lift_kernel<MODE, 4>), grid, block, 0, static_cast<hipStream_t>(stream), a);
    LS_CHECK_LAUNCH(name);
    return LS_OK;
}

}  // namespace

extern "C" {

int ls_guide_lift_hash(const void* step, const void* blob, const int32_t* offsets, int64_t blob_bytes, int T, int S, uint64_t* hashes,
                       uint8_t* alive, void* stream) {
    LiftArgs a;
    if (int rc = lift_check("ls_guide_lift_hash", step, blob, offsets, blob_bytes, T, S, T, hashes && alive, a)) return rc;
    a.hashes = reinterpret_cast<unsigned long long*>(hashes); a.alive = alive;
    return lift_launch<MODE_HASH>("guide_lift_kernel (hash)", a, stream);
}

int ls_guide_lift_cols(const void* step, const void* blob, const int32_t* offsets, int64_t blob_bytes, int T, int S, const int32_t* ids,
                       int n, int32_t* cols, void* stream) {
    LiftArgs a;
    if (int rc = lift_check("ls_guide_lift_cols", step, blob, offsets, blob_bytes, T, S, n, ids && cols, a)) return rc;
    a.ids = ids; a.cols = cols;
    return lift_launch<MODE_COLS>("guide_lift_kernel (cols)", a, stream);
}

int ls_guide_lift_check(const void* step, const void* blob, const int32_t* offsets, int64_t blob_bytes, int T, int S, const int32_t* reps,
                        int C, const int32_t* group, uint8_t* mismatch, void* stream) {
    LiftArgs a;
    if (int rc = lift_check("ls_guide_lift_check", step, blob, offsets, blob_bytes, T, S, T, reps && group && mismatch, a)) return rc;
    if (C < 1) LS_FAIL(LS_ERR_INVALID_ARG, "ls_guide_lift_check: C=%d (>= 1)", C);
    a.reps = reps; a.C = C; a.group = group; a.mismatch = mismatch;
    return lift_launch<MODE_CHECK>("guide_lift_kernel (check)", a, stream);
}

}  // extern "C"
