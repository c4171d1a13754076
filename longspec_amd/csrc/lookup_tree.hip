// lookup_tree.hip -- the tree drafter of prompt-lookup speculation (lookup_generate(branches=B); gfx950 / CDNA4): up to B distinct
// continuations of earlier occurrences of the text's last few tokens, laid out as a level-major tree for ONE verification pass.
// No weights, no floating point.
//
// The text of batch row z is T = prompt_ids[z, :il] ++ output_ids[z, :w] with il = input_len[z] (clamped to the prompt's columns)
// and w = written[z] (clamped to the output's columns), L = il + w.  m(e), the candidates and their key (m << 32) | e are those of
// lookup.hip.  The LS_NGRAM_TOP = 8 candidates with the largest keys are walked in descending order; one is kept when its
// gamma-token continuation c_e[i] = T[e + i mod (L - e)] differs from every kept one, until B are kept (nb of them).  Slot j < nb
// is kept candidate j, a slot >= nb copies slot 0; without a candidate every slot is T[L-1] repeated.  Node 1 + (d-1)*B + j of the
// tree (F = 1 + B*gamma nodes, the root first) is depth d = 1..gamma of branch j.
//
// ngram_tree_match_kernel  (chunks of NG_CHUNK ends, rows) workgroups: the one-pass walk of ngram_match_kernel, then the
//                          workgroup's NG_TOP largest keys in descending order, zero padded -- NG_TOP rounds of "the maximum below
//                          the previous one", exact because e makes every key unique -- as NG_TOP records per (row, chunk).  A
//                          chunk wholly at or behind L writes zeros.
// ngram_tree_draft_kernel  one wave per row: every lane sorts the records of its chunks into its own NG_TOP largest, NG_TOP wave
//                          maxima pop the row's; lane i < gamma loads token i of the NG_TOP continuations; one OR over those
//                          lanes of "q and r differ here" feeds the distinctness walk; then all_spec[z, 1:], the mask rows 1..
//                          (tree_commit resets the mask every round), info and the two histograms.
// Every record and every output is rewritten by every call and nothing is counted with atomics, so the pair replays from a
// captured graph.  Every index is clamped before use, as in lookup.hip: a text longer than the host's bound only loses its most
// recent ends.
#include "lookup_text.h"

namespace {

constexpr int NG_THREADS = 256;
constexpr int NG_PER = 4;
constexpr int NG_CHUNK = NG_THREADS * NG_PER;
constexpr int NG_MAX_N = 8, NG_MAX_GAMMA = 15;
constexpr int NG_TOP = LS_NGRAM_TOP;
static_assert(NG_CHUNK == LS_NGRAM_CHUNK, "chunk of candidate ends");
static_assert(NG_TOP == 8, "the draft kernel names its candidates one by one");

struct NgramTreeArgs {
    const int64_t* prompt;   // [b, prompt_cols], row stride prompt_sb
    long prompt_sb;
    int prompt_cols;
    const int32_t* input_len;
    const int64_t* out;      // [b, out_cap], row stride out_sb
    long out_sb;
    int out_cap;
    const int32_t* written;  // [b]: output columns that are text
    int nchunks;             // chunks per row (from the host's bound of L)
    int gamma, branches, max_ngram, min_ngram;
    int64_t* spec;           // [b, F] dense, F = 1 + branches * gamma
    int64_t* mask;           // [b, F, F] dense
    int32_t* info;           // [b, branches, 2]
    int64_t* hist;           // [b, max_ngram + 1] dense; may be null
    int64_t* hist_nb;        // [b, branches + 1] dense; may be null
    unsigned long long* rec; // [b, nchunks, NG_TOP]
};

__device__ __forceinline__ Text text_of(const NgramTreeArgs& a, int z) {
    return text_from(a.prompt + (long)z * a.prompt_sb, a.prompt_cols, a.out + (long)z * a.out_sb, a.out_cap, a.input_len[z],
                     a.written[z]);
}

__global__ __launch_bounds__(NG_THREADS) void ngram_tree_match_kernel(NgramTreeArgs a) {
    __shared__ int64_t suf[NG_MAX_N];                              // suf[j] = T[L-1-j]
    __shared__ unsigned long long part[2][NG_THREADS / NG_WAVE];
    const int chunk = blockIdx.x, z = blockIdx.y, tid = threadIdx.x;
    const Text t = text_of(a, z);
    const int L = t.L;
    const long base = (long)chunk * NG_CHUNK;
    unsigned long long* rec = a.rec + ((long)z * a.nchunks + chunk) * NG_TOP;
    if (base >= L) {                                               // (uniform over the workgroup)
        if (tid < NG_TOP) rec[tid] = 0ull;
        return;
    }
    if (tid < a.max_ngram && tid < L) suf[tid] = t.at(L - 1 - tid);
    __syncthreads();
    int64_t last[NG_PER];
#pragma unroll
    for (int k = 0; k < NG_PER; ++k) {
        const long e = base + tid + k * NG_THREADS;                // the end; T[e-1] is its last token
        last[k] = e >= 1 && e < L ? t.at((int)e - 1) : 0;
    }
    const int64_t s0 = suf[0];
    unsigned long long key[NG_PER];
#pragma unroll
    for (int k = 0; k < NG_PER; ++k) {
        key[k] = 0ull;
        const long e64 = base + tid + k * NG_THREADS;
        if (e64 < 1 || e64 >= L || last[k] != s0) continue;
        const int e = (int)e64;
        const int cap = e < a.max_ngram ? e : a.max_ngram;         // k <= min(max_ngram, e) <= L - 1: suf[j] is loaded for j < cap
        int m = 1;
        while (m < cap && t.at(e - 1 - m) == suf[m]) ++m;
        if (m >= a.min_ngram) key[k] = ((unsigned long long)m << 32) | (unsigned)e;
    }
    // round r: the largest key below round r-1's.  part[] is double-buffered: one barrier per round
    unsigned long long prev = ~0ull;
#pragma unroll 1
    for (int r = 0; r < NG_TOP; ++r) {
        unsigned long long best = 0ull;
#pragma unroll
        for (int k = 0; k < NG_PER; ++k) best = key[k] < prev && key[k] > best ? key[k] : best;
        best = wave_max(best);
        if ((tid & (NG_WAVE - 1)) == 0) part[r & 1][tid / NG_WAVE] = best;
        __syncthreads();
        best = part[r & 1][0];
#pragma unroll
        for (int i = 1; i < NG_THREADS / NG_WAVE; ++i) best = part[r & 1][i] > best ? part[r & 1][i] : best;
        if (tid == 0) rec[r] = best;
        if (best == 0ull) {                                        // (uniform: read from LDS) nothing is left
            if (tid > r && tid < NG_TOP) rec[tid] = 0ull;
            return;
        }
        prev = best;
    }
}

// v into the descending list top[0..NG_TOP)
#define NG_INSERT(v)                                                  \
    do {                                                              \
        unsigned long long x_ = (v);                                  \
        _Pragma("unroll") for (int i_ = 0; i_ < NG_TOP; ++i_) {       \
            const unsigned long long hi_ = x_ > top[i_] ? x_ : top[i_]; \
            x_ = x_ > top[i_] ? top[i_] : x_;                         \
            top[i_] = hi_;                                            \
        }                                                             \
    } while (0)

__global__ __launch_bounds__(NG_WAVE) void ngram_tree_draft_kernel(NgramTreeArgs a) {
    const int z = blockIdx.x, lane = threadIdx.x;
    const Text t = text_of(a, z);
    const int L = t.L, gamma = a.gamma, B = a.branches, F = 1 + B * gamma;
    const unsigned long long* rec = a.rec + (long)z * a.nchunks * NG_TOP;
    // this lane's NG_TOP largest records, descending
    unsigned long long top[NG_TOP];
#pragma unroll
    for (int i = 0; i < NG_TOP; ++i) top[i] = 0ull;
    for (int c = lane; c < a.nchunks; c += NG_WAVE) {
        unsigned long long v[NG_TOP];
#pragma unroll
        for (int i = 0; i < NG_TOP; ++i) v[i] = rec[(long)c * NG_TOP + i];
        if (v[0] == 0ull) continue;                                // (a chunk's records are descending)
#pragma unroll
        for (int i = 0; i < NG_TOP; ++i) NG_INSERT(v[i]);
    }
    // the row's NG_TOP largest: the wave's maximum pops the head of the lane that holds it (keys of a row are unique)
    int cn[NG_TOP], ce[NG_TOP];
    bool ok = true;                                                // candidates are valid up to the first that is not
#pragma unroll
    for (int r = 0; r < NG_TOP; ++r) {
        const unsigned long long best = wave_max(top[0]);
        if (best != 0ull && top[0] == best) {
#pragma unroll
            for (int i = 0; i + 1 < NG_TOP; ++i) top[i] = top[i + 1];
            top[NG_TOP - 1] = 0ull;
        }
        const int n = (int)(best >> 32), e = (int)(best & 0xffffffffull);
        ok = ok && n >= 1 && n <= a.max_ngram && e >= 1 && e < L;  // else: none (or a record no call of this shape wrote)
        cn[r] = ok ? n : 0;
        ce[r] = ok ? e : -1;
    }
    // token `lane` of every continuation; without a candidate, of the fallback T[L-1] repeated
    int64_t c[NG_TOP];
    const bool mine = lane < gamma;
#pragma unroll
    for (int r = 0; r < NG_TOP; ++r) {
        c[r] = 0;
        if (mine && cn[r] > 0) c[r] = t.at(ce[r] + lane % (L - ce[r]));      // e <= e + i mod (L - e) <= L - 1
    }
    if (mine && cn[0] == 0 && L >= 1) c[0] = t.at(L - 1);
    // the distinctness walk: candidate r is kept when it differs from every kept q < r, until B are kept.  Bit r*(r-1)/2 + q of
    // `diff`: continuations q < r differ in some token (one OR over the wave's lanes < gamma)
    unsigned diff = 0u;
#pragma unroll
    for (int r = 1; r < NG_TOP; ++r)
#pragma unroll
        for (int q = 0; q < r; ++q) diff |= mine && c[r] != c[q] ? 1u << (r * (r - 1) / 2 + q) : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) diff |= __shfl_xor(diff, off, NG_WAVE);
    unsigned kept = 0u;
    int nb = 0;
#pragma unroll
    for (int r = 0; r < NG_TOP; ++r) {
        bool dup = false;
#pragma unroll
        for (int q = 0; q < r; ++q) dup = dup || (((kept >> q) & 1u) && !((diff >> (r * (r - 1) / 2 + q)) & 1u));
        if (cn[r] > 0 && nb < B && !dup) {
            kept |= 1u << r;
            ++nb;
        }
    }
    // slots: kept candidate r is slot popcount(kept below r); the rest copy slot 0 (candidate 0, or the fallback)
    int64_t* spec = a.spec + (long)z * F;
    int32_t* info = a.info + (long)z * B * 2;
#pragma unroll
    for (int r = 0; r < NG_TOP; ++r) {
        if (!((kept >> r) & 1u)) continue;
        const int j = __popc(kept & ((1u << r) - 1u));             // < nb <= B
        if (mine) spec[1 + lane * B + j] = c[r];
        if (lane == 0) {
            info[2 * j] = cn[r];
            info[2 * j + 1] = ce[r];
        }
    }
    for (int j = nb; j < B; ++j) {
        if (mine) spec[1 + lane * B + j] = c[0];
        if (lane == 0) {
            info[2 * j] = 0;
            info[2 * j + 1] = -1;
        }
    }
    // mask rows 1 .. F-1: the root column and the nodes of the row's branch at depths <= its own
    int64_t* mask = a.mask + (long)z * F * F;
    for (int col = lane; col < F; col += NG_WAVE) {
        const int cj = col >= 1 ? (col - 1) % B : -1, cd = col >= 1 ? (col - 1) / B : -1;
        int rj = 0, rd = 0;                                        // branch and depth - 1 of the row
        for (int row = 1; row < F; ++row) {
            mask[(long)row * F + col] = col == 0 || (cj == rj && cd <= rd) ? 1 : 0;
            if (++rj == B) {
                rj = 0;
                ++rd;
            }
        }
    }
    if (lane == 0) {                                               // one writer per row
        if (a.hist) a.hist[(long)z * (a.max_ngram + 1) + cn[0]] += 1;
        if (a.hist_nb) a.hist_nb[(long)z * (B + 1) + nb] += 1;
    }
}

int chunks_of(int64_t len_bound) { return (int)((len_bound + NG_CHUNK - 1) / NG_CHUNK); }

}  // namespace

extern "C" {

size_t ls_ngram_tree_workspace_bytes(int b, int64_t len_bound) {
    if (b < 1 || len_bound < 1 || len_bound > (1ll << 31) - 2) return 0;
    return (size_t)b * (size_t)chunks_of(len_bound) * NG_TOP * sizeof(unsigned long long);
}

int ls_ngram_tree_draft(const int64_t* prompt_ids, int64_t prompt_stride_b, int prompt_cols, const int32_t* input_len,
                        const int64_t* output_ids, int64_t out_stride_b, int out_cap, const int32_t* written, int b, int64_t len_bound,
                        int gamma, int branches, int max_ngram, int min_ngram, int64_t* all_spec, int64_t* tree_mask, int32_t* info,
                        int64_t* hist, int64_t* hist_nb, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "ls_ngram_tree_draft";
    if (!prompt_ids || !input_len || !output_ids || !written || !all_spec || !tree_mask || !info || !workspace)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: null pointer", what);
    if (b < 1 || b > 65535 || prompt_cols < 1 || prompt_cols >= (1 << 30) || out_cap < 1 || out_cap >= (1 << 30) ||
        prompt_stride_b < prompt_cols || out_stride_b < out_cap)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: b=%d prompt columns %d (row stride %ld) output columns %d (row stride %ld)", what, b, prompt_cols,
                (long)prompt_stride_b, out_cap, (long)out_stride_b);
    if (len_bound < 1 || len_bound > (1ll << 31) - 2) LS_FAIL(LS_ERR_INVALID_ARG, "%s: length bound %ld", what, (long)len_bound);
    if (gamma < 1 || gamma > NG_MAX_GAMMA || branches < 1 || branches > NG_TOP || max_ngram < 1 || max_ngram > NG_MAX_N ||
        min_ngram < 1 || min_ngram > max_ngram)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: gamma=%d (1..%d) branches=%d (1..%d) max_ngram=%d (1..%d) min_ngram=%d (1..max_ngram)", what,
                gamma, NG_MAX_GAMMA, branches, NG_TOP, max_ngram, NG_MAX_N, min_ngram);
    if ((reinterpret_cast<uintptr_t>(prompt_ids) | reinterpret_cast<uintptr_t>(output_ids) | reinterpret_cast<uintptr_t>(all_spec) |
         reinterpret_cast<uintptr_t>(tree_mask) | reinterpret_cast<uintptr_t>(hist) | reinterpret_cast<uintptr_t>(hist_nb) |
         reinterpret_cast<uintptr_t>(workspace)) % 8 != 0 || reinterpret_cast<uintptr_t>(info) % 4 != 0)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: misaligned pointer", what);
    if (workspace_bytes < ls_ngram_tree_workspace_bytes(b, len_bound))
        LS_FAIL(LS_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes,
                ls_ngram_tree_workspace_bytes(b, len_bound));
    NgramTreeArgs a;
    a.prompt = prompt_ids; a.prompt_sb = (long)prompt_stride_b; a.prompt_cols = prompt_cols; a.input_len = input_len;
    a.out = output_ids; a.out_sb = (long)out_stride_b; a.out_cap = out_cap; a.written = written;
    a.nchunks = chunks_of(len_bound);
    a.gamma = gamma; a.branches = branches; a.max_ngram = max_ngram; a.min_ngram = min_ngram;
    a.spec = all_spec; a.mask = tree_mask; a.info = info; a.hist = hist; a.hist_nb = hist_nb;
    a.rec = static_cast<unsigned long long*>(workspace);
    hipLaunchKernelGGL(ngram_tree_match_kernel, dim3(a.nchunks, b), dim3(NG_THREADS), 0, static_cast<hipStream_t>(stream), a);
    LS_CHECK_LAUNCH("ngram_tree_match_kernel");
    hipLaunchKernelGGL(ngram_tree_draft_kernel, dim3(b), dim3(NG_WAVE), 0, static_cast<hipStream_t>(stream), a);
    LS_CHECK_LAUNCH("ngram_tree_draft_kernel");
    return LS_OK;
}

}  // extern "C"
