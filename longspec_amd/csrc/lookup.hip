// lookup.hip -- the drafter of prompt-lookup (n-gram) speculation (lookup_generate; gfx950 / CDNA4): propose what followed the
// most recent earlier occurrence of the text's last few tokens.  No weights, no floating point.
//
// The text of batch row z is T = prompt_ids[z, :il] ++ output_ids[z, :w] with il = input_len[z] (clamped to the prompt's columns)
// and w = cache_lens[z] - input_len[z] + 1 (clamped to the output's columns), L = il + w tokens.  For an end e in 1 .. L-1, m(e)
// is the largest k <= min(max_ngram, e) with T[e-k:e] == T[L-k:L]; the winner has the largest m >= min_ngram, then the largest e.
//
// ngram_match_kernel  (chunks of NGRAM_CHUNK ends, rows) workgroups.  A workgroup keeps the row's last max_ngram tokens in LDS; a
//                     lane takes NG_PER ends, NG_THREADS apart (consecutive lanes read consecutive tokens), loads T[e-1] for all
//                     of them first, and only where that equals the last token walks backwards to m(e): ONE pass over the text
//                     gives the longest match at every end.  key = (m << 32) | e where m >= min_ngram, else 0; the workgroup's
//                     maximum is one 64-bit record per (row, chunk) in the workspace.  A chunk wholly at or behind L writes 0.
// ngram_draft_kernel  one wave per row: the maximum over the row's records, then lane i < gamma writes the draft
//                     d[i] = T[e + i mod (L - e)] (the continuation, read on into the draft itself where it reaches the end of
//                     the text) to spec_buffer[z, 1 + i]; no candidate: T[L-1].  Lane 0 writes info[z] = (n, e) and hist[z, n] += 1.
// Every record is rewritten by every call and nothing is counted with atomics, so the pair replays from a captured graph.  Every
// index is clamped before use: a prompt read is below min(il, prompt columns), an output read below min(w, output columns), and a
// text longer than the host's bound only loses its most recent ends.
#include "lookup_text.h"

namespace {

constexpr int NG_THREADS = 256;
constexpr int NG_PER = 4;
constexpr int NG_CHUNK = NG_THREADS * NG_PER;
constexpr int NG_MAX_N = 8, NG_MAX_GAMMA = 15;
static_assert(NG_CHUNK == LS_NGRAM_CHUNK, "chunk of candidate ends");

struct NgramArgs {
    const int64_t* prompt;   // [b, prompt_cols], row stride prompt_sb
    long prompt_sb;
    int prompt_cols;
    const int32_t* input_len;
    const int64_t* out;      // [b, out_cap], row stride out_sb
    long out_sb;
    int out_cap;
    const int32_t* cache_lens;
    int nchunks;             // records per row (from the host's bound of L)
    int gamma, max_ngram, min_ngram;
    int64_t* spec;           // [b, gamma + 1] dense
    int32_t* info;           // [b, 2]
    int64_t* hist;           // [b, max_ngram + 1] dense; may be null
    unsigned long long* rec; // [b, nchunks]
};

__device__ __forceinline__ Text text_of(const NgramArgs& a, int z) {
    const long il_raw = a.input_len[z];
    return text_from(a.prompt + (long)z * a.prompt_sb, a.prompt_cols, a.out + (long)z * a.out_sb, a.out_cap, il_raw,
                     (long)a.cache_lens[z] - il_raw + 1);
}

__global__ __launch_bounds__(NG_THREADS) void ngram_match_kernel(NgramArgs a) {
    __shared__ int64_t suf[NG_MAX_N];                              // suf[j] = T[L-1-j]
    __shared__ unsigned long long part[NG_THREADS / NG_WAVE];
    const int chunk = blockIdx.x, z = blockIdx.y, tid = threadIdx.x;
    const Text t = text_of(a, z);
    const int L = t.L;
    const long base = (long)chunk * NG_CHUNK;
    unsigned long long* rec = a.rec + (long)z * a.nchunks + chunk;
    if (base >= L) {                                               // (uniform over the workgroup)
        if (tid == 0) *rec = 0ull;
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
    unsigned long long best = 0ull;
#pragma unroll
    for (int k = 0; k < NG_PER; ++k) {
        const long e64 = base + tid + k * NG_THREADS;
        if (e64 < 1 || e64 >= L || last[k] != s0) continue;
        const int e = (int)e64;
        const int cap = e < a.max_ngram ? e : a.max_ngram;         // k <= min(max_ngram, e) <= L - 1: suf[j] is loaded for j < cap
        int m = 1;
        while (m < cap && t.at(e - 1 - m) == suf[m]) ++m;
        if (m >= a.min_ngram) {
            const unsigned long long key = ((unsigned long long)m << 32) | (unsigned)e;
            best = key > best ? key : best;
        }
    }
    best = wave_max(best);
    if ((tid & (NG_WAVE - 1)) == 0) part[tid / NG_WAVE] = best;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int i = 1; i < NG_THREADS / NG_WAVE; ++i) best = part[i] > best ? part[i] : best;
        *rec = best;
    }
}

__global__ __launch_bounds__(NG_WAVE) void ngram_draft_kernel(NgramArgs a) {
    const int z = blockIdx.x, lane = threadIdx.x;
    const Text t = text_of(a, z);
    const int L = t.L;
    const unsigned long long* rec = a.rec + (long)z * a.nchunks;
    unsigned long long best = 0ull;
    for (int c = lane; c < a.nchunks; c += NG_WAVE) best = rec[c] > best ? rec[c] : best;
    best = wave_max(best);
    int n = (int)(best >> 32), e = (int)(best & 0xffffffffull);
    if (n < 1 || n > a.max_ngram || e < 1 || e >= L) {             // no candidate (or a record no call of this shape wrote)
        n = 0;
        e = -1;
    }
    if (lane < a.gamma) {
        int64_t d = 0;
        if (n > 0) d = t.at(e + lane % (L - e));                   // e <= e + i mod (L - e) <= L - 1
        else if (L >= 1) d = t.at(L - 1);
        a.spec[(long)z * (a.gamma + 1) + 1 + lane] = d;
    }
    if (lane == 0) {
        a.info[2 * z] = n;
        a.info[2 * z + 1] = e;
        if (a.hist) a.hist[(long)z * (a.max_ngram + 1) + n] += 1;  // one writer per row
    }
}

int chunks_of(int64_t len_bound) { return (int)((len_bound + NG_CHUNK - 1) / NG_CHUNK); }

}  // namespace

extern "C" {

size_t ls_ngram_workspace_bytes(int b, int64_t len_bound) {
    if (b < 1 || len_bound < 1 || len_bound > (1ll << 31) - 2) return 0;
    return (size_t)b * (size_t)chunks_of(len_bound) * sizeof(unsigned long long);
}

int ls_ngram_draft(const int64_t* prompt_ids, int64_t prompt_stride_b, int prompt_cols, const int32_t* input_len,
                   const int64_t* output_ids, int64_t out_stride_b, int out_cap, const int32_t* cache_lens, int b, int64_t len_bound,
                   int gamma, int max_ngram, int min_ngram, int64_t* spec_buffer, int32_t* info, int64_t* hist, void* workspace,
                   size_t workspace_bytes, void* stream) {
    const char* what = "ls_ngram_draft";
    if (!prompt_ids || !input_len || !output_ids || !cache_lens || !spec_buffer || !info || !workspace)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: null pointer", what);
    if (b < 1 || b > 65535 || prompt_cols < 1 || prompt_cols >= (1 << 30) || out_cap < 1 || out_cap >= (1 << 30) ||
        prompt_stride_b < prompt_cols || out_stride_b < out_cap)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: b=%d prompt columns %d (row stride %ld) output columns %d (row stride %ld)", what, b, prompt_cols,
                (long)prompt_stride_b, out_cap, (long)out_stride_b);
    if (len_bound < 1 || len_bound > (1ll << 31) - 2) LS_FAIL(LS_ERR_INVALID_ARG, "%s: length bound %ld", what, (long)len_bound);
    if (gamma < 1 || gamma > NG_MAX_GAMMA || max_ngram < 1 || max_ngram > NG_MAX_N || min_ngram < 1 || min_ngram > max_ngram)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: gamma=%d (1..%d) max_ngram=%d (1..%d) min_ngram=%d (1..max_ngram)", what, gamma, NG_MAX_GAMMA,
                max_ngram, NG_MAX_N, min_ngram);
    if ((reinterpret_cast<uintptr_t>(prompt_ids) | reinterpret_cast<uintptr_t>(output_ids) | reinterpret_cast<uintptr_t>(spec_buffer) |
         reinterpret_cast<uintptr_t>(hist) | reinterpret_cast<uintptr_t>(workspace)) % 8 != 0 || reinterpret_cast<uintptr_t>(info) % 4 != 0)
        LS_FAIL(LS_ERR_INVALID_ARG, "%s: misaligned pointer", what);
    if (workspace_bytes < ls_ngram_workspace_bytes(b, len_bound))
        LS_FAIL(LS_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, ls_ngram_workspace_bytes(b, len_bound));
    NgramArgs a;
    a.prompt = prompt_ids; a.prompt_sb = (long)prompt_stride_b; a.prompt_cols = prompt_cols; a.input_len = input_len;
    a.out = output_ids; a.out_sb = (long)out_stride_b; a.out_cap = out_cap; a.cache_lens = cache_lens;
    a.nchunks = chunks_of(len_bound);
    a.gamma = gamma; a.max_ngram = max_ngram; a.min_ngram = min_ngram;
    a.spec = spec_buffer; a.info = info; a.hist = hist; a.rec = static_cast<unsigned long long*>(workspace);
    hipLaunchKernelGGL(ngram_match_kernel, dim3(a.nchunks, b), dim3(NG_THREADS), 0, static_cast<hipStream_t>(stream), a);
    LS_CHECK_LAUNCH("ngram_match_kernel");
    hipLaunchKernelGGL(ngram_draft_kernel, dim3(b), dim3(NG_WAVE), 0, static_cast<hipStream_t>(stream), a);
    LS_CHECK_LAUNCH("ngram_draft_kernel");
    return LS_OK;
}

}  // extern "C"
