/*
 * longspec_hip.h -- C ABI of liblongspec_hip.so: MI355X (gfx950) kernels for the
 * draft-then-verify decode round of LongSpec.
 *
 * The reference (sail-sg/LongSpec) has no FFI layer of its own; its operator
 * seams on this path are Python callables.  Each entry point below
 * replaces one of those seams and cites it (paths relative to the reference
 * root).  Conventions: extern "C"; raw DEVICE pointers + explicit dims/strides
 * (in elements); caller-allocated outputs and workspace (size-query functions);
 * every launch is stream-ordered on `stream` (a hipStream_t passed as void*);
 * no host synchronisation, no allocation, no hidden global state except the
 * thread-local last-error string.  Return value: 0 = ok, negative = LS_ERR_*.
 * Sequence lengths live on the DEVICE (int32), as in the reference
 * (`cache_seqlens=cache_lens`); `kv_len_hint` is a host-side upper bound used
 * only to size the launch grid.
 *
 * dtype: LS_F16 (the reference hard-codes fp16, longspec/test/llama_glide.py:474)
 * or LS_BF16.  head_dim must be 128 (longspec/test/llama.py:95).
 */
#ifndef LONGSPEC_HIP_H
#define LONGSPEC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LS_OK 0
#define LS_ERR_INVALID_ARG (-1)
#define LS_ERR_UNSUPPORTED (-2)
#define LS_ERR_WORKSPACE (-3)
#define LS_ERR_LAUNCH (-4)

#define LS_F16 0
#define LS_BF16 1

/* how the "new key block" (tree / appended tokens) is computed and merged */
#define LS_NEW_NONE 0   /* prefix only                                                         */
#define LS_NEW_FLASH 1  /* flash_attn_with_kvcache(k=,v=) semantics: ONE softmax over prefix+new */
#define LS_NEW_TARGET 2 /* LlamaAttention.tree_part_fwd + fp16 merge  (llama.py:387,394-421)    */
#define LS_NEW_DRAFT 3  /* triton_tree_attn._fwd_kernel + fp32 merge  (llama_glide.py:300-329)  */

typedef struct ls_attn_desc {
    /* tensors (device) */
    const void* q;      /* [b, sq, H, 128]                     q_stride_{b,s,h}                  */
    void* k_cache;      /* [b, S, Hkv, 128]  read; written when scatter_new != 0                  */
    void* v_cache;      /*                                      kc_stride_{b,s,h} (shared by K,V) */
    const void* k_new;  /* [b, n_new_rows, Hkv, 128] or NULL    kn_stride_{b,s,h}                 */
    const void* v_new;
    const int32_t* cache_seqlens; /* [b] valid prefix rows L (device)                             */
    const uint32_t* mask_bits;    /* [b, sq, mask_words] bit j of row r = new-block key j visible */
    void* out;          /* [b, sq, H, 128] dtype                out_stride_{b,s,h}                */
    float* lse;         /* [b, H, sq] fp32 or NULL: soft-max log-normaliser (NONE/FLASH); the tree   */
                        /* kernel's L in LS_NEW_DRAFT mode; not available in LS_NEW_TARGET mode     */
    void* ev_start;     /* optional hipEvent_t pair recorded on `stream` around the stage-1 kernel  */
    void* ev_stop;      /* (profiling: per-launch duration of the streaming kernel), or NULL        */
    /* dims */
    int32_t b, sq, H, Hkv;
    int32_t dtype;         /* LS_F16 / LS_BF16                                                    */
    int32_t new_mode;      /* LS_NEW_*                                                            */
    int32_t n_new;         /* keys in the new block (0 for LS_NEW_NONE)                           */
    int32_t n_new_cached;  /* leading new-block keys that already sit in the cache at L + j       */
    int32_t mask_words;    /* uint32 words per mask row (>= ceil(n_new/32))                       */
    int32_t scatter_new;   /* write k_new/v_new rows into the caches at L + n_new_cached + i      */
    int32_t causal;        /* prefix: bottom-right causal alignment (flash-attn semantics)        */
    int32_t window_left;   /* prefix: sliding window to the left, -1 = none                       */
    int32_t n_app;         /* keys counted as appended for the bottom-right alignment (sk = L+n_app) */
    int32_t prescale_q;    /* LS_NEW_TARGET: last layer multiplies q by the scale first (G1)      */
    int32_t kv_len_hint;   /* host upper bound of max(cache_seqlens) -- grid sizing only          */
    int32_t n_splits;      /* 0 = choose automatically                                            */
    float softmax_scale;
    int64_t q_stride_b, q_stride_s, q_stride_h;
    int64_t kc_stride_b, kc_stride_s, kc_stride_h;
    int64_t kn_stride_b, kn_stride_s, kn_stride_h;
    int64_t out_stride_b, out_stride_s, out_stride_h;
} ls_attn_desc;

/* ---- library ---------------------------------------------------------------- */
int ls_version(void);
const char* ls_last_error(void);

/* ---- attention (K1..K7) ------------------------------------------------------- */

/* Bytes of scratch an attention call with this descriptor needs (split-KV partials). */
size_t ls_attn_workspace_bytes(const ls_attn_desc* d);

/* Number of prefix partials stage 1 writes for this descriptor (splits x key-slices). */
int ls_attn_num_parts(const ls_attn_desc* d);

/* Name of the stage-1 kernel that serves this descriptor ("attn_verify_kernel", "attn_partial_ws_kernel",
 * "attn_partial_kernel"): what a profiler will show for the call -- diagnostics / benchmark labels only. */
const char* ls_attn_kernel_name(const ls_attn_desc* d);

/* One fused attention call = stage 1 (split-KV partials + new-block part) then
 * stage 2 (log-sum-exp combine + reference-order merge), both on `stream`.
 *  LS_NEW_NONE / LS_NEW_FLASH : flash_attn_with_kvcache as called at
 *      longspec/test/llama.py:324,385 and llama_glide.py:261,265,297,300
 *  LS_NEW_TARGET : LlamaAttention.tree_decoding, llama.py:385-387 + tree_part_fwd :394-421
 *      (prefix flash-decoding + KV scatter + tree-masked part + fp16 merge)   [K1+K2+K3]
 *  LS_NEW_DRAFT  : GlideAttention.tree_decoding self-attn branch, llama_glide.py:300-302
 *      + triton_tree_part_fwd :309-329 (window prefix + Triton tree kernel + fp32 merge) [K5+K6] */
int ls_attn_fwd(const ls_attn_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* Diagnostic: workgroups (key split x kv head) that had to REDO their split since the last reset because a soft-max numerator
 * left the fp16 range of the split's fixed reference (csrc/attn.hip: the reference is the maximum over the split's first 64
 * keys; flash-attn's running maximum, SURVEY App. C, has no such event).  Synchronises the device; not for the decode path.
 * Returns the count (and zeroes it when reset != 0), -1 on a HIP error. */
long ls_attn_redo_count(int reset);

/* Stage 1 only: writes partials into the workspace (multi-GPU path). */
int ls_attn_partial(const ls_attn_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* Combine this rank's prefix partials into ONE normalised partial for the exchange:
 * o32 [b,sq,H,128] fp32, lse [b,H,sq] fp32 (the tree part stays in the workspace). */
int ls_attn_reduce_local(const ls_attn_desc* d, void* workspace, size_t workspace_bytes,
                         float* o32, float* lse, void* stream);

/* Stage 2 with externally gathered prefix partials (fixed rank order => deterministic):
 * parts_o [n_parts][b,sq,H,128] fp32, parts_lse [n_parts][b,H,sq]; the new-block part is
 * taken from `workspace` (written by ls_attn_partial).  N-way generalisation of
 * llama.py:385-387,420. */
int ls_attn_finish(const ls_attn_desc* d, const float* parts_o, const float* parts_lse, int n_parts,
                   int64_t part_o_stride, int64_t part_lse_stride, /* elements between parts; 0 = dense */
                   void* workspace, size_t workspace_bytes, void* stream);

/* N-way log-sum-exp merge of normalised partials (no new block): out [b,sq,H,128] dtype
 * and/or o32 + lse.  Any of out/o32/lse may be NULL. */
int ls_lse_merge(const float* parts_o, const float* parts_lse, int n_parts, int b, int sq, int H,
                 int dtype, void* out, float* o32, float* lse, void* stream);

/* tree_mask int64 [b,M,N] (non-zero = visible; llama_glide.py:984,1082-1085) -> packed
 * uint32 [b,M,words] (bit j%32 of word j/32), zero padded. */
int ls_pack_tree_mask(const int64_t* tree_mask, int b, int M, int N, uint32_t* bits, int words, void* stream);

/* ---- skinny linear layers (weight-streaming GEMM, M <= 80 token rows) ---------------- */

#define LS_EPI_NONE 0     /* y = x W^T (+ bias)                                                     */
#define LS_EPI_SILU_MUL 1 /* y = silu(x Wg^T) * (x Wu^T): w[0] = ls_linear_pack_gate_up(Wg, Wu), n[0] = N */
#define LS_EPI_QKV_ROPE 2 /* q|k|v projection + apply_rotary_pos_emb on q and k (llama.py:375-378): segments 0 and 1
                           * are packed by ls_linear_pack_rope and rotated with rope_cos/rope_sin, segment 2 is plain */

typedef struct ls_linear_desc {
    const void* x;        /* [M, K] dtype, row stride ldx (elements)                                  */
    const void* w[3];     /* weight segments, each [n[i], K] PACKED by ls_linear_pack_weight          */
    const void* bias[3];  /* [n[i]] dtype or NULL                                                     */
    void* y;              /* [M, sum n[i]] dtype, row stride ldy (LS_EPI_SILU_MUL: [M, n[0]])         */
    void* ev_start;       /* optional hipEvent_t pair recorded on `stream` around the kernel, or NULL */
    void* ev_stop;
    int32_t M, K;         /* M <= 80 token rows; K a multiple of 64 (>= 128)                          */
    int32_t n[3];         /* rows of each weight segment (multiples of 128 when n_seg > 1)            */
    int32_t n_seg;        /* 1..3 segments sharing x: q|k|v in one launch                             */
    int32_t dtype;        /* LS_F16 / LS_BF16                                                         */
    int32_t epilogue;     /* LS_EPI_*                                                                 */
    int32_t n_splits;     /* split-K factor, 0 = automatic (a function of N, K only -- never of M)    */
    int64_t ldx, ldy;
    const void* rope_cos; /* LS_EPI_QKV_ROPE: cos / sin [M, 128] dtype of the rows' positions (ls_rope_cos_sin) */
    const void* rope_sin;
    const void* residual; /* LS_EPI_NONE, optional: [M, sum n[i]] dtype (row stride ldr) added to the ROUNDED projection, */
    int64_t ldr;          /* `residual + mlp(x)` of the decoder layers (llama_glide.py:466); NULL = none                  */
    /* LlamaRMSNorm (llama.py:36 / qwen2.py:73-90) folded into the projection that consumes it.  `norm_weight` != NULL: x is
     * the UN-normalised residual stream and the launch multiplies `norm_weight * dtype(x32 * rsqrt(mean(x32^2) + eps))`
     * instead -- bit-identical to ls_rmsnorm_fwd followed by the plain launch.  The rows' sums of squares come as
     * `ssq_parts` fp32 partials per row (one per 64 columns of x, column order), written by the launch that produced x:
     * `ssq_out` != NULL (LS_EPI_NONE, one segment, N % 64 == 0) makes this launch such a producer: [M, N / 64] fp32
     * partial sums of the squares of the values it stores (after bias and residual).                                  */
    const void* norm_weight; /* [K] dtype or NULL                                                                        */
    const float* ssq_in;     /* [M, ssq_parts] fp32                                                                      */
    float* ssq_out;          /* [M, N / 64] fp32 or NULL                                                                 */
    int32_t ssq_parts;
    float norm_eps;
} ls_linear_desc;

/* Weights are streamed in the MFMA A-operand layout: pack each nn.Linear.weight [N, K] (row-major,
 * contiguous) ONCE after loading the checkpoint.  Packed size = ceil(N/64)*64 * K elements; for the
 * 64-row slab g, 32-wide k-step s and 16-row tile t the 1 KB block sits at element offset
 * ((g*(K/32) + s)*4 + t)*512 and holds, for lane l, W[64g + 16t + l%16][32s + 8(l/16) .. +8] at offset
 * 8*l (rows >= N are zero). */
size_t ls_linear_packed_bytes(int N, int K);
int ls_linear_pack_weight(const void* weight, void* packed, int N, int K, int dtype, void* stream);

/* gate_proj and up_proj [N, K] of one MLP packed as ONE matrix of 2N rows (ls_linear_packed_bytes(2N, K))
 * whose 16-row tiles alternate gate, up, gate, up ...: the operand of LS_EPI_SILU_MUL.  N % 16 == 0. */
int ls_linear_pack_gate_up(const void* gate_weight, const void* up_weight, void* packed, int N, int K,
                           int dtype, void* stream);

/* A q_proj / k_proj weight [heads*128, K] for LS_EPI_QKV_ROPE: same block structure, but within every head the
 * 16-row tiles are stored in the order 0,4,1,5,2,6,3,7 so that rows d and d+64 -- a rotary pair -- are finished by
 * the same wave.  The output columns are the plain ones. */
int ls_linear_pack_rope(const void* weight, void* packed, int N, int K, int dtype, void* stream);

/* Bytes of workspace (slab counters + split-K partials).  The workspace must be ZERO-FILLED once
 * before its first use; every call leaves the counter region zero again, so one workspace can serve
 * all launches of a stream. */
size_t ls_linear_workspace_bytes(const ls_linear_desc* d);

/* The projections of a decode pass: q/k/v/o_proj (longspec/test/llama.py:361-363,390;
 * llama_glide.py:248-250,268,285-287,305), LlamaMLP / Qwen2MLP.forward (transformers; vendored
 * qwen2.py:218-230: down_proj(act_fn(gate_proj(x)) * up_proj(x))), lm_head (llama_glide.py:960,1019,
 * 1046,1091).  fp32 accumulation in a fixed k order that does not depend on M; every linear's output
 * is rounded to dtype where nn.Linear rounds it.  LS_ERR_UNSUPPORTED for M > 80 or K % 64 != 0 (those
 * are plain library GEMMs: prefill). */
int ls_linear_fwd(const ls_linear_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* Cache hint for the launch `d` describes (no counterpart in the reference; writes nothing): the same grid requests the
 * first `units` register sets (8 KB each) of every wave's weight stream with the default cache policy, so that they sit in
 * the L2 of the XCD the matching workgroup of ls_linear_fwd(d) runs on.  Issued while a latency-bound kernel (RMSNorm,
 * attention finish) occupies the stream, it takes the HBM ramp off the projection that follows. */
int ls_linear_prefetch(const ls_linear_desc* d, int units, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the same linear layers with 8-bit (OCP e4m3fn) weights -------------------------------------
 *
 * W[n, k] = q[n, k] * scale[n]: one e4m3fn byte per element (gfx950's FP8, not MI300's fnuz) and one fp32 scale per
 * output row.  Activations, bias, accumulation (fp32, MFMA f16/bf16) and every rounding point are those of
 * ls_linear_fwd; only the weight stream is half as long.  No counterpart in the reference (longspec/test keeps 16-bit
 * weights); the seams served are ls_linear_fwd's: llama.py:361-363,390, LlamaMLP.forward (vendored qwen2.py:218-230),
 * llama_glide.py:248-250,268,285-287,305, lm_head at llama_glide.py:960,1019,1046,1091.
 *
 * With power-of-two scales, q * scale is exactly representable in fp16 / bf16 and ls_linear_w8_fwd is BIT-IDENTICAL to
 * ls_linear_fwd on the de-quantised 16-bit weight for the same descriptor (same n_splits): the launch plan and the k order
 * of every row are shared.
 *
 * Packed layout: ceil(N/64)*64 * K bytes; the 1 KB block of (64-row group g, 64-wide k chunk c, 16-row tile t) sits at
 * byte offset ((g*(K/64) + c)*4 + t)*1024 and holds, for lane l, the 8 bytes q[64g + 16t + l%16][64c + 8(l/16) .. +8]
 * at offset 16*l and the 8 bytes q[same row][64c + 32 + 8(l/16) .. +8] at offset 16*l + 8 (rows >= N are zero). */
size_t ls_linear_w8_packed_bytes(int N, int K);

/* Row-wise quantiser: weight [N, K] dtype (row-major, contiguous, K % 8 == 0) -> q [N, K] e4m3fn bytes, scale [N] fp32.
 *   amax = max_k |w[n,k]|;  scale[n] = 2^ceil(log2(amax / 448))  (pow2_scale != 0; exponent arithmetic, exponent >= -120)
 *                           scale[n] = amax / 448                 (pow2_scale == 0);   amax == 0 -> scale = 1
 *   q[n,k] = e4m3fn(w[n,k] / scale[n]), round to nearest even, saturating at +-448 (never the NaN encoding).
 * Bit for bit what longspec_amd/quant.py::quantize_rows_e4m3 computes on the host. */
int ls_linear_w8_quantize(const void* weight, int N, int K, int dtype, int pow2_scale, uint8_t* q, float* scale,
                          void* stream);

/* q [N, K] bytes -> the streamed layout (K % 64 == 0).  q_up != NULL: a gate/up pair of an MLP with alternating 16-row
 * tiles (2N rows, N % 16 == 0: the operand of LS_EPI_SILU_MUL, as ls_linear_pack_gate_up).  rope != 0: the q/k layout
 * of LS_EPI_QKV_ROPE (N = heads x 128, as ls_linear_pack_rope). */
int ls_linear_w8_pack(const uint8_t* q, const uint8_t* q_up, void* packed, int N, int K, int rope, void* stream);

/* As ls_linear_workspace_bytes / ls_linear_fwd with d->w[i] pointing at 8-bit packed segments (d->dtype is the
 * activation / output dtype) and scale[i] the fp32 [n[i]] row scales of segment i, 16-byte aligned (LS_EPI_SILU_MUL:
 * scale[0] = the gate rows', scale[1] = the up rows').  y = round(acc * scale[n] (+ bias[n])), then the epilogue.  The
 * folded RMSNorm fields (norm_weight, ssq_in, ssq_out) are LS_ERR_UNSUPPORTED here, and there is no prefetch call. */
size_t ls_linear_w8_workspace_bytes(const ls_linear_desc* d);
int ls_linear_w8_fwd(const ls_linear_desc* d, const float* const scale[3], void* workspace, size_t workspace_bytes,
                     void* stream);

/* ---- the same linear layers with 4-bit (OCP MX FP4) weights --------------------------------------
 *
 * W[n, k] = e2m1(q[n, k]) * 2^(e[n, k/32] - 127): 4-bit elements {+-0, 0.5, 1, 1.5, 2, 3, 4, 6} (sign, 2 exponent bits, 1
 * mantissa bit), two per byte with the lower k in the low nibble, and one e8m0 scale byte per 32 consecutive k of a row.
 * No counterpart in the reference (longspec/test keeps 16-bit weights); the seams served are ls_linear_fwd's:
 * llama.py:361-363,390, LlamaMLP.forward (vendored qwen2.py:218-230), llama_glide.py:248-250,268,285-287,305, lm_head at
 * llama_glide.py:960,1019,1046,1091.
 * Activations, bias, accumulation (fp32, MFMA f16/bf16) and every rounding point are those of ls_linear_fwd; the nibbles
 * are converted on their way into the MFMA operand (v_cvt_scalef32_pk_{f16,bf16}_fp4) with the block scale as the
 * instruction's scale operand, so no scale is applied behind the sums.  This path takes scale bytes in [114, 140]
 * (2^-13 .. 2^13) only: every non-zero de-quantised value is then a normal fp16 and an exact bf16 number and
 * ls_linear_w4_fwd is BIT-IDENTICAL to ls_linear_fwd on the de-quantised 16-bit weight for the same descriptor (same
 * n_splits): the launch plan and the k order of every row are shared.
 *
 * Packed layout: ceil(N/64) * (K/64) * 2176 bytes; the chunk of (64-row group g, 64-wide k chunk c) sits at byte offset
 * (g*(K/64) + c)*2176 and holds, for tile t = 0..3 and lane l = 0..63, the 4 bytes (8 nibbles)
 * q[64g + 16t + l%16][64c + 8(l/16) .. +8] at 512*t + 8*l and the 4 bytes q[same row][64c + 32 + 8(l/16) .. +8] at
 * 512*t + 8*l + 4, followed at 2048 + 8*r + 2*t + ks by the scale byte e[64g + 16t + r][2c + ks] (r = 0..15, ks = 0, 1).
 * Rows >= N are zero.  0.5 + 1/32 bytes are streamed per weight element.
 */
size_t ls_linear_w4_packed_bytes(int N, int K);

/* Block quantiser: weight [N, K] dtype (row-major, contiguous, K % 32 == 0) -> q [N, K/2] nibble bytes, e [N, K/32] e8m0.
 *   amax = max |w| over the 32-k block;  E = ceil(log2(amax / 6)) by exponent arithmetic, clamped to [-13, 13];
 *   amax == 0 -> E = 0;  e = E + 127;  element = e2m1(w / 2^E), round to nearest, ties to the even mantissa bit, saturating
 *   at +-6, the sign of w kept (a zero magnitude included).
 * Bit for bit what longspec_amd/quant.py::quantize_blocks_mxfp4 computes on the host. */
int ls_linear_w4_quantize(const void* weight, int N, int K, int dtype, uint8_t* q, uint8_t* e, void* stream);

/* (q, e) -> the streamed layout (K % 64 == 0).  q_up / e_up != NULL: a gate/up pair of an MLP with alternating 16-row
 * tiles (2N rows, N % 16 == 0: the operand of LS_EPI_SILU_MUL, as ls_linear_pack_gate_up).  rope != 0: the q/k layout of
 * LS_EPI_QKV_ROPE (N = heads x 128, as ls_linear_pack_rope).  A scale byte outside [114, 140] is LS_ERR_UNSUPPORTED (a
 * checkpoint quantised elsewhere with a wider exponent range): the call WAITS for its kernel on `stream` to find out (a
 * set-up call; LS_ERR_UNSUPPORTED on a capturing stream -- pack before a HIP-graph capture, never inside one). */
int ls_linear_w4_pack(const uint8_t* q, const uint8_t* e, const uint8_t* q_up, const uint8_t* e_up, void* packed, int N,
                      int K, int rope, void* stream);

/* As ls_linear_workspace_bytes / ls_linear_fwd with d->w[i] pointing at 4-bit packed segments (d->dtype is the
 * activation / output dtype); K % 64 == 0 and K >= 128.  The folded RMSNorm fields (norm_weight, ssq_in, ssq_out) are
 * LS_ERR_UNSUPPORTED here, and there is no prefetch call. */
size_t ls_linear_w4_workspace_bytes(const ls_linear_desc* d);
int ls_linear_w4_fwd(const ls_linear_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* ---- RMSNorm / RoPE (K8, K9) ------------------------------------------------ */

/* LlamaRMSNorm.forward (transformers; imported at longspec/test/llama.py:36; vendored
 * longspec/test/qwen2.py:82-87): y = w * dtype(x32 * rsqrt(mean(x32^2)+eps)).
 * Optional fused residual add: if residual != NULL, x <- x + residual is formed first
 * (rounded to dtype, as `residual + hidden_states` llama.py:492) and written to sum_out. */
int ls_rmsnorm_fwd(const void* x, const void* residual, const void* weight, void* y, void* sum_out,
                   int rows, int hidden, float eps, int dtype, void* stream);

/* LlamaRotaryEmbedding.forward (transformers; vendored qwen2.py:163-178):
 * cos/sin [rows,128] dtype from int64 positions and fp32 inv_freq[64]. */
int ls_rope_cos_sin(const int64_t* positions, const float* inv_freq, float attention_scaling,
                    void* cos, void* sin, int rows, int dtype, void* stream);

/* apply_rotary_pos_emb(q,k,cos,sin,unsqueeze_dim=2) (llama.py:378, llama_glide.py:294), in
 * place on q [rows,Hq,128] and k [rows,Hk,128] (row strides in elements). */
int ls_rope_apply(void* q, void* k, const void* cos, const void* sin, int rows, int Hq, int Hk,
                  int64_t q_row_stride, int64_t k_row_stride, int dtype, void* stream);

/* Tree positions: pos[r] = base[b] + sum_j mask[b,r,j] - 1 (llama.py:575-577, llama_glide.py:1032) */
int ls_tree_positions(const int64_t* tree_mask, const int32_t* base, int b, int M, int N,
                      int64_t* positions, void* stream);

/* ---- beam-tree growth / greedy verification on the lm_head logits ------------------------- */

/* Scratch for the two entry points below (per-chunk maxima, sums and candidates). */
size_t ls_topk_workspace_bytes(int rows, int vocab, int k);

/* `(lm_head(h).float().log_softmax(-1) + history[..., None]).view(-1).topk(k)` of one batch row
 * (longspec/test/llama_glide.py:1019-1020, 1046-1064): logits [rows, vocab] dtype (row stride ld), history
 * [rows] fp32 or NULL.  out_vals [k] fp32 descending, out_idx [k] int64 = row * vocab + column; equal
 * values are ordered by the smaller index.  vocab % 8 == 0, k <= 64, rows <= 128. */
int ls_logprob_topk(const void* logits, int rows, int vocab, int64_t ld, int dtype, const float* history, int k,
                    float* out_vals, int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream);

/* ls_logprob_topk that also keeps the rows' log-probs, the draft's `spec_logits[:, lo:mid] = current_logp` of the
 * temperature > 0 rounds (longspec/test/llama_glide.py:1025,1074): logp[row * logp_ld + j] = (x[j] - m) - ln sum exp(x - m)
 * in fp32 for every input row, m and the sum being the ones the top-k values are computed from -- a second pass over the
 * 16-bit row between the two stages.  logp: 16-byte aligned, logp_ld >= vocab floats and a multiple of 4 (a row slice of
 * spec_logits [1, Fn, V]).  out_vals / out_idx are bit-identical to ls_logprob_topk on the same input. */
int ls_logprob_topk_store(const void* logits, int rows, int vocab, int64_t ld, int dtype, const float* history, int k,
                          float* out_vals, int64_t* out_idx, float* logp, int64_t logp_ld, void* workspace,
                          size_t workspace_bytes, void* stream);

/* `lm_head(h).argmax(-1)` (llama_glide.py:578,1091): out_idx [rows] int64, first maximum of each row. */
int ls_argmax_rows(const void* logits, int rows, int vocab, int64_t ld, int dtype, int64_t* out_idx,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Scratch for ls_sample_rows (per-row selection state, per-chunk histograms and candidates). */
size_t ls_sample_workspace_bytes(int rows, int vocab);

/* One draw per row from soft-max(x / temperature) restricted by top-k and top-p (no counterpart in the reference, whose
 * temperature > 0 paths are ls_tree_verify_stochastic and the chain's rejection block): logits [rows, vocab] dtype (row
 * stride ld; vocab and ld multiples of 8, 16-byte aligned), positions [rows] int64 and streams [rows] int32 (NULL = 0) on the
 * device.  The kept set is {x_j >= t}: top_k > 0 keeps the k largest values counted with multiplicity (ties at the k-th
 * value all kept); top_p < 1 then keeps, of those, the values down to the largest v whose mass from the top,
 * sum n(v') exp((v' - x_max) / temperature) over v' >= v, reaches top_p of the kept mass.  A -inf logit is kept only in a row
 * without a finite one.  The draw is the Gumbel-max with Philox4x32-10, key (seed lo, seed hi), counter (j >> 2, position lo,
 * position hi, stream), output word j & 3 = w_j:  u_j = ((w_j >> 9) + 0.5) * 2^-23,  key_j = x_j / temperature - ln(-ln u_j)
 * in fp32;  out_idx [rows] = the kept column with the largest key, ties to the smaller column.  Optional outputs (NULL to
 * skip): out_top2_idx / out_top2_key [rows, 2] = winner and runner-up among the kept (-1 / -inf when one is kept), out_kept
 * [rows] = size of the kept set, out_threshold [rows] = its smallest value.  A row's outputs depend on that row's logits,
 * position, stream and the scalar arguments only -- not on the other rows, their number, or the run.
 * LS_ERR_INVALID_ARG: vocab or ld not a multiple of 8, misaligned pointers, temperature <= 0, top_k < 0, top_p outside (0, 1]. */
int ls_sample_rows(const void* logits, int rows, int vocab, int64_t ld, int dtype, const int64_t* positions, const int32_t* streams,
                   uint64_t seed, float temperature, int top_k, float top_p, int64_t* out_idx, int64_t* out_top2_idx,
                   float* out_top2_key, int32_t* out_kept, float* out_threshold, void* workspace, size_t workspace_bytes,
                   void* stream);

/* ls_sample_rows with two more filters.  Order: top_k -> top_p -> min_p -> typical_p, each on the set the former kept.
 *   min_p in [0, 1] (0 = off): keep j iff exp((x_j - x_max) / temperature) >= min_p.
 *   typical_p in (0, 1] (1 = off), locally typical sampling on the set S kept so far: with a(v) = (x_max - v) / temperature,
 *     q(v) = exp(-a(v)) / Z over S and A = sum q a (the entropy is ln Z + A, the surprise of v is ln Z + a(v)), the distance of
 *     v is d(v) = |a(v) - A|; d* is the smallest distance with sum of q over {d(v) <= d*} >= typical_p and {j in S : d(x_j) <= d*}
 *     is kept, ties at d* included.  The kept values are a contiguous run [lo, hi] of S's values; the maximum may be dropped.
 * out_threshold [rows] = the smallest kept finite value, out_upper [rows] (optional) = the largest (-inf for a row without a
 * finite logit), out_kept = the kept count.  With min_p = 0 and typical_p = 1 the launches and every output bit are those of
 * ls_sample_rows.  Everything else -- the draw, the keying, alignment, the independence of the rows -- as ls_sample_rows.
 * LS_ERR_INVALID_ARG: as ls_sample_rows, and min_p outside [0, 1] or typical_p outside (0, 1]. */
typedef struct ls_sample_desc {
    const void* logits;          /* [rows, vocab] dtype, row stride ld                                   */
    const int64_t* positions;    /* [rows]                                                               */
    const int32_t* streams;      /* [rows] or NULL (= 0)                                                 */
    int64_t* out_idx;            /* [rows]                                                               */
    int64_t* out_top2_idx;       /* [rows, 2] or NULL                                                    */
    float* out_top2_key;         /* [rows, 2] or NULL                                                    */
    int32_t* out_kept;           /* [rows] or NULL                                                       */
    float* out_threshold;        /* [rows] or NULL                                                       */
    float* out_upper;            /* [rows] or NULL                                                       */
    int64_t ld;
    uint64_t seed;
    int32_t rows, vocab, dtype, top_k;
    float temperature, top_p, min_p, typical_p;
} ls_sample_desc;

/* Scratch for ls_sample_rows_ex: ls_sample_workspace_bytes plus, with typical_p < 1, 768 KiB per row (counts and prefix sums
 * of the 2^16 values; fully rewritten by every call, no clearing needed). */
size_t ls_sample_ex_workspace_bytes(const ls_sample_desc* d);
int ls_sample_rows_ex(const ls_sample_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* ls_sample_rows_ex with two cuts (csrc/sample_cut.hip; longspec_amd/cut.py).  Order: top_n_sigma -> top_k -> top_p -> min_p ->
 * typical_p -> xtc, each on the set the former kept.  m is the row maximum, T the temperature of the descriptor.
 *   top_n_sigma = n, finite and >= 0 (0 = off): over the N finite logits of the row (-inf takes no part) sigma =
 *     sqrt(sum (x - mean)^2 / N), the population deviation of the raw 16-bit values, NOT divided by T; keep x_j >= m - n sigma.
 *     A threshold set that holds the maximum, so it intersects with top_k in either order, and top_p's mass is taken over what
 *     both kept.  sigma = 0 (one finite logit, all equal) keeps the maxima; a row without a finite logit is left alone.  The
 *     sums are taken in double on y = x - m in a fixed order (per-chunk partial records, plain stores, summed in chunk order):
 *     the bits do not depend on scheduling.
 *   xtc = (probability P in [0, 1], 0 = off; threshold theta in (0, 1]), "exclude top choices".  The row's coin is
 *     Philox4x32-10 with key (seed lo, seed hi) and counter (0xFFFFFFFF, position lo, position hi, stream) -- token noise has
 *     counter word 0 = column >> 2 < 2^22, the streams cannot meet --, u = ((w0 >> 9) + 0.5) * 2^-23, and the cut happens iff
 *     u < P in fp32.  Then, with S the set kept so far, F(v) = floor(2^40 exp((v - m) / T)) in double as top_p forms it and
 *     Z = sum of F over S (unsigned 64-bit): v* = the smallest value occurring in S with F(v*) >= ceil(theta Z), and every j in S
 *     with x_j > v* is dropped.  ALL tokens tied at v* stay (llama.cpp keeps one of them; the rule mirrors top_k's ties).  If
 *     only the largest value of S qualifies, or none does, the row is unchanged: theta > 0.5 is a no-op without a tie at the
 *     top.  One departure from the letter of the rule: where Z = 0 -- typical_p has moved S more than 40 ln 2 * T below m, so
 *     that every F floors to 0 -- ceil(theta * 0) = 0 would let every value qualify; such a row is left unchanged.  A row whose
 *     coin does not fire is not read by the xtc kernels.
 * out_kept, out_threshold, out_upper and the top-2 outputs describe the final set.  With `cut` NULL or both filters off the
 * launches and every output bit are those of ls_sample_rows_ex.
 * LS_ERR_INVALID_ARG, before any launch: as ls_sample_rows_ex, and top_n_sigma < 0 or not finite, xtc_probability outside
 * [0, 1], xtc_threshold outside (0, 1], a NaN in any of them, reserved != 0. */
typedef struct ls_sample_cut {
    float top_n_sigma, xtc_probability, xtc_threshold;
    int32_t reserved;            /* 0 */
} ls_sample_cut;

/* Scratch for ls_sample_rows_cut: that of ls_sample_rows_ex (the cuts keep their partial records in its histogram area). */
size_t ls_sample_cut_workspace_bytes(const ls_sample_desc* d, const ls_sample_cut* cut);
int ls_sample_rows_cut(const ls_sample_desc* d, const ls_sample_cut* cut, void* workspace, size_t workspace_bytes, void* stream);

/* Token penalties and a logit bias on TARGET logits, in front of ls_argmax_rows / ls_sample_rows (csrc/penalty.hip; no counterpart
 * in the reference).  state [b, vocab] int32 (batch stride state_stride_b): bits 0-30 of a word = times the token was generated
 * (first token included), bit 31 = the token occurs in the valid part of the prompt.  logits / out [b, rows, vocab] dtype with
 * batch and row strides in elements; out == logits is allowed.  Row r of batch z adds to its history every extra_ids[z, c]
 * (int64, batch stride ids_stride_b) with extra_mask[z, r, c] != 0 (int64, batch / row strides, unit column stride; a batch
 * stride of 0 = one mask for every batch row), c < n_extra: a duplicate counts twice, an id outside [0, vocab) is ignored;
 * n_extra = 0: no extras, both pointers may be NULL.  Per element v with 16-bit logit x, in fp32, every operation rounded once
 * and never contracted, with c = count of v in the state + in the row's selected extras:
 *   1. c > 0 or the prompt bit:  x = x / repetition when x > 0 (the correctly rounded IEEE quotient), else x = x * repetition
 *   2. c > 0:                    t = frequency * float(c);  x = x - t;  x = x - presence
 *   3. bias != NULL:             x = x + bias[v]            (bias [vocab] fp32; -inf bans a token)
 *   4. out = x rounded to nearest-even in dtype (-inf stays -inf, an overflow becomes +-inf)
 * One launch, no workspace, no atomics; a row's output depends on that row, its extras and the scalars only.
 * LS_ERR_INVALID_ARG, before any launch: vocab or a stride not a multiple of 8, a row stride < vocab, logits / out / state / bias
 * not 16-byte aligned, repetition <= 0 (or NaN), n_extra outside 0..1024. */
int ls_penalize_rows(const void* logits, void* out, int b, int rows, int vocab, int dtype, int64_t in_stride_b, int64_t in_stride_r,
                     int64_t out_stride_b, int64_t out_stride_r, const int32_t* state, int64_t state_stride_b,
                     const int64_t* extra_ids, int64_t ids_stride_b, const int64_t* extra_mask, int64_t mask_stride_b,
                     int64_t mask_stride_r, int n_extra, float repetition, float presence, float frequency, const float* bias,
                     void* stream);

/* Update of that state: for every ids[z, j] (int64, batch stride ids_stride_b), j < n and -- with num != NULL -- j <
 * num[z * num_stride] (int64), inside [0, vocab): prompt == 0 adds 1 per occurrence (integer atomics: the same id three times in
 * one call adds 3, bit 31 is never touched below 2^31 occurrences); prompt != 0 ORs bit 31 (idempotent, the count is not
 * touched).  Ids outside the vocabulary -- zero padding aside, the out-of-vocabulary pad of the accepted-id row -- are ignored. */
int ls_token_state_add(int32_t* state, int b, int vocab, int64_t state_stride_b, const int64_t* ids, int n, int64_t ids_stride_b,
                       const int64_t* num, int64_t num_stride, int prompt, void* stream);

/* Log-probabilities of emitted tokens and their top-n alternatives (logprobs=; csrc/logprob.hip; no counterpart in the reference).
 * logits [b, rows, vocab] dtype with batch and row strides in elements: the TARGET's logits as the token was picked from them,
 * i.e. behind ls_penalize_rows.  ids [b, rows] int64 (batch stride ids_stride_b): the chosen column of every row.  Per row, in
 * fp32 with every operation rounded once, m = max_i x_i and lse = ln sum_i exp((x_i - m) / temperature):
 *   lp_j = (x_j - m) / temperature - lse
 * over the FULL vocabulary -- the tempered (and penalised) soft-max, not the set a top-k / top-p cut of the sampler keeps.
 *   row_lp      [b, rows] fp32      lp of the chosen column; NaN for an id outside [0, vocab); -inf for a -inf logit
 *   row_top_val [b, rows, n] fp32   lp of the n columns with the largest logits, ordered by (logit descending, column ascending)
 *   row_top_idx [b, rows, n] int64  with -0.0 == +0.0 (the order of ls_argmax_rows), their columns; a row with fewer than n columns
 *                                   is padded with (-inf, -1).  Both NULL when n == 0.
 * Equal logits of a row get bit-equal values, and row_lp is bit-equal to the chosen column's list entry when it is listed.  A row
 * whose maximum is -inf gives NaN.  A row's outputs depend on that row, its id, temperature and n only.  Two launches: (chunks of
 * 8192 columns, rows * b) workgroups write one record each (max, sum, n candidates) into the workspace, one workgroup per row
 * merges them in chunk order; no floating-point atomics.  LS_ERR_INVALID_ARG, before any launch: vocab or a stride not a multiple
 * of 8, a row stride < vocab, misaligned pointers (logits 16 bytes), temperature <= 0 (or NaN, or infinite), n outside 0..20,
 * rows * b outside 1..1024.  LS_ERR_UNSUPPORTED: vocab > 524288. */
size_t ls_token_logprobs_workspace_bytes(int b, int rows, int vocab, int n);
int ls_token_logprobs(const void* logits, int b, int rows, int vocab, int dtype, int64_t stride_b, int64_t stride_r,
                      const int64_t* ids, int64_t ids_stride_b, float temperature, int n, float* row_lp, float* row_top_val,
                      int64_t* row_top_idx, void* workspace, size_t workspace_bytes, void* stream);

/* The rows a round accepted -> the output columns of the tokens they produced (one launch, one workgroup per batch row).  For
 * j < num[z * num_stride] (int64; num == NULL: every j < max_rows):  src = map ? map[z, j] : j  (map int64 [b, max_rows]),
 * dst = base[z] + base_add + j  (base int32 [b], on the device);  row_lp[z, src] -> out_token[z, dst] and the n-vectors
 * row_top_val / row_top_idx [z, src, :] -> out_top_val / out_top_idx [z, dst, :]  (out_* [b, out_cap(, n)], dense).  src outside
 * [0, rows) and dst outside [0, out_cap) are skipped, never written.  n == 0: the four top-n pointers may be NULL. */
int ls_logprob_commit(const float* row_lp, const float* row_top_val, const int64_t* row_top_idx, int b, int rows, int n,
                      const int64_t* map, int max_rows, const int64_t* num, int64_t num_stride, const int32_t* base, int base_add,
                      float* out_token, float* out_top_val, int64_t* out_top_idx, int out_cap, void* stream);

/* Stop conditions of the decode loops (stop=; csrc/stop.hip; no counterpart in the reference, which tests one EOS id).
 * table: int32 [LS_STOP_TABLE_WORDS] on the device -- [0] n_ids (0..64), [1] n_seqs (0..16), [2] min_tokens, [3] the word count,
 * [4:68] the stop token ids (-1 padded), [68:85] offsets of the stop sequences into the token area, [85:341] their tokens back to
 * back (1..16 each).  Counts and offsets are clamped to this layout on the device before they index anything.
 *
 * ls_stop_scan: one wave per batch row, behind the round's commit.  output_ids [b, width] int64 (row stride out_stride_b);
 * w = written[z] - (written_sub ? written_sub[z] : 0) + written_add columns are written (clamped to 0..width), the last
 * n = (num ? num[z * num_stride] : num_const) of them by this round (clamped to 0..w).  A stop matches at column c >= min_tokens
 * when output_ids[z, c] is a stop id, or a sequence of length L <= c + 1 equals output_ids[z, c-L+1 : c+1]; no read goes in front
 * of column 0 or to column w and beyond.  Among the round's columns the smallest c wins and, there, the first stop in listing
 * order (ids, then sequences): stop_state[z] (int32 [b, 4]) = (length = c + 1, which, match_start = c - L + 1, reserved).  A row
 * whose stop_state[z, 0] is >= 0 already matches nothing new.  In both cases the columns [length, w) of output_ids go back to
 * `fill`, of spec_mask (optional, row stride mask_stride_b) to 0, of lp_token / lp_top / lp_top_ids (optional, dense
 * [b, width(, lp_n)]) to NaN / -inf / -1, and round_state[z * state_stride_b + 1] |= 2 (optional: the round's state tensor, so that
 * its one host read carries the hit).  A row without a match is not touched.  Exact; no workspace, no atomics.
 *
 * ls_stop_ban_rows: the min_tokens ban on 16-bit target logits [b, rows, vocab] (strides in elements), IN PLACE, one wave per row.
 * Row r of batch z predicts column (base ? base[z] : 0) - (base_sub ? base_sub[z] : 0) + base_add + depth(r), depth = 0
 * (depth_mode 0), r (1) or the number of non-zero mask[z, r, 1 : mask_cols] (2; mask int64, batch / row strides, unit column
 * stride).  Where that column is < min_tokens the entries of the stop ids inside [0, vocab) become -inf; every other element and
 * every other row keeps its bits. */
#define LS_STOP_TABLE_WORDS 341
int ls_stop_scan(int64_t* output_ids, int b, int64_t out_stride_b, int width, const int32_t* written, const int32_t* written_sub,
                 int written_add, const int64_t* num, int64_t num_stride, int num_const, const int32_t* table, int table_words,
                 int32_t* stop_state, int64_t fill, int64_t* round_state, int64_t state_stride_b, int64_t* spec_mask,
                 int64_t mask_stride_b, float* lp_token, float* lp_top, int64_t* lp_top_ids, int lp_n, void* stream);
int ls_stop_ban_rows(void* logits, int b, int rows, int vocab, int dtype, int64_t stride_b, int64_t stride_r, const int32_t* table,
                     int table_words, const int32_t* base, const int32_t* base_sub, int base_add, int depth_mode,
                     const int64_t* mask, int64_t mask_stride_b, int64_t mask_stride_r, int mask_cols, void* stream);

/* Banned sequences and no-repeat n-grams on the target's logits (ban=; csrc/ban.hip; no counterpart in the reference).
 * table: int32 [LS_BAN_TABLE_WORDS] on the device -- [0] n_seqs (0..64), [1] n = no_repeat_ngram (0 = off, 1..16), [2] reserved,
 * [3] the word count, [4:69] offsets of the sequences into the token area, [69:1093] their tokens back to back (1..16 each, -1
 * padded).  Counts, n and offsets are clamped to this layout on the device before they index anything.
 *
 * ls_ban_rows: 16-bit logits [b, rows, vocab] (strides in elements, unit column stride, rows must not overlap), IN PLACE, one
 * launch.  The text of row r of batch z is t = output_ids[z, :w] ++ path(r), m tokens: w = (base ? base[z] : 0) - (base_sub ?
 * base_sub[z] : 0) + base_add clamped to 0..width (output_ids int64 [b, width], row stride out_stride_b; NULL with width 0: no
 * columns), path(r) = extra_ids[z, c] for the c < n_extra with extra_mask[z, r, c] != 0, IN INCREASING c (extra_ids int64, row
 * stride ids_stride_b; extra_mask int64, strides mask_stride_b -- 0: one mask for the batch -- and mask_stride_r, unit column
 * stride; n_extra 0..LS_BAN_MAX_EXTRA).  Ids are compared as 64-bit integers, whatever their value.  Forbidden in row (z, r):
 *   - s[L-1] of every listed sequence s of length L with L - 1 <= m and t[m-L+1 .. m-1] == s[0 .. L-2]  (L = 1: always);
 *   - with n >= 1 and m >= n - 1: t[j] for every j in [n-1, m-1] with t[j-n+1 .. j-1] == t[m-n+1 .. m-1]  (n = 1: all of t).
 * A forbidden id inside [0, vocab) gets the type's -inf pattern (0xfc00 / 0xff80) by a plain 16-bit store -- two lanes that hit
 * one address store the same value --; every other element keeps its bits; ids outside [0, vocab) are never written.  Nothing
 * in front of column 0 or at column w and beyond is read.  Grid (ceil(rows / 4) + ceil(width / LS_BAN_CHUNK) * ceil(rows / 32), b)
 * workgroups of 256: a path workgroup takes one row per wave, assembles its ordered path in LDS and tests the sequences and the
 * positions j >= w; a chunk workgroup reads the text columns [k * LS_BAN_CHUNK - 16, (k + 1) * LS_BAN_CHUNK) once into LDS and tests
 * its positions j < w against the last n - 1 tokens of each of its 32 rows (k * LS_BAN_CHUNK >= w, or n = 0: it returns at
 * once).  The grid depends on host-side shapes only: nothing is read back, safe inside a replayed graph.  Exact; no workspace,
 * no atomics, no floating point.  LS_ERR_INVALID_ARG, before any launch: null logits / table, a dtype that is not 16-bit, b or
 * rows outside 1..65535, vocab < 1, stride_r < vocab, table_words != LS_BAN_TABLE_WORDS, width outside 0..2^23 or without
 * output_ids, out_stride_b < width, n_extra outside 0..LS_BAN_MAX_EXTRA (128: a verification pass has at most 80 rows) or without
 * its two tensors. */
#define LS_BAN_TABLE_WORDS 1093
#define LS_BAN_CHUNK 1024
#define LS_BAN_MAX_EXTRA 128
int ls_ban_rows(void* logits, int b, int rows, int vocab, int dtype, int64_t stride_b, int64_t stride_r, const int32_t* table,
                int table_words, const int64_t* output_ids, int64_t out_stride_b, int width, const int32_t* base,
                const int32_t* base_sub, int base_add, const int64_t* extra_ids, int64_t ids_stride_b, const int64_t* extra_mask,
                int64_t mask_stride_b, int64_t mask_stride_r, int n_extra, void* stream);

/* The DRY repetition penalty on the target's logits (dry=; csrc/dry.hip; no counterpart in the reference).
 * table: int32 [LS_DRY_TABLE_WORDS] on the device -- [0] number of breakers (0..64), [1] allowed_length (1..LS_DRY_MAX_MATCH),
 * [2] last_n (0 = the whole text, else 1..2^23), [3] the word count, [4:37] pen[0 .. 32] as fp32 bits, [37:101] the breaker ids
 * (-1 padded).  Counts are clamped to this layout on the device before they index anything.
 *
 * ls_dry_rows: 16-bit logits [b, rows, vocab] (strides in elements, unit column stride, rows must not overlap), IN PLACE, two
 * launches of one kernel.  The text t of row (z, r), its m tokens, w, output_ids, base / base_sub / base_add and the extras are
 * those of ls_ban_rows, n_extra 0..LS_BAN_MAX_EXTRA included.  With lo = max(0, m - last_n) (last_n = 0: 0): nothing changes if
 * m - lo < 2 or t[m-1] is a breaker.  For every j in [lo, m-2] with t[j] == t[m-1], L(j) is the largest L <= LS_DRY_MAX_MATCH
 * with j-k >= lo, t[j-k] == t[m-1-k] and t[j-k] no breaker for all k < L; len[v] = the maximum of L(j) over the j with
 * t[j+1] == v.  Every v inside [0, vocab) with len[v] >= allowed_length becomes dtype(float(logits[z, r, v]) - pen[len[v]]): one
 * fp32 subtract, rounded to nearest even; a NaN keeps its bits, -inf stays -inf.  Every other element keeps its bits; ids
 * outside [0, vocab) take part in the matches (compared as 64-bit integers) and are never penalised.
 * scratch: int32, scratch_words >= b * rows * vocab, indexed [z, r, v] densely; ALL ZERO ON ENTRY, ALL ZERO ON EXIT.  Pass 0 raises
 * scratch[z, r, v] to len[v] with device-scope atomic maxima, pass 1 visits the same positions and the one thread whose
 * compare-and-swap (len[v] -> 0) succeeds rewrites the element: one writer per element, bits that do not depend on scheduling, a
 * scratch that cleans itself.  The cost depends on the text, never on vocab: no sweep of the scratch or of the rows.
 * Grid (ceil(rows / 4) + ceil(width / LS_BAN_CHUNK) * ceil(rows / 32), b) workgroups of 256, twice: a path workgroup takes one row
 * per wave and the positions j >= w-1, whose candidate t[j+1] is a token of the row's path; a chunk workgroup reads the columns
 * [k * LS_BAN_CHUNK - 32, (k + 1) * LS_BAN_CHUNK] once into LDS and tests its positions j <= w-2 against the last 32 tokens of
 * each of its 32 rows (a chunk at or behind w-1, or in front of every row's lo: it returns at once).  The grid depends on
 * host-side shapes only: nothing is read back, nothing is allocated, safe inside a replayed graph.
 * LS_ERR_INVALID_ARG, before any launch: the refusals of ls_ban_rows, table_words != LS_DRY_TABLE_WORDS, a null or misaligned
 * scratch or scratch_words < b * rows * vocab. */
#define LS_DRY_MAX_MATCH 32
#define LS_DRY_TABLE_WORDS 101
int ls_dry_rows(void* logits, int b, int rows, int vocab, int dtype, int64_t stride_b, int64_t stride_r, const int32_t* table,
                int table_words, const int64_t* output_ids, int64_t out_stride_b, int width, int32_t* scratch, int64_t scratch_words,
                const int32_t* base, const int32_t* base_sub, int base_add, const int64_t* extra_ids, int64_t ids_stride_b,
                const int64_t* extra_mask, int64_t mask_stride_b, int64_t mask_stride_r, int n_extra, void* stream);

/* Watermarked decoding: a keyed green-list bias on the target's logits, and its detector (watermark=; csrc/watermark.hip; no
 * counterpart in the reference).  This definition is a public contract: a text marked today verifies with a later build.
 * All arithmetic is on unsigned 64-bit words, modulo 2^64, with M1 = 0x9E3779B97F4A7C15, M2 = 0xBF58476D1CE4E5B9,
 * M3 = 0x94D049BB133111EB:
 *   fin(z):  z = (z ^ (z >> 30)) * M2;  z = (z ^ (z >> 27)) * M3;  return z ^ (z >> 31)        (the SplitMix64 finaliser)
 *   state of the context c_1 .. c_h, oldest first (int64 ids reinterpreted as uint64, whatever their value):
 *            s = fin(key + M1);  for each c_i:  s = fin((s ^ c_i) + M1)
 *   u(s, v) = fin(s + (v + 1) * M1);  v is GREEN after that context iff (u >> 32) < T.
 * table: int32 [LS_WATERMARK_TABLE_WORDS] on the device -- [0] h (1..LS_WATERMARK_MAX_CONTEXT; clamped on the device), [1] T =
 * floor(gamma * 2^32) as bits (1..2^32-1), [2] delta as fp32 bits, [3] the word count, [4] [5] the key's low and high word,
 * [6] [7] zero.
 *
 * ls_watermark_rows: 16-bit logits [b, rows, vocab] (strides in elements, unit column stride, rows must not overlap), IN PLACE,
 * one launch.  The text t of row (z, r), its m tokens, w, output_ids, base / base_sub / base_add and the extras are those of
 * ls_ban_rows, n_extra 0..LS_BAN_MAX_EXTRA included.  A row with m < h keeps its bits and its elements are not read.  Otherwise
 * s is the state of t[m-h .. m-1] and every green v inside [0, vocab) becomes dtype(float(logits[z, r, v]) + delta): one fp32
 * add, rounded to nearest even; a NaN keeps its bits, -inf stays -inf.  Every element that is not green keeps its bits.  NOT
 * idempotent: a second call adds delta again.  Grid (ceil((vocab + 7) / 8192), rows, b) workgroups of 256: wave 0 assembles the
 * row's path in LDS, takes the last h tokens from the path's tail and -- where the path is shorter -- from the end of the
 * committed columns, folds them serially and leaves s in LDS; every thread then takes four groups of eight ids that are
 * 16-byte aligned in memory -- one 16-byte load, the eight u by additions of M1 from one multiplied-out start, and one 16-byte
 * store unless none of the eight is green --; the groups that hang over a row's two ends (a row is only 2-byte aligned, vocab
 * may be odd) go element by element.  Nothing is allocated, nothing is read back: safe inside a replayed graph.
 * LS_ERR_INVALID_ARG, before any launch: the refusals of ls_ban_rows, with table_words != LS_WATERMARK_TABLE_WORDS.
 *
 * ls_watermark_score: ids int64 [b, n] (row stride stride_b >= n; n 0..2^31-1), lengths int32 [b] or NULL (clamped to 0..n;
 * NULL: n).  Position c of row z is scored iff h <= c < length; it is green iff ids[z, c] is green after ids[z, c-h .. c-1].
 * counts int32 [b, 2] = (scored, green), OVERWRITTEN (cleared on the stream in front of the launch, then integer atomic adds of
 * per-workgroup ballot counts: the result does not depend on scheduling); flags int8 [b, n] dense or NULL: -1 not scored,
 * 0 red, 1 green; hashes uint64 [b, n] dense or NULL: u of a scored position, 0 elsewhere.  Grid (ceil(n / 256), b) workgroups
 * of 256, a thread per position, which folds its own context; n = 0: the counts are cleared and nothing is launched.
 * LS_ERR_INVALID_ARG: a null table / counts / ids, table_words, b outside 1..65535, n out of range, stride_b < n with b > 1,
 * misaligned counts or hashes. */
#define LS_WATERMARK_TABLE_WORDS 8
#define LS_WATERMARK_MAX_CONTEXT 8
int ls_watermark_rows(void* logits, int b, int rows, int vocab, int dtype, int64_t stride_b, int64_t stride_r, const int32_t* table,
                      int table_words, const int64_t* output_ids, int64_t out_stride_b, int width, const int32_t* base,
                      const int32_t* base_sub, int base_add, const int64_t* extra_ids, int64_t ids_stride_b, const int64_t* extra_mask,
                      int64_t mask_stride_b, int64_t mask_stride_r, int n_extra, void* stream);
int ls_watermark_score(const int64_t* ids, int b, int64_t n, int64_t stride_b, const int32_t* lengths, const int32_t* table,
                       int table_words, int32_t* counts, int8_t* flags, uint64_t* hashes, void* stream);

/* Guided decoding: a deterministic automaton over token ids on the target's logits (guide=; csrc/guide.hip; no counterpart in
 * the reference).  table: int32 [table_words] on the device, 16-byte aligned (longspec_amd/guide.py builds it) --
 *   [0] S >= 1   [1] C (1..LS_GUIDE_MAX_CLASSES)   [2] start   [3] vocab   [4] the word count   [5:8] reserved (0)
 *   [8 : 8 + K]  the classes of ids 0 .. vocab-1 as 16-bit values, two per word, the even id in the low half, LS_GUIDE_NO_CLASS
 *                (0xFFFF) = forbidden in every state; K = ceil(vocab / 2) rounded up to a multiple of 4 words (padding 0xFFFF),
 *                so that the transition area starts 16-byte aligned
 *   [8 + K : 8 + K + S * C]  next, int32 [S, C] row-major: the state behind a token of class c in state s, -1 = no transition
 * with S * C <= LS_GUIDE_MAX_CELLS.  walk(s, id) = -1 where s < 0, id lies outside [0, vocab) or its class is forbidden (0xFFFF,
 * or a value >= C), else next[s, class(id)], a value outside [-1, S) counting as -1.  A header whose S, C, vocab are out of range
 * or whose areas do not fit table_words makes every row dead and every state -1: nothing read from the table indexes memory
 * unclamped.
 *
 * ls_guide_rows: 16-bit logits [b, rows, vocab] (strides in elements, unit column stride, rows must not overlap), IN PLACE, one
 * launch.  Row r of batch z starts in s = state[z] (int32 [b]; outside [-1, S): -1) and walks every extra_ids[z, c], c <
 * n_extra, with extra_mask[z, r, c] != 0, IN INCREASING c (extra_ids int64, row stride ids_stride_b; extra_mask int64, strides
 * mask_stride_b -- 0: one mask for the batch -- and mask_stride_r, unit column stride; n_extra 0..LS_GUIDE_MAX_EXTRA), ids
 * bounded by the smaller of `vocab` and the table's.  s < 0 behind the walk: the row is DEAD and every element keeps its bits (a
 * committed state of -1 leaves all its rows alone).  Otherwise every v in [0, vocab) with walk(s, v) < 0 -- ids at or beyond the
 * table's vocab included -- gets the type's -inf pattern (0xfc00 / 0xff80); every other element keeps its bits, NaN payloads, -0.0
 * and the gaps between rows included.  The logits are never read.  Grid (ceil(vocab / LS_GUIDE_SLICE), rows, b) workgroups of 256:
 * every workgroup redoes its row's walk (the path assembled by ballot + prefix, the classes of all path tokens looked up in
 * parallel, the chain through next serial), packs next[s, :] into C allow bits in LDS and streams its slice of the vocabulary with
 * 16-byte class loads; a group of eight ids that is wholly forbidden at a 16-byte aligned address is one 16-byte store, a wholly
 * allowed one nothing, anything else 16-bit stores of the forbidden ids (a row that is only 2-byte aligned, the ragged tail of a
 * vocab that is no multiple of 8).  The grid depends on host-side shapes only: nothing is read back, safe inside a replayed
 * graph.  Exact; no workspace, no atomics, no floating point.  LS_ERR_INVALID_ARG, before any launch: null logits / table /
 * state, a dtype that is not 16-bit, b or rows outside 1..65535, vocab < 1, stride_r < vocab, table_words < LS_GUIDE_HEADER_WORDS,
 * a table that is not 16-byte aligned, n_extra outside 0..LS_GUIDE_MAX_EXTRA or without its two tensors.
 *
 * ls_guide_advance: state[z] (int32 [b], IN PLACE) = state[z] walked along ids[z, j], j < min(num[z * num_stride], n) (ids int64
 * [b, n], row stride ids_stride_b; num int64, NULL: all n; negative: 0; n 1..LS_GUIDE_MAX_EXTRA), ids bounded by the table's
 * vocab.  -1 stays -1.  One wave per batch row: the classes in parallel, the chain serial.  One launch, graph-safe; the same
 * refusals for b, n, the table and negative strides. */
#define LS_GUIDE_HEADER_WORDS 8
#define LS_GUIDE_MAX_CLASSES 16384
#define LS_GUIDE_MAX_CELLS 16777216
#define LS_GUIDE_NO_CLASS 65535
#define LS_GUIDE_MAX_EXTRA 128
#ifndef LS_GUIDE_SLICE       /* (measurement builds set another slice: tools/ab_guide_round.py; a multiple of 2048) */
#define LS_GUIDE_SLICE 8192
#endif
int ls_guide_rows(void* logits, int b, int rows, int vocab, int dtype, int64_t stride_b, int64_t stride_r, const int32_t* table,
                  int table_words, const int32_t* state, const int64_t* extra_ids, int64_t ids_stride_b, const int64_t* extra_mask,
                  int64_t mask_stride_b, int64_t mask_stride_r, int n_extra, void* stream);
int ls_guide_advance(int32_t* state, int b, const int32_t* table, int table_words, const int64_t* ids, int n, int64_t ids_stride_b,
                     const int64_t* num, int64_t num_stride, void* stream);

/* The lift of a byte-level DFA to the tokens of a vocabulary (Guide.from_byte_dfa / Guide.from_regex on a device;
 * csrc/guide_lift.hip; no counterpart in the reference).  A token's behaviour is the vector state -> state of running its bytes.
 *   step     16-bit [256, S + 1] on the device, BYTE-major: step[c * (S + 1) + s] = the state behind byte c in state s, S = the
 *            dead state (step[c, S] = S); S in 1..LS_GUIDE_LIFT_MAX_STATES.  An entry beyond S counts as S.
 *   blob     uint8 [blob_bytes]: the bytes of all tokens back to back (a valid pointer also where blob_bytes is 0)
 *   offsets  int32 [T + 1]: token t is blob[offsets[t] : offsets[t + 1]]; a pair that is not 0 <= begin <= end <= blob_bytes
 *            counts as an empty token.  An empty token is dead from every state.
 * One launch each, lanes across states, several tokens per wave where S < 64, slices of 64 states beyond; nothing read indexes
 * memory unclamped.  Exact; no workspace, no atomics, no floating point; every output element is written by every call.
 *
 * ls_guide_lift_hash: hashes uint64 [T, 2] = two independent 64-bit hashes of every token's vector (each the wrap-around sum over
 * s of a mix of (s, the end state of s), summed across lanes by shuffles: equal vectors have equal hashes); alive uint8 [T] = 1
 * where the token is not empty and some state survives it, else 0.
 * ls_guide_lift_cols: cols int32 [n, S] = the vector of token ids[i] (int32 [n]; an id outside [0, T): an empty token), -1 = dead.
 * ls_guide_lift_check: mismatch uint8 [T] = 1 where group[t] >= 0 (int32 [T]) and the token's vector differs from
 * reps[group[t]] (int32 [C, S], -1 = dead) or group[t] >= C; else 0.  Tokens with group[t] < 0 are not walked.
 * LS_ERR_INVALID_ARG, before any launch: a null pointer, S outside 1..LS_GUIDE_LIFT_MAX_STATES, T, n or C < 1, blob_bytes < 0. */
#define LS_GUIDE_LIFT_MAX_STATES 16384
int ls_guide_lift_hash(const void* step, const void* blob, const int32_t* offsets, int64_t blob_bytes, int T, int S, uint64_t* hashes,
                       uint8_t* alive, void* stream);
int ls_guide_lift_cols(const void* step, const void* blob, const int32_t* offsets, int64_t blob_bytes, int T, int S, const int32_t* ids,
                       int n, int32_t* cols, void* stream);
int ls_guide_lift_check(const void* step, const void* blob, const int32_t* offsets, int64_t blob_bytes, int T, int S, const int32_t* reps,
                        int C, const int32_t* group, uint8_t* mismatch, void* stream);

/* The drafter of prompt-lookup (n-gram) speculation (lookup_generate; csrc/lookup.hip; no counterpart in the reference, whose
 * every loop needs a trained draft layer).  The text of batch row z is T = prompt_ids[z, :il] ++ output_ids[z, :w], il =
 * input_len[z] clamped to 0..prompt_cols, w = cache_lens[z] - input_len[z] + 1 clamped to 0..out_cap (the columns written so far,
 * the last round's bonus token included), L = il + w; prompt padding and output columns at or behind w are never read.  For an
 * end e in 1 .. L-1, m(e) is the largest k <= min(max_ngram, e) with T[e-k:e] == T[L-k:L] (ids compared as 64-bit integers,
 * occurrences may overlap the suffix); among the ends with m(e) >= min_ngram the largest m wins, then the largest e.
 *   spec_buffer [b, gamma+1] int64 dense   [z, 1+i] = T[e + i mod (L - e)], i < gamma: the continuation, read on into the draft
 *                                          itself where it reaches the end of the text; no candidate: T[L-1].  Column 0 is kept.
 *   info        [b, 2] int32               (n, e) = (m of the winner, its end), or (0, -1)
 *   hist        [b, max_ngram+1] int64     hist[z, n] += 1 (one writer per row, no atomics); may be NULL
 * len_bound is a HOST-side upper bound of L (the bound the round's attention launches are sized from): it sizes the grid and the
 * workspace, nothing on the device is read for it; a longer text is searched over its first ends only and never read out of range.
 * Two launches: (chunks of LS_NGRAM_CHUNK ends, b) workgroups write one 64-bit record (m << 32 | e) each into the workspace -- one
 * pass over the text, 8-byte loads --, one wave per row takes their maximum and writes the results.  Every record is rewritten by
 * every call: nothing to zero between calls, safe inside a replayed graph.  Exact; no floating point.  LS_ERR_INVALID_ARG, before
 * any launch: gamma outside 1..15, max_ngram outside 1..8, min_ngram outside 1..max_ngram, b outside 1..65535, a column count
 * outside 1..2^30-1 or above its row stride, misaligned pointers. */
#define LS_NGRAM_CHUNK 1024
size_t ls_ngram_workspace_bytes(int b, int64_t len_bound);
int ls_ngram_draft(const int64_t* prompt_ids, int64_t prompt_stride_b, int prompt_cols, const int32_t* input_len,
                   const int64_t* output_ids, int64_t out_stride_b, int out_cap, const int32_t* cache_lens, int b, int64_t len_bound,
                   int gamma, int max_ngram, int min_ngram, int64_t* spec_buffer, int32_t* info, int64_t* hist, void* workspace,
                   size_t workspace_bytes, void* stream);

/* The TREE drafter of prompt-lookup speculation (lookup_generate(branches=B); csrc/lookup_tree.hip): up to B distinct continuations
 * per round, laid out as a level-major tree that ls_verify_attention's packed tree mask, ls_tree_verify_inputs, ls_tree_collapse and
 * ls_tree_commit take as it is.  The text, m(e), the candidates and their key (m, e) are ls_ngram_draft's, but for the output
 * columns that count as text: w = written[z] clamped to 0..out_cap (the tree round's emitted_dev; its cache_lens lags the text by
 * the tokens the next pass feeds again).  The LS_NGRAM_TOP candidates with the largest keys are walked in descending order; one is
 * kept when its gamma-token continuation c_e[i] = T[e + i mod (L - e)] differs from every kept one, until `branches` are kept (nb
 * of them).  Slot j < nb holds kept candidate j, a slot >= nb a copy of slot 0; with nb = 0 every slot is T[L-1] repeated.  Slot 0
 * is what ls_ngram_draft drafts from the same text.  F = 1 + branches * gamma nodes, the root first; node 1 + (d-1)*branches + j
 * is depth d = 1..gamma of branch j.
 *   all_spec  [b, F] int64 dense        [z, 1 + (d-1)*branches + j] = slot_j[d-1]; column 0 (the root) is kept
 *   tree_mask [b, F, F] int64 dense     rows 1.. in full: 1 at column 0 and at the nodes of the row's branch at depths <= its own,
 *                                       else 0; row 0 is kept
 *   info      [b, branches, 2] int32    (n, e) of the slot's candidate; (0, -1) for slots >= nb
 *   hist      [b, max_ngram+1] int64    hist[z, n of slot 0] += 1: comparable with ls_ngram_draft's; may be NULL
 *   hist_nb   [b, branches+1] int64     hist_nb[z, nb] += 1; may be NULL
 * Two launches, shaped like ls_ngram_draft's: (chunks of LS_NGRAM_CHUNK ends, b) workgroups leave their LS_NGRAM_TOP largest keys in
 * descending order, zero padded, as records of 8 bytes in the workspace (one pass over the text); one wave per row takes the row's
 * LS_NGRAM_TOP largest, loads the continuations, does the distinctness walk and writes everything above.  No atomics; every record
 * and every output is rewritten by every call: safe inside a replayed graph.  Exact.  LS_ERR_INVALID_ARG, before any launch: as
 * ls_ngram_draft, and branches outside 1..LS_NGRAM_TOP. */
#define LS_NGRAM_TOP 8
size_t ls_ngram_tree_workspace_bytes(int b, int64_t len_bound);      /* b * chunks * LS_NGRAM_TOP records of 8 bytes */
int ls_ngram_tree_draft(const int64_t* prompt_ids, int64_t prompt_stride_b, int prompt_cols, const int32_t* input_len,
                        const int64_t* output_ids, int64_t out_stride_b, int out_cap, const int32_t* written, int b, int64_t len_bound,
                        int gamma, int branches, int max_ngram, int min_ngram, int64_t* all_spec, int64_t* tree_mask, int32_t* info,
                        int64_t* hist, int64_t* hist_nb, void* workspace, size_t workspace_bytes, void* stream);

/* ls_logprob_topk and ls_argmax_rows with the lm_head SHARDED BY VOCABULARY over the ranks of a node (no counterpart in the reference, which
 * replicates: llama_glide.py:474).  A "record" is what stage 1 produces per (8192-logit chunk, row): the chunk's max, its sum of
 * exp(x - max) and its k largest logits with their GLOBAL columns -- rows * (2 + 2k) floats per chunk slot, chunk-major.
 *   ls_topk_stage1   this rank's slice logits_local [rows, vocab_local] (global columns col_base .. , col_base a multiple of
 *                    ls_topk_chunk()) -> records [nslots][rows][2 + 2k]; slots beyond the slice are written as empty records, so
 *                    that every rank can contribute the same number of slots to an all-gather;
 *   ls_topk_stage2   all ranks' slots in rank order = global chunk order -> the log-soft-max top-k (argmax = 0: out_vals [k],
 *                    out_idx [k] = row * vocab + column, history [rows] or NULL) or the per-row arg-max (argmax = 1: k = 1,
 *                    out_idx [rows], out_vals [rows] or NULL).
 * Bit-identical to ls_logprob_topk / ls_argmax_rows on the gathered logits for any number of ranks. */
int ls_topk_chunk(void);
int ls_topk_stage1(const void* logits_local, int rows, int vocab_local, int64_t ld, int dtype, int k, int col_base, int nslots,
                   float* records, void* stream);
int ls_topk_stage2(const float* records, int rows, int vocab, int k, int nslots, const float* history, int argmax, float* out_vals,
                   int64_t* out_idx, void* stream);

/* ---- beam-tree bookkeeping of a round (K10) ----------------------------------------------
 * The reference spells these steps as a few dozen tiny tensor ops per round
 * (longspec/test/llama_glide.py:1019-1121); each is one launch here, one workgroup per batch row. */

/* One more tree level (llama_glide.py:1021-1027 for the root's children, :1056-1075 deeper): new node
 * mid+j (j < k) is the child of node  lo + topk_idx[j] / vocab  and carries token  topk_idx[j] % vocab:
 *   all_spec[mid+j] = token;  logp_sum[mid+j] = topk_vals[j];
 *   tree_mask[mid+j, :] = tree_mask[father, :] + I[mid+j, :]          (the gather + diag_one of :1066-1067)
 * tree_mask [b,F,F] int64, all_spec [b,F] int64, logp_sum [b,F] fp32, topk_vals [b,k] fp32, topk_idx [b,k] int64.
 * positions [b,k] int64 / bits [b,k,words] (both or neither): what ls_tree_positions / ls_pack_tree_mask give
 * on tree_mask[mid:mid+k, :mid+k] for the draft pass over the new level, with base + base_add as the cache
 * length.  base [b] int32 (nullable) is advanced by base_add in place (`draft_cache_lens += acc - 1`, :1027). */
int ls_tree_grow(int64_t* tree_mask, int64_t* all_spec, float* logp_sum, const float* topk_vals,
                 const int64_t* topk_idx, int b, int F, int k, int64_t vocab, int lo, int mid,
                 int32_t* base, int base_add, int64_t* positions, uint32_t* bits, int words, void* stream);

/* Inputs of the verification pass (llama_glide.py:1078-1086).  R rows = [a accepted | F-1 tree nodes | pads]:
 *   veri_spec [b,R] int64 = [acc_ids[:a], all_spec[1:], 0...]        (acc_ids row stride acc_stride)
 *   mask = tril(ones(R,R)); mask[a:a+F-1, a:a+F-1] = tree_mask[1:,1:]; mask = tril(mask)
 *   positions [b,R] int64 = cache_lens + mask.sum(-1) - 1 (llama.py:575-577); bits [b,R,words] = mask != 0.
 * bump [b] int32 (nullable) += bump_add: the `draft_cache_lens += 1` of :1076. */
int ls_tree_verify_inputs(const int64_t* acc_ids, int64_t acc_stride, int a, const int64_t* all_spec,
                          const int64_t* tree_mask, int b, int F, int R, const int32_t* cache_lens,
                          int64_t* veri_spec, int64_t* positions, uint32_t* bits, int words,
                          int32_t* bump, int bump_add, void* stream);

/* LlamaGlide.tree_verification (longspec/test/llama_glide.py:1128-1175): all_spec/all_llm_pred [b,F]
 * int64, tree_mask [b,F,F] int64 (entries >= 0), cache_lens [b] int32 (+ cache_len_add = the `acc - 1`
 * of :1104).  Outputs: acc_ids [b,max_acc] int64 zero-padded, acc_num [b] int64, double_input [b] int32,
 * index_mapping [b,max_acc] int64 (-1 padded).  Moves the LAST target layer's KV rows
 * len+index_mapping[j] -> len+j (j < acc_num) in the same launch (k_cache NULL: no move). */
int ls_tree_collapse(const int64_t* all_spec, const int64_t* all_llm_pred, const int64_t* tree_mask,
                     const int32_t* cache_lens, int cache_len_add, int b, int F, int non_leaf_len, int max_acc,
                     int64_t* acc_ids, int64_t* acc_num, int32_t* double_input, int64_t* index_mapping,
                     void* k_cache, void* v_cache, int64_t kc_stride_b, int64_t kc_stride_s,
                     int row_elems, int dtype, void* stream);

/* LlamaGlide.verify_stochastic (longspec/test/llama_glide.py:1177-1245), temperature > 0: the speculative-sampling walk down
 * the draft tree, one workgroup per batch row.  all_spec [b,F] int64, tree_mask [b,F,F] int64, llm_logits [b,F,V] dtype
 * (target logits; strides in elements), spec_logp [b,Fs,V] fp32 (draft log-probs of the non-leaf nodes).  The reference
 * draws from Python's `random` and from torch.multinomial; both streams are handed in pre-drawn:
 *   mt_words [b,n_words] uint32 = the next raw outputs of Python's Mersenne Twister (random.getrandbits(32)): one word per
 *     random.choice attempt (>> (32 - bit_length(len))), two per random.random();  words_used [b] int32 = how many the walk
 *     consumed (-1: the buffer was too short) so that the host can re-synchronise its generator;
 *   exp_noise [b,V] dtype = torch.empty(V).exponential_(1): multinomial(p, 1) is argmax(p / noise) (ATen's one-sample path).
 * acc_ids [b,max_acc] int64 zero padded (max_acc >= tree depth + 2), acc_num [b] int64; workspace: b*V floats.
 * Kept from the reference on purpose: the acceptance ratio of child NODE s reads both distributions at vocabulary index s
 * (:1222); target probabilities are rounded to dtype after every operation (:1186,1231-1235).
 * LS_ERR_INVALID_ARG, before any launch: V < F (vocabulary index s of a child node would be out of range; the reference
 * raises an IndexError there), max_acc outside 2..15, n_words < 3, temperature <= 0. */
int ls_tree_verify_stochastic(const int64_t* all_spec, const int64_t* tree_mask, const void* llm_logits, int64_t logits_stride_b,
                              int64_t logits_stride_r, const float* spec_logp, int64_t logp_stride_b, int64_t logp_stride_r,
                              int b, int F, int Fs, int V, int dtype, float temperature, const uint32_t* mt_words, int n_words,
                              const void* exp_noise, int64_t* acc_ids, int max_acc, int64_t* acc_num, int32_t* words_used,
                              float* workspace, void* stream);

/* End of the round (llama_glide.py:1093-1121): output_ids[z, emitted + j] = acc_ids[z, j] (j < acc_num);
 * state[z] = (acc_num, any(output_ids[z, :out_cap] == eos)) for the round's single host read; the tree
 * state reset (tree_mask = 0, column 0 = 1; all_spec = 0, all_spec[0] = last accepted id; logp_sum = 0);
 * target_lens [b] int32 += target_add and draft_kv_lens [b] int32 += acc_num (both nullable).
 * emitted_dev [b] int32 (nullable): when given, the write offset is read from it instead of `emitted` and
 * advanced by acc_num -- a round replayed from a HIP graph carries no host-side integers. */
int ls_tree_commit(const int64_t* acc_ids, const int64_t* acc_num, int b, int max_acc, int64_t* output_ids,
                   int64_t out_stride, int out_cap, int emitted, int32_t* emitted_dev, int has_eos, int64_t eos,
                   int64_t* state, int64_t* tree_mask, int64_t* all_spec, float* logp_sum, int F,
                   int32_t* target_lens, int target_add, int32_t* draft_kv_lens, void* stream);

/* End of a round at temperature > 0 (llama_glide.py:1094-1121), what follows verify_stochastic, in one launch:
 *   output_ids[z, c + j] = acc_ids[z, j] for ALL j < max_acc (the zero padding too), c = cache_lens[z] - input_len[z]
 *     (cache_lens was advanced by `temp_input_len - 1` only, :1094: the next round overwrites part of this one);
 *   draft_kv_lens [b] int32 += acc_num (:1110); the tree state reset of ls_tree_commit (:1113-1116);
 *   acc_pad [b,pad_width] int64 = acc_ids, zero padded (the next round's draft step 0 reads it; may be acc_ids itself);
 *   state [b,4] int64 = (acc_num, any(output_ids[z, :out_cap] == eos) (:1120), words_used[z] as ls_tree_verify_stochastic
 *     left it (-1: the pre-drawn words ran out), cache_lens + acc_num - input_len + budget_add > out_cap (:1118, budget_add =
 *     gamma + 2)) -- the round's single host read.
 * cache_lens itself is not changed and the accepted KV rows are not compacted, as in the reference's T > 0 branch. */
int ls_tree_commit_stochastic(const int64_t* acc_ids, const int64_t* acc_num, const int32_t* words_used, int b, int max_acc,
                              int64_t* output_ids, int64_t out_stride, int out_cap, const int32_t* cache_lens,
                              const int32_t* input_len, int budget_add, int has_eos, int64_t eos, int64_t* state,
                              int64_t* tree_mask, int64_t* all_spec, float* logp_sum, int F, int32_t* draft_kv_lens,
                              int64_t* acc_pad, int pad_width, void* stream);

/* End of a chain-speculation round (spec_generate, llama_glide.py:738-770), gamma draft tokens:
 *   verification = cumprod(llm[:, :-1] == spec[:, 1:]); correct_len = sum + 1; llm[:, 1:] *= verification;
 *   output_ids[z, base+1 .. base+gamma] = llm[z, :gamma]; output_ids[z, base+correct_len] = bonus = llm[z, correct_len-1]
 *   (base = cache_lens - input_len); cache_lens += correct_len; draft_cache_lens = cache_lens - (correct_len == gamma+1);
 *   next_spec_start_token [b,2] = (llm[correct_len-2], llm[correct_len-1]) when every draft was accepted, else [0] = bonus;
 *   spec_buffer[z,0] = bonus; state [b,2] = (correct_len, any(output_ids[z, :base+correct_len+2] == eos)).
 * llm_verify_output / spec_buffer [b, gamma+1] int64 (both updated in place), lengths int32.
 * accept_mask [b, gamma] int64 or NULL: at temperature > 0 the verification is the cumulative product of the rejection-
 * sampling verdicts (:725-732) instead of the token comparison (:738). */
int ls_chain_commit(int64_t* llm_verify_output, int64_t* spec_buffer, int b, int gamma, int64_t* output_ids,
                    int64_t out_stride, int out_cap, int32_t* cache_lens, int32_t* draft_cache_lens,
                    const int32_t* input_len, int64_t* next_spec_start_token, int has_eos, int64_t eos,
                    int64_t* state, const int64_t* accept_mask, void* stream);

/* `embed_tokens(ids)` of a short pass (llama.py:579, llama_glide.py:1003,1030): out [n,hidden] =
 * table[ids] (table [vocab,hidden] dtype, ids int64 inside the vocabulary). */
int ls_embed_rows(const void* table, int64_t vocab, int hidden, int dtype, const int64_t* ids, int n,
                  void* out, void* stream);

/* Head of a decode pass in one launch: `embed_tokens(ids)` (llama.py:579, llama_glide.py:1003,1030) + the pass's RoPE table
 * (LlamaRotaryEmbedding.forward, llama.py:580 / llama_glide.py:1005-1006,1032-1033) + the first decoder layer's
 * `input_layernorm` (llama.py:487 via LlamaDecoderLayer.forward, llama_glide.py:437).  Bit-identical to
 * ls_embed_rows + ls_rope_cos_sin + ls_rmsnorm_fwd (the same device code); rows <= 128.
 *   ids [rows] int64; position of row i = positions[i] (int64) if given, else pos_base[i / q_len] + i % q_len + pos_add
 *   (int32 lengths on the device: `arange(q_len) + cache_lens[:, None]`);
 *   embeds [rows,hidden] = table[ids] (the residual stream), normed [rows,hidden] = RMSNorm(embeds) * norm_weight,
 *   cosv / sinv [rows,128]. */
int ls_pass_head(const void* table, int64_t vocab, int hidden, int dtype, const int64_t* ids, int rows,
                 const int64_t* positions, const int32_t* pos_base, int q_len, int pos_add, const float* inv_freq,
                 float attention_scaling, const void* norm_weight, float eps, void* embeds, void* normed, void* cosv,
                 void* sinv, void* stream);

/* ---- multi-GPU: peer exchange of the per-rank attention records -----------------
 * Replaces the one all-gather per attention call of a sequence-sharded prefix (the reference has no counterpart:
 * `device_map="auto"`, llama_glide.py:474) by peer stores into IPC-mapped mailboxes + flags, so that a decode round
 * containing it is pure kernel launches and replays from a HIP graph.  One object per process (= per GPU).
 *   create  -> handle (64 bytes, exchanged between the ranks by the host: torch.distributed, a pipe, ...)
 *           -> connect (all `world` handles in rank order; opens the peers' mailboxes)
 *           -> all_gather any number of times; every rank issues the same sequence of calls
 *   all_gather: gathered[r*stride_floats .. +n_floats) = rank r's `record` (n_floats <= cap_floats, multiples of 4,
 *   16-byte aligned).  Two launches on `stream`, no host synchronisation.  A peer that never delivers makes the
 *   wait give up after seconds and latches `timed_out` (ls_xchg_status; the gathered data is then invalid). */
#define LS_XCHG_MAX_WORLD 16
#define LS_XCHG_HANDLE_BYTES 64
typedef struct ls_xchg ls_xchg;
int ls_xchg_create(int rank, int world, size_t cap_floats, ls_xchg** out);
int ls_xchg_handle(ls_xchg* x, void* handle /* LS_XCHG_HANDLE_BYTES */);
int ls_xchg_connect(ls_xchg* x, const void* handles /* world * LS_XCHG_HANDLE_BYTES, rank order */);
int ls_xchg_all_gather(ls_xchg* x, const float* record, size_t n_floats, float* gathered, size_t stride_floats, void* stream);
int ls_xchg_status(ls_xchg* x, uint64_t* epoch, int* timed_out); /* synchronising; diagnostics only */
/* How long a wait polls before it gives up (default about 1 s; rank skew on a node is milliseconds).  Ranks that SHARE
 * one GPU (tests) stall each other for whole scheduling quanta and need tens of seconds.  Synchronising. */
int ls_xchg_set_timeout(ls_xchg* x, double seconds);
/* The same exchange fused into the two combine kernels of a sharded attention call: ls_attn_reduce_push =
 * ls_attn_reduce_local whose record goes straight into the peers' mailboxes (+ flags); ls_attn_finish_xchg =
 * ls_attn_finish over the mailbox slots of this exchange, read once every rank's flag is up.  One exchange =
 * one reduce_push followed by one finish_xchg on every rank (3 launches per attention call, 2 without a shard). */
int ls_attn_reduce_push(const ls_attn_desc* d, void* workspace, size_t workspace_bytes, ls_xchg* x, void* stream);
int ls_attn_finish_xchg(const ls_attn_desc* d, ls_xchg* x, void* workspace, size_t workspace_bytes, void* stream);
int ls_xchg_destroy(ls_xchg* x);

#ifdef __cplusplus
}
#endif
#endif /* LONGSPEC_HIP_H */
