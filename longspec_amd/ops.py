"""Operator layer: torch tensors in, HIP kernels (through the C ABI) out.

One function per reference seam of the draft-then-verify round:

  kvcache_attention      flash_attn_with_kvcache   longspec/test/llama.py:324,385, llama_glide.py:261,265,297,300
  verify_attention       LlamaAttention.tree_decoding + tree_part_fwd + merge   llama.py:385-387,394-421
  draft_tree_attention   GlideAttention.tree_decoding (self-attn) + triton_tree_part_fwd  llama_glide.py:300-329
  tree_attention         triton_tree_attn.attention   triton_tree_attn.py:19-77
  rmsnorm / rope_*       LlamaRMSNorm / LlamaRotaryEmbedding / apply_rotary_pos_emb (transformers)
  tree_collapse          LlamaGlide.tree_verification  llama_glide.py:1128-1175
  lse_merge              N-way form of llama.py:385-387,420 for sequence-sharded prefix KV
  logprob_topk / argmax_rows   beam growth and greedy verification on the lm_head logits  llama_glide.py:1019-1064,1091
                         (logp_out=: the draft's log-prob table of the temperature > 0 rounds, :1025,1074)
  sample_rows            one draw per row from the target's tempered, top-k / top-p / min_p / typical_p filtered distribution (sampling=;
                         no counterpart in the reference)
  penalize_rows / token_state_add   repetition / presence / frequency penalties and a logit bias on the target's logits, per
                         row from that row's own history, and the [batch, vocab] state they read (penalties=; no counterpart)
  ngram_draft            the drafter of prompt-lookup speculation: the continuation of the most recent earlier occurrence of
                         the text's last tokens (lookup_generate; no counterpart)
  ngram_tree_draft       its tree drafter: up to `branches` distinct continuations as a level-major tree (lookup_generate(branches=))
  token_logprobs / logprob_commit   log-prob of every emitted token under the distribution it was taken from and the row's
                         top-n alternatives; the accepted rows' results -> the tokens' output columns (logprobs=; no counterpart)
  stop_scan / stop_ban_rows   stop tokens, stop sequences and min_tokens (stop=; no counterpart)
  ban_rows               banned sequences and no-repeat n-grams on the target's logits, per row from the committed text and the
                         row's ordered path (ban=; no counterpart)
  dry_rows               the DRY repetition penalty on the target's logits: an id loses the more the longer the repeat it would
                         extend, per row from the committed text and the row's ordered path (dry=; no counterpart)
  guide_rows / guide_advance   guided decoding: the tokens a DFA over token ids forbids in the state behind the row's path, and
                         the per-row committed state they start from (guide=; no counterpart)
  guide_lift (_hash / _cols / _check)   the classes of a vocabulary's tokens under a byte-level DFA, the set-up of a guide
                         (Guide.from_byte_dfa / Guide.from_regex with a device; no counterpart)
  tree_commit / tree_commit_stochastic   end of a round at temperature 0 / > 0  llama_glide.py:1093-1121
  linear / linear_multi / mlp_gate_up   the projections of a decode pass (M <= 80 token rows):
                         q/k/v/o_proj llama.py:361-363,390, LlamaMLP (qwen2.py:218-230), lm_head llama_glide.py:1091
                         -- with 16-bit (pack_weight), 8-bit e4m3 (pack_weight8) or 4-bit MXFP4 (pack_weight4) packed weights

Everything runs on the CURRENT torch stream, without host synchronisation.  There is
no fallback: a missing extension or a CPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os
import math
from types import SimpleNamespace
from typing import Optional, Tuple

import torch

from . import _C
from ._C import LS_F16, LS_NEW_DRAFT, LS_NEW_FLASH, LS_NEW_NONE, LS_NEW_TARGET, AttnDesc

_DT = {torch.float16: _C.LS_F16, torch.bfloat16: _C.LS_BF16}


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """Raw hipStream_t of torch's current stream (the C accessors when this torch has them: the public
    torch.cuda.current_stream() costs ~8 us of Python per call, twice per operator)."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _dtype(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype} (fp16/bf16 only)") from None


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("longspec_amd ops run on the GPU only (no CPU path): got a CPU tensor")


class _Workspace:
    """Per-device scratch for split-KV partials, grown on demand.  Calls on one stream are
    ordered, so one buffer per (device, stream) is reused by every call."""

    def __init__(self):
        self._buf = {}

    def get(self, device, nbytes: int) -> torch.Tensor:
        key = (device.index, _stream())
        buf = self._buf.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
            self._buf[key] = buf
        return buf


_ws = _Workspace()
_causal_bits = {}


class _ZeroedWorkspace:
    """Scratch of the skinny-GEMM kernel (slab counters + split-K partials).  Zero-filled once when
    (re)allocated; every launch leaves its counters zero again (include/longspec_hip.h)."""

    def __init__(self):
        self._buf = {}

    def get(self, device, nbytes: int, stream: Optional[int] = None) -> torch.Tensor:
        key = (device.index, _stream() if stream is None else stream)
        buf = self._buf.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.zeros(max(nbytes, 32 << 20), dtype=torch.uint8, device=device)
            self._buf[key] = buf
        return buf


_gemm_ws = _ZeroedWorkspace()


def workspace_tensors():
    """The scratch buffers currently handed out (a captured HIP graph keeps them alive: it holds their addresses)."""
    return (list(_ws._buf.values()) + list(_gemm_ws._buf.values()) + list(_sample_ws._buf.values())
            + list(_logprob_ws._buf.values()) + list(_ngram_ws._buf.values()) + list(_ngram_tree_ws._buf.values()))


_linear_need = {}            # (shape key) -> workspace bytes of the launch plan
LINEAR_MAX_ROWS = 80


def linear_supported(x: torch.Tensor, in_features: int) -> bool:
    """True when the weight-streaming kernel takes this shape; otherwise the caller has a plain library
    GEMM on its hands (prefill: M in the thousands), which is hipBLASLt's job, not this kernel's."""
    rows = x.numel() // x.shape[-1]
    return x.is_cuda and x.dtype in _DT and 1 <= rows <= LINEAR_MAX_ROWS and in_features % 64 == 0 and in_features >= 128


class PackedWeight:
    """An ``nn.Linear.weight`` [N, K] re-laid-out once by ``ls_linear_pack_weight`` into the MFMA A-operand
    order the skinny kernel streams (include/longspec_hip.h).  ``data`` is a flat tensor of the weight's
    dtype with ceil(N/16)*16*K elements."""
    __slots__ = ("data", "n", "k", "dtype", "rope")

    def __init__(self, data, n, k):
        self.data, self.n, self.k, self.dtype, self.rope = data, n, k, data.dtype, False


def pack_weight(weight: torch.Tensor, rope: bool = False) -> PackedWeight:
    """``rope=True``: a q_proj / k_proj weight [heads*128, K] for ``linear_qkv_rope`` (rotary pairs in neighbouring tiles)."""
    _dev(weight)
    if weight.dim() != 2 or weight.shape[1] % 32 != 0:
        raise ValueError("pack_weight: [N, K] weight with K a multiple of 32 expected")
    w = weight.detach().contiguous()
    N, K = w.shape
    lib = _C.load()
    nbytes = lib.ls_linear_packed_bytes(N, K)
    out = torch.empty(nbytes // 2, dtype=w.dtype, device=w.device)
    if rope:
        _C.check(lib.ls_linear_pack_rope(w.data_ptr(), out.data_ptr(), N, K, _dtype(w), _stream()), "ls_linear_pack_rope")
    else:
        _C.check(lib.ls_linear_pack_weight(w.data_ptr(), out.data_ptr(), N, K, _dtype(w), _stream()), "ls_linear_pack_weight")
    pw = PackedWeight(out, N, K)
    pw.rope = rope
    return pw


def pack_gate_up(gate_weight: torch.Tensor, up_weight: torch.Tensor) -> PackedWeight:
    """gate_proj / up_proj of one MLP as one packed matrix with alternating 16-row tiles (operand of mlp_gate_up)."""
    _dev(gate_weight, up_weight)
    if gate_weight.shape != up_weight.shape or gate_weight.dim() != 2 or gate_weight.shape[0] % 16 or gate_weight.shape[1] % 32:
        raise ValueError("pack_gate_up: two [N, K] weights with N % 16 == 0 and K % 32 == 0 expected")
    g, u = gate_weight.detach().contiguous(), up_weight.detach().contiguous()
    N, K = g.shape
    lib = _C.load()
    out = torch.empty(lib.ls_linear_packed_bytes(2 * N, K) // 2, dtype=g.dtype, device=g.device)
    _C.check(lib.ls_linear_pack_gate_up(g.data_ptr(), u.data_ptr(), out.data_ptr(), N, K, _dtype(g), _stream()),
             "ls_linear_pack_gate_up")
    return PackedWeight(out, N, K)


class PackedWeight8:
    """A weight [N, K] as OCP e4m3fn bytes in the streamed 8-bit layout (``ls_linear_w8_pack``, include/longspec_hip.h)
    plus one fp32 scale per row: ``W[n, k] = q[n, k] * scale[n]``.  ``data`` is a flat uint8 tensor of ceil(N/64)*64*K
    bytes; ``scale`` is [N] (a gate/up pair: [2, N], gate rows first).  ``dtype`` is always ``torch.uint8``: the
    activation dtype is the caller's."""
    __slots__ = ("data", "scale", "n", "k", "dtype", "rope", "pair")

    def __init__(self, data, scale, n, k, rope=False, pair=False):
        self.data, self.scale, self.n, self.k, self.dtype, self.rope, self.pair = data, scale, n, k, torch.uint8, rope, pair


W8_CALLS = 0          # launches of ls_linear_w8_fwd so far (tests assert that a quantised model really streams 8-bit weights)


def quantize_rows_e4m3(weight: torch.Tensor, pow2: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """Device twin of ``quant.quantize_rows_e4m3`` (bit-identical): fp16 / bf16 [N, K] -> (q uint8 [N, K], scale fp32 [N])."""
    _dev(weight)
    if weight.dim() != 2 or weight.shape[1] % 8 != 0:
        raise ValueError("quantize_rows_e4m3: [N, K] weight with K a multiple of 8 expected")
    w = weight.detach().contiguous()
    N, K = w.shape
    q = torch.empty((N, K), dtype=torch.uint8, device=w.device)
    scale = torch.empty((N,), dtype=torch.float32, device=w.device)
    _C.check(_C.load().ls_linear_w8_quantize(w.data_ptr(), N, K, _dtype(w), int(bool(pow2)), q.data_ptr(), scale.data_ptr(), _stream()),
             "ls_linear_w8_quantize")
    return q, scale


def _as_q_scale(weight):
    """``weight``: a 16-bit [N, K] tensor (quantised here, power-of-two scales) or a pre-quantised ``(q uint8 [N, K],
    scale fp32 [N])`` pair (any positive scales: a checkpoint quantised elsewhere)."""
    if isinstance(weight, (tuple, list)):
        q, scale = weight
        _dev(q, scale)
        if q.dtype != torch.uint8 or q.dim() != 2 or scale.numel() != q.shape[0]:
            raise ValueError("pack_weight8: a pre-quantised weight is (q uint8 [N, K], scale [N])")
        return q.contiguous(), scale.detach().to(torch.float32).reshape(-1).contiguous()
    return quantize_rows_e4m3(weight)


def pack_weight8(weight, rope: bool = False) -> PackedWeight8:
    """Quantise (unless ``weight`` is already a ``(q, scale)`` pair) and pack for the 8-bit skinny GEMM.  ``rope=True``:
    the q/k layout of ``linear_qkv_rope``."""
    q, scale = _as_q_scale(weight)
    N, K = q.shape
    if K % 64 != 0 or K < 128 or (rope and N % 128 != 0):
        raise ValueError("pack_weight8: K must be a multiple of 64 (>= 128); rope=True needs N = heads x 128")
    lib = _C.load()
    out = torch.empty(lib.ls_linear_w8_packed_bytes(N, K), dtype=torch.uint8, device=q.device)
    _C.check(lib.ls_linear_w8_pack(q.data_ptr(), None, out.data_ptr(), N, K, int(rope), _stream()), "ls_linear_w8_pack")
    return PackedWeight8(out, scale, N, K, rope=rope)


def pack_gate_up8(gate_weight, up_weight) -> PackedWeight8:
    """gate_proj / up_proj of one MLP (16-bit tensors or ``(q, scale)`` pairs) as one 8-bit packed matrix with alternating
    16-row tiles: the operand of ``mlp_gate_up``."""
    (qg, sg), (qu, su) = _as_q_scale(gate_weight), _as_q_scale(up_weight)
    if qg.shape != qu.shape or qg.shape[0] % 16 or qg.shape[1] % 64 or qg.shape[1] < 128:
        raise ValueError("pack_gate_up8: two [N, K] weights with N % 16 == 0 and K % 64 == 0 expected")
    N, K = qg.shape
    lib = _C.load()
    out = torch.empty(lib.ls_linear_w8_packed_bytes(2 * N, K), dtype=torch.uint8, device=qg.device)
    _C.check(lib.ls_linear_w8_pack(qg.data_ptr(), qu.data_ptr(), out.data_ptr(), N, K, 0, _stream()), "ls_linear_w8_pack")
    return PackedWeight8(out, torch.stack([sg, su]).contiguous(), N, K, pair=True)


class PackedWeight4:
    """A weight [N, K] as OCP MX FP4 (e2m1 nibbles, one e8m0 scale byte per 32 k of a row) in the streamed 4-bit layout
    (``ls_linear_w4_pack``, include/longspec_hip.h): ``data`` is a flat uint8 tensor of ceil(N/64) * (K/64) * 2176 bytes
    that holds the scale bytes too.  ``dtype`` is always ``torch.uint8``: the activation dtype is the caller's."""
    __slots__ = ("data", "n", "k", "dtype", "rope", "pair")

    def __init__(self, data, n, k, rope=False, pair=False):
        self.data, self.n, self.k, self.dtype, self.rope, self.pair = data, n, k, torch.uint8, rope, pair


W4_CALLS = 0          # launches of ls_linear_w4_fwd so far (tests assert that a quantised model really streams 4-bit weights)


def quantize_blocks_mxfp4(weight: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Device twin of ``quant.quantize_blocks_mxfp4`` (bit-identical): fp16 / bf16 [N, K] -> (q uint8 [N, K/2], e uint8
    [N, K/32])."""
    _dev(weight)
    if weight.dim() != 2 or weight.shape[1] % 32 != 0 or weight.shape[1] == 0:
        raise ValueError("quantize_blocks_mxfp4: [N, K] weight with K a multiple of 32 expected")
    w = weight.detach().contiguous()
    N, K = w.shape
    q = torch.empty((N, K // 2), dtype=torch.uint8, device=w.device)
    e = torch.empty((N, K // 32), dtype=torch.uint8, device=w.device)
    _C.check(_C.load().ls_linear_w4_quantize(w.data_ptr(), N, K, _dtype(w), q.data_ptr(), e.data_ptr(), _stream()),
             "ls_linear_w4_quantize")
    return q, e


def _as_q_e(weight):
    """``weight``: a 16-bit [N, K] tensor (quantised here) or a pre-quantised ``(q uint8 [N, K/2], e uint8 [N, K/32])`` pair
    (an MXFP4 checkpoint quantised elsewhere; its exponent bytes must lie in [114, 140], ``ls_linear_w4_pack`` checks)."""
    if isinstance(weight, (tuple, list)):
        q, e = weight
        _dev(q, e)
        if (q.dtype != torch.uint8 or e.dtype != torch.uint8 or q.dim() != 2 or e.dim() != 2 or q.shape[0] != e.shape[0]
                or q.shape[1] != e.shape[1] * 16):
            raise ValueError("pack_weight4: a pre-quantised weight is (q uint8 [N, K/2], e uint8 [N, K/32])")
        return q.contiguous(), e.contiguous()
    return quantize_blocks_mxfp4(weight)


def pack_weight4(weight, rope: bool = False) -> PackedWeight4:
    """Quantise (unless ``weight`` is already a ``(q, e)`` pair) and pack for the 4-bit skinny GEMM.  ``rope=True``: the
    q/k layout of ``linear_qkv_rope``."""
    q, e = _as_q_e(weight)
    N, K = q.shape[0], q.shape[1] * 2
    if K % 64 != 0 or K < 128 or (rope and N % 128 != 0):
        raise ValueError("pack_weight4: K must be a multiple of 64 (>= 128); rope=True needs N = heads x 128")
    lib = _C.load()
    out = torch.empty(lib.ls_linear_w4_packed_bytes(N, K), dtype=torch.uint8, device=q.device)
    _C.check(lib.ls_linear_w4_pack(q.data_ptr(), e.data_ptr(), None, None, out.data_ptr(), N, K, int(rope), _stream()),
             "ls_linear_w4_pack")
    return PackedWeight4(out, N, K, rope=rope)


def pack_gate_up4(gate_weight, up_weight) -> PackedWeight4:
    """gate_proj / up_proj of one MLP (16-bit tensors or ``(q, e)`` pairs) as one 4-bit packed matrix with alternating
    16-row tiles: the operand of ``mlp_gate_up``."""
    (qg, eg), (qu, eu) = _as_q_e(gate_weight), _as_q_e(up_weight)
    if qg.shape != qu.shape or qg.shape[0] % 16 or qg.shape[1] % 32 or qg.shape[1] < 64:
        raise ValueError("pack_gate_up4: two [N, K] weights with N % 16 == 0 and K % 64 == 0 (>= 128) expected")
    N, K = qg.shape[0], qg.shape[1] * 2
    lib = _C.load()
    out = torch.empty(lib.ls_linear_w4_packed_bytes(2 * N, K), dtype=torch.uint8, device=qg.device)
    _C.check(lib.ls_linear_w4_pack(qg.data_ptr(), eg.data_ptr(), qu.data_ptr(), eu.data_ptr(), out.data_ptr(), N, K, 0, _stream()),
             "ls_linear_w4_pack")
    return PackedWeight4(out, N, K, pair=True)


# ---- what the wrappers of the logit-rule operators share.  Plain functions of tensor metadata: none touches the device or the
# library, and ``who`` is the operator's name in the messages (csrc/rule_rows.h is the same conventions behind the C ABI).

def _rows16(x: torch.Tensor, unit_batch_free: bool = False) -> torch.Tensor:
    """``x`` [rows, V] or [b, R, V] as the kernels load it, 16 bytes at a time -- unit column stride, row strides multiples of 8
    elements, the first element 16-byte aligned -- or a contiguous copy.  ``unit_batch_free``: a batch of 1 may have any batch
    stride (``logprob_topk`` launches per batch row)."""
    lead = x.stride()[1 if unit_batch_free and x.shape[0] == 1 else 0:-1]
    if x.stride(-1) != 1 or any(s % 8 != 0 for s in lead) or x.data_ptr() % 16 != 0:
        x = x.contiguous()
    return x


def _rule_rows(logits: torch.Tensor, who: str):
    """Logits an operator rewrites IN PLACE: 16-bit [b, V] or [b, R, V] with unit column stride and rows that do not overlap ->
    (the [b, R, V] view, b, R, V).  The row stride to pass is ``max(x.stride(1), V)`` (a single row may have any)."""
    if logits.dim() not in (2, 3) or logits.dtype not in _DT or logits.stride(-1) != 1:
        raise TypeError(f"{who}: logits must be fp16 / bf16 [b, V] or [b, R, V] with unit column stride")
    x = logits if logits.dim() == 3 else logits.unsqueeze(1)
    b, R, V = x.shape
    if (R > 1 and x.stride(1) < V) or (b > 1 and x.stride(0) < V):
        raise ValueError(f"{who}: overlapping rows")
    return x, b, R, V


def _extras(extra_ids, extra_mask, b: int, R: int, who: str, limit: Optional[int] = None):
    """A row's extras, ``extra_ids`` int64 [b, C] selected by ``extra_mask`` int64 [b, R, C] or [R, C] (one mask for the whole
    batch: batch stride 0) -> (ids_p, ids_sb, mask_p, mask_sb, mask_sr, C); no ids or C = 0: no extras.  ``limit``: the
    operator's column limit; an operator that has one also refuses a mask without ids."""
    if extra_ids is None or extra_ids.shape[-1] == 0:
        if limit is not None and extra_mask is not None and extra_ids is None:
            raise ValueError(f"{who}: extra_mask needs extra_ids")
        return None, 0, None, 0, 0, 0
    if extra_mask is None:
        raise ValueError(f"{who}: extra_ids needs extra_mask")
    C = extra_ids.shape[-1]
    if limit is not None and C > limit:
        raise ValueError(f"{who}: {C} extra columns, at most {limit}")
    if extra_ids.dtype != torch.int64 or extra_ids.dim() != 2 or extra_ids.shape[0] != b or extra_ids.stride(1) != 1:
        raise TypeError(f"{who}: extra_ids must be int64 [b, C] with contiguous rows")
    if extra_mask.dtype != torch.int64 or extra_mask.dim() not in (2, 3) or extra_mask.stride(-1) != 1 \
            or tuple(extra_mask.shape[-2:]) != (R, C) or (extra_mask.dim() == 3 and extra_mask.shape[0] != b):
        raise TypeError(f"{who}: extra_mask must be int64 [b, R, C] or [R, C] with unit column stride")
    return (extra_ids.data_ptr(), extra_ids.stride(0), extra_mask.data_ptr(), extra_mask.stride(0) if extra_mask.dim() == 3 else 0,
            extra_mask.stride(-2), C)


def _num(num, b: int, who: str):
    """``num`` int64 [b] with any stride, or None -> (num_p, num_s)."""
    if num is None:
        return None, 0
    if num.dtype != torch.int64 or num.numel() != b or num.dim() != 1:
        raise TypeError(f"{who}: num must be int64 [b]")
    return num.data_ptr(), num.stride(0)


def _id_rows(ids: torch.Tensor, b: int, who: str, most: Optional[int] = None) -> torch.Tensor:
    """``ids`` int64 [b, n] (or flat, b * n) with unit column stride, copied when it has another; ``most``: 1 <= n <= most."""
    if ids.dim() == 1:
        ids = ids.view(b, -1)
    if ids.dtype != torch.int64 or ids.dim() != 2 or ids.shape[0] != b:
        raise TypeError(f"{who}: ids must be int64 [b, n]")
    if most is not None and not (1 <= ids.shape[1] <= most):
        raise ValueError(f"{who}: {ids.shape[1]} ids per row, 1..{most}")
    if ids.shape[1] > 1 and ids.stride(1) != 1:
        ids = ids.contiguous()
    return ids


def _lp_buffers(triple, b: int, cols: int, n: int, who: str, names) -> None:
    """The three dense log-prob buffers of ``cols`` rows or columns: fp32 [b, cols], fp32 [b, cols, n], int64 [b, cols, n]."""
    for t, shape, dt, name in zip(triple, ((b, cols), (b, cols, n), (b, cols, n)), (torch.float32, torch.float32, torch.int64), names):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise TypeError(f"{who}: {name} must be a contiguous {dt} tensor of shape {shape}")


def _ngram_buffers(prompt_ids, output_ids, len_bound, info, info_tail, hists, who: str):
    """What the two n-gram drafters share: the text buffers (int64 [b, columns], unit column stride, rows apart), the host-side
    ``len_bound``, ``info`` int32 [b, *info_tail] (allocated when None) and the optional histograms ``hists`` = ((tensor, name,
    columns), ...), int64 [b, columns] -> (b, info)."""
    for t, name in ((prompt_ids, "prompt_ids"), (output_ids, "output_ids")):
        if t.dtype != torch.int64 or t.dim() != 2 or t.stride(1) != 1:
            raise TypeError(f"{who}: {name} must be int64 [b, columns] with contiguous rows")
    b = output_ids.shape[0]
    if prompt_ids.shape[0] != b or (b > 1 and (prompt_ids.stride(0) < prompt_ids.shape[1] or output_ids.stride(0) < output_ids.shape[1])):
        raise ValueError(f"{who}: prompt_ids and output_ids must have one row per batch row, rows apart")
    if int(len_bound) < 1:
        raise ValueError(f"{who}: len_bound={len_bound}")
    shape = (b,) + tuple(info_tail)
    if info is None:
        info = torch.empty(shape, dtype=torch.int32, device=output_ids.device)
    elif info.dtype != torch.int32 or tuple(info.shape) != shape or not info.is_contiguous():
        raise TypeError(f"{who}: info must be a contiguous int32 [{', '.join(map(str, shape))}] tensor")
    for t, name, cols in hists:
        if t is not None and (t.dtype != torch.int64 or tuple(t.shape) != (b, cols) or not t.is_contiguous()):
            raise TypeError(f"{who}: {name} must be a contiguous int64 [{b}, {cols}] tensor")
    return b, info


def logprob_topk(logits: torch.Tensor, history: Optional[torch.Tensor], k: int,
                 logp_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(logits.float().log_softmax(-1) + history[..., None]).view(bsz, -1).topk(k)`` (llama_glide.py:1019-1020,
    1046-1064) straight from the fp16 lm_head output: logits [bsz, rows, V], history [bsz, rows] fp32 or None ->
    (values [bsz, k] fp32 descending, flat indices [bsz, k] int64 = row * V + column).
    ``logp_out`` [bsz, rows, V] fp32 (a row slice of ``spec_logits``, :1025,1074): also receives
    ``logits.float().log_softmax(-1)``, written by the same launch sequence (``ls_logprob_topk_store``); the returned
    values and indices do not depend on it."""
    _dev(logits, history, logp_out)
    if logits.dim() == 2:
        logits = logits.unsqueeze(1)
    logits = _rows16(logits, unit_batch_free=True)
    b, R, V = logits.shape
    if logp_out is not None and (logp_out.dtype != torch.float32 or tuple(logp_out.shape) != (b, R, V) or logp_out.stride(-1) != 1):
        raise TypeError("logprob_topk: logp_out must be fp32 [bsz, rows, V] with a contiguous last dimension")
    if k > 64 or R > 128 or R * ((V + 8191) // 8192) * k > 5120 or R * ((V + 8191) // 8192) > 512 or V % 8:
        # beyond the fused kernel's candidate budget (trees wider than BASELINE's 16 per level): library kernels
        lp = logits.float().log_softmax(dim=-1)
        if logp_out is not None:
            logp_out.copy_(lp)
        if history is not None:
            lp = lp + history[:, :, None].float()
        return lp.view(b, -1).topk(dim=-1, k=k, largest=True, sorted=True)
    vals = torch.empty((b, k), dtype=torch.float32, device=logits.device)
    idx = torch.empty((b, k), dtype=torch.int64, device=logits.device)
    if history is not None:
        history = history.to(torch.float32).contiguous()
    lib = _C.load()
    need = lib.ls_topk_workspace_bytes(R, V, k)
    ws = _ws.get(logits.device, max(need, 1))
    for i in range(b):
        hist = history[i].data_ptr() if history is not None else None
        if logp_out is None:
            _C.check(lib.ls_logprob_topk(logits[i].data_ptr(), R, V, logits.stride(1), _dtype(logits), hist, k, vals[i].data_ptr(),
                                         idx[i].data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "ls_logprob_topk")
        else:
            _C.check(lib.ls_logprob_topk_store(logits[i].data_ptr(), R, V, logits.stride(1), _dtype(logits), hist, k,
                                               vals[i].data_ptr(), idx[i].data_ptr(), logp_out[i].data_ptr(), logp_out.stride(1),
                                               ws.data_ptr(), ws.numel(), _stream()), "ls_logprob_topk_store")
    return vals, idx


def argmax_rows(logits: torch.Tensor) -> torch.Tensor:
    """``logits.argmax(-1)`` for lm_head outputs [..., V] (first maximum), int64 [...]."""
    _dev(logits)
    shape = logits.shape[:-1]
    V = logits.shape[-1]
    x = _rows16(logits.reshape(-1, V))
    out = torch.empty((x.shape[0],), dtype=torch.int64, device=logits.device)
    lib = _C.load()
    need = lib.ls_topk_workspace_bytes(x.shape[0], V, 1)
    ws = _ws.get(logits.device, max(need, 1))
    _C.check(lib.ls_argmax_rows(x.data_ptr(), x.shape[0], V, x.stride(0), _dtype(x), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                _stream()), "ls_argmax_rows")
    return out.view(shape)


_sample_ws = _Workspace()    # its own buffer: a captured round holds its address, and other operators' growth must not move it


def sample_rows(logits: torch.Tensor, positions: torch.Tensor, sampling, streams: Optional[torch.Tensor] = None,
                return_top2: bool = False, return_upper: bool = False, cut=None):
    """One draw per row of lm_head outputs [..., V] from soft-max(x / T) under ``sampling``'s top-k / top-p
    (``ls_sample_rows``) and, where the object has them switched on, min_p / typical_p (``ls_sample_rows_ex``): int64 [...].  ``positions`` [...] int64 = absolute position of the token each row PREDICTS FROM
    (the position fed to RoPE for that row), ``streams`` [...] int32 = its batch row (None: 0) -- with the seed they key the
    noise, so a position draws the same noise in every loop.  ``return_top2``: also (top2_idx [..., 2], top2_key [..., 2],
    kept [...] int32, threshold [...] fp32 = the smallest kept value); ``return_upper`` appends upper [...] fp32, the largest
    kept value (below the row maximum where typical_p dropped it).  ``cut`` (``longspec_amd.Cut``, None: off): top_n_sigma and
    xtc on the same draw (``ls_sample_rows_cut``; ``longspec_amd/cut.py`` has the definitions); a ``Cut`` with both filters off
    is None."""
    _dev(logits, positions, streams)
    if cut is not None and not (cut.top_n_sigma > 0.0 or cut.xtc_probability > 0.0):
        cut = None
    min_p, typical_p = float(getattr(sampling, "min_p", 0.0)), float(getattr(sampling, "typical_p", 1.0))
    shape = logits.shape[:-1]
    V = logits.shape[-1]
    x = _rows16(logits.reshape(-1, V))
    n = x.shape[0]
    pos = positions.reshape(-1).to(torch.int64).contiguous()
    if pos.numel() != n:
        raise ValueError(f"sample_rows: {n} rows of logits, {pos.numel()} positions")
    strm = None
    if streams is not None:
        strm = streams.reshape(-1).to(torch.int32).contiguous()
        if strm.numel() != n:
            raise ValueError(f"sample_rows: {n} rows of logits, {strm.numel()} streams")
    dev = logits.device
    out = torch.empty((n,), dtype=torch.int64, device=dev)
    t2i = t2k = kept = thr = upper = None
    if return_upper:
        upper = torch.empty((n,), dtype=torch.float32, device=dev)
    if return_top2:
        t2i = torch.empty((n, 2), dtype=torch.int64, device=dev)
        t2k = torch.empty((n, 2), dtype=torch.float32, device=dev)
        kept = torch.empty((n,), dtype=torch.int32, device=dev)
        thr = torch.empty((n,), dtype=torch.float32, device=dev)
    lib = _C.load()
    ptr = lambda t: t.data_ptr() if t is not None else None
    if cut is None and min_p == 0.0 and typical_p == 1.0 and not return_upper:
        need = lib.ls_sample_workspace_bytes(n, V)
        ws = _sample_ws.get(dev, max(need, 1))
        _C.check(lib.ls_sample_rows(x.data_ptr(), n, V, x.stride(0), _dtype(x), pos.data_ptr(), ptr(strm), sampling.seed,
                                    sampling.temperature, sampling.top_k, sampling.top_p, out.data_ptr(), ptr(t2i), ptr(t2k),
                                    ptr(kept), ptr(thr), ws.data_ptr(), ws.numel(), _stream()), "ls_sample_rows")
    else:
        d = _C.SampleDesc(logits=x.data_ptr(), positions=pos.data_ptr(), streams=ptr(strm), out_idx=out.data_ptr(),
                          out_top2_idx=ptr(t2i), out_top2_key=ptr(t2k), out_kept=ptr(kept), out_threshold=ptr(thr),
                          out_upper=ptr(upper), ld=x.stride(0), seed=sampling.seed, rows=n, vocab=V, dtype=_dtype(x),
                          top_k=sampling.top_k, temperature=sampling.temperature, top_p=sampling.top_p, min_p=min_p,
                          typical_p=typical_p)
        if cut is None:
            need = lib.ls_sample_ex_workspace_bytes(C.byref(d))
            ws = _sample_ws.get(dev, max(need, 1))
            _C.check(lib.ls_sample_rows_ex(C.byref(d), ws.data_ptr(), ws.numel(), _stream()), "ls_sample_rows_ex")
        else:
            c = _C.SampleCut(top_n_sigma=cut.top_n_sigma, xtc_probability=cut.xtc_probability, xtc_threshold=cut.xtc_threshold,
                             reserved=0)
            need = lib.ls_sample_cut_workspace_bytes(C.byref(d), C.byref(c))
            ws = _sample_ws.get(dev, max(need, 1))
            _C.check(lib.ls_sample_rows_cut(C.byref(d), C.byref(c), ws.data_ptr(), ws.numel(), _stream()), "ls_sample_rows_cut")
    res = (out.view(shape),)
    if return_top2:
        res += (t2i.view(*shape, 2), t2k.view(*shape, 2), kept.view(shape), thr.view(shape))
    if return_upper:
        res += (upper.view(shape),)
    return res if len(res) > 1 else res[0]


def penalize_rows(logits: torch.Tensor, state: torch.Tensor, penalties, extra_ids: Optional[torch.Tensor] = None,
                  extra_mask: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """TARGET logits [b, V] or [b, R, V] rewritten under ``penalties`` (``longspec_amd.Penalties``) from each row's history
    (``ls_penalize_rows``): ``state`` [b, V] int32 (bits 0-30 = times generated, bit 31 = in the prompt) plus, for row r of
    batch z, every ``extra_ids[z, c]`` (int64 [b, C]) with ``extra_mask[z, r, c] != 0`` (int64 [b, R, C], or [R, C] = one mask
    for the whole batch).  ``bias``: ``penalties.bias_table(V, device)`` when the caller keeps it (the decode loops do: the
    table is not rebuilt per call, and never inside a graph capture); None: built here.  Returns a NEW contiguous tensor of the input's shape and dtype: what follows (``argmax_rows``,
    ``sample_rows``) reads it as it is, whatever the input aliased."""
    _dev(logits, state, extra_ids, extra_mask)
    shape = logits.shape
    V = shape[-1]
    if logits.dim() not in (2, 3):
        raise ValueError("penalize_rows: logits [b, V] or [b, R, V]")
    x = logits if logits.dim() == 3 else logits.unsqueeze(1)
    b, R = x.shape[0], x.shape[1]
    x = _rows16(x)
    if state.dtype != torch.int32 or tuple(state.shape) != (b, V) or state.stride(1) != 1:
        raise TypeError(f"penalize_rows: state must be int32 [{b}, {V}] with contiguous rows")
    ids_p, ids_sb, mask_p, mask_sb, mask_sr, C = _extras(extra_ids, extra_mask, b, R, "penalize_rows")
    out = torch.empty((b, R, V), dtype=x.dtype, device=x.device)
    if bias is None:
        bias = penalties.bias_table(V, x.device)
    elif bias.dtype != torch.float32 or tuple(bias.shape) != (V,) or not bias.is_contiguous() or bias.device != x.device:
        raise TypeError(f"penalize_rows: bias must be a contiguous fp32 [{V}] tensor on the logits' device")
    _C.check(_C.load().ls_penalize_rows(x.data_ptr(), out.data_ptr(), b, R, V, _dtype(x), x.stride(0), x.stride(1), out.stride(0),
                                        out.stride(1), state.data_ptr(), state.stride(0), ids_p, ids_sb, mask_p, mask_sb, mask_sr, C,
                                        penalties.repetition, penalties.presence, penalties.frequency,
                                        bias.data_ptr() if bias is not None else None, _stream()), "ls_penalize_rows")
    return out.view(shape)


def token_state_add(state: torch.Tensor, ids: torch.Tensor, num: Optional[torch.Tensor] = None, prompt: bool = False) -> None:
    """Update the penalty state [b, V] int32 in place (``ls_token_state_add``): every ``ids[z, j]`` (int64 [b, n]) with
    ``j < num[z]`` (``num`` [b] int64, None: all) inside the vocabulary adds 1 to its word's count, or -- ``prompt`` -- sets
    bit 31.  Ids outside [0, V) are ignored."""
    _dev(state, ids, num)
    if state.dtype != torch.int32 or state.dim() != 2 or state.stride(1) != 1:
        raise TypeError("token_state_add: state must be int32 [b, V] with contiguous rows")
    b, V = state.shape
    ids = _id_rows(ids, b, "token_state_add")
    num_p, num_s = _num(num, b, "token_state_add")
    _C.check(_C.load().ls_token_state_add(state.data_ptr(), b, V, state.stride(0), ids.data_ptr(), ids.shape[1], ids.stride(0),
                                          num_p, num_s, 1 if prompt else 0, _stream()), "ls_token_state_add")


_logprob_ws = _Workspace()   # its own buffer, as _sample_ws: a captured round holds its address
LOGPROB_MAX_ROWS, LOGPROB_MAX_N = 1024, 20      # the limits of ls_token_logprobs (rows x batch, top n)


def token_logprobs(logits: torch.Tensor, ids: torch.Tensor, temperature: float = 1.0, n: int = 0):
    """Log-prob of the chosen token of every row of TARGET logits [b, V] or [b, R, V] -- as the token was picked from them,
    i.e. behind ``penalize_rows`` -- and the row's top ``n`` (``ls_token_logprobs``): ``ids`` int64 [b] / [b, R].  In fp32,
    ``lp_j = (x_j - m) / temperature - ln sum_i exp((x_i - m) / temperature)`` over the full vocabulary.  Returns
    (row_lp [b, R] fp32, top_val [b, R, n] fp32, top_idx [b, R, n] int64): the n largest logits in (logit descending, column
    ascending) order; an id outside the vocabulary gives NaN, a short row is padded with (-inf, -1)."""
    _dev(logits, ids)
    if logits.dim() not in (2, 3):
        raise ValueError("token_logprobs: logits [b, V] or [b, R, V]")
    x = logits if logits.dim() == 3 else logits.unsqueeze(1)
    b, R, V = x.shape
    x = _rows16(x)
    if ids.dtype != torch.int64 or ids.numel() != b * R or ids.shape[0] != b:
        raise TypeError(f"token_logprobs: ids must be int64 [{b}, {R}]")
    ids = ids.view(b, R)
    if R > 1 and ids.stride(1) != 1:
        ids = ids.contiguous()
    dev = x.device
    row_lp = torch.empty((b, R), dtype=torch.float32, device=dev)
    top_val = torch.empty((b, R, n), dtype=torch.float32, device=dev)
    top_idx = torch.empty((b, R, n), dtype=torch.int64, device=dev)
    lib = _C.load()
    # sized once for the largest call the kernel takes at this vocabulary (3.3 MB at V = 128 256), not for this call: the
    # buffer of a stream never moves while the vocabulary stays, so a captured round's address stays the one later calls use
    need = lib.ls_token_logprobs_workspace_bytes(1, LOGPROB_MAX_ROWS, V, LOGPROB_MAX_N)
    ws = _logprob_ws.get(dev, max(need, 1))
    _C.check(lib.ls_token_logprobs(x.data_ptr(), b, R, V, _dtype(x), x.stride(0), x.stride(1), ids.data_ptr(), ids.stride(0),
                                   float(temperature), n, row_lp.data_ptr(), top_val.data_ptr() if n else None,
                                   top_idx.data_ptr() if n else None, ws.data_ptr(), ws.numel(), _stream()), "ls_token_logprobs")
    return row_lp, top_val, top_idx


def logprob_commit(rows, out, base: torch.Tensor, base_add: int = 0, num: Optional[torch.Tensor] = None,
                   index_map: Optional[torch.Tensor] = None) -> None:
    """The accepted rows of ``rows`` = (row_lp, top_val, top_idx) of ``token_logprobs`` -> the columns of ``out`` (a namespace
    of ``token`` [b, W] fp32, ``top`` [b, W, n] fp32, ``top_ids`` [b, W, n] int64, dense) that belong to the tokens they
    produced (``ls_logprob_commit``, one launch): for ``j < num[z]`` (int64 [b], any stride; None: every row of ``index_map``,
    or of ``rows``), row ``index_map[z, j]`` (int64 [b, J]; None: row j) goes to column ``base[z] + base_add + j`` (``base``
    int32 [b]).  Rows and columns out of range are skipped."""
    row_lp, top_val, top_idx = rows
    _dev(row_lp, top_val, top_idx, out.token, out.top, out.top_ids, base, num, index_map)
    b, R = row_lp.shape
    n = top_val.shape[2]
    W = out.token.shape[1]
    _lp_buffers(rows, b, R, n, "logprob_commit", ("row_lp", "top_val", "top_idx"))
    _lp_buffers((out.token, out.top, out.top_ids), b, W, n, "logprob_commit", ("out.token", "out.top", "out.top_ids"))
    if base.dtype != torch.int32 or base.numel() != b or not base.is_contiguous():
        raise TypeError("logprob_commit: base must be a contiguous int32 [b] tensor")
    J, map_p = R, None
    if index_map is not None:
        if index_map.dtype != torch.int64 or index_map.dim() != 2 or index_map.shape[0] != b or not index_map.is_contiguous():
            raise TypeError("logprob_commit: index_map must be a contiguous int64 [b, J] tensor")
        J, map_p = index_map.shape[1], index_map.data_ptr()
    num_p, num_s = _num(num, b, "logprob_commit")
    ptr = lambda t: t.data_ptr() if n else None
    _C.check(_C.load().ls_logprob_commit(row_lp.data_ptr(), ptr(top_val), ptr(top_idx), b, R, n, map_p, J, num_p, num_s,
                                         base.data_ptr(), base_add, out.token.data_ptr(), ptr(out.top), ptr(out.top_ids), W,
                                         _stream()), "ls_logprob_commit")


STOP_TABLE_WORDS = 341     # int32 words of a stop table (longspec_amd/stop.py, LS_STOP_TABLE_WORDS)


def _stop_table(table, what):
    if table.dtype != torch.int32 or table.dim() != 1 or table.numel() != STOP_TABLE_WORDS or not table.is_contiguous():
        raise TypeError(f"{what}: table must be a contiguous int32 [{STOP_TABLE_WORDS}] tensor (Stop.table)")
    return table.data_ptr()


def stop_scan(output_ids: torch.Tensor, table: torch.Tensor, stop_state: torch.Tensor, written: torch.Tensor,
              written_sub: Optional[torch.Tensor] = None, written_add: int = 0, num: Optional[torch.Tensor] = None,
              num_const: int = 1, fill: int = 0, state: Optional[torch.Tensor] = None, spec_mask: Optional[torch.Tensor] = None,
              logprobs=None) -> None:
    """The stop test of a round or step, behind its commit (``ls_stop_scan``, one launch, one wave per batch row; the definition
    is ``longspec_amd/stop.py``).  Of ``output_ids`` [b, W] int64, ``written[z] - written_sub[z] + written_add`` columns are
    written (int32 [b] tensors on the device), the last ``num[z]`` (int64 [b], any stride; None: ``num_const``) by this round.
    A row of ``stop_state`` [b, 4] int32 that has not stopped and matches a stop of ``table`` (``Stop.table``) among those
    columns becomes (length, which, match_start, reserved); for such a row and for one that had stopped before, the columns
    [length, written) of ``output_ids`` go back to ``fill``, of ``spec_mask`` [b, W] int64 to 0 and of ``logprobs`` (the
    namespace of ``logprobs.py``, W columns) to NaN / -inf / -1, and ``state[z, 1] |= 2`` (``state`` int64 [b, >= 2]: the round's
    state tensor).  Everything in place."""
    lp = (logprobs.token, logprobs.top, logprobs.top_ids) if logprobs is not None else ()
    _dev(output_ids, table, stop_state, written, written_sub, num, state, spec_mask, *lp)
    if output_ids.dtype != torch.int64 or output_ids.dim() != 2 or output_ids.stride(1) != 1:
        raise TypeError("stop_scan: output_ids must be int64 [b, W] with contiguous rows")
    b, W = output_ids.shape
    tab_p = _stop_table(table, "stop_scan")
    if stop_state.dtype != torch.int32 or tuple(stop_state.shape) != (b, 4) or not stop_state.is_contiguous():
        raise TypeError(f"stop_scan: stop_state must be a contiguous int32 [{b}, 4] tensor")
    num_p, num_s = _num(num, b, "stop_scan")
    if num is None and num_const < 0:
        raise ValueError(f"stop_scan: num_const={num_const}")
    state_p, state_s = None, 0
    if state is not None:
        if state.dtype != torch.int64 or state.dim() != 2 or state.shape[0] != b or state.shape[1] < 2 or state.stride(1) != 1:
            raise TypeError("stop_scan: state must be int64 [b, >= 2] with contiguous rows")
        state_p, state_s = state.data_ptr(), state.stride(0)
    mask_p, mask_s = None, 0
    if spec_mask is not None:
        if spec_mask.dtype != torch.int64 or tuple(spec_mask.shape) != (b, W) or spec_mask.stride(1) != 1:
            raise TypeError(f"stop_scan: spec_mask must be int64 [{b}, {W}] with contiguous rows")
        mask_p, mask_s = spec_mask.data_ptr(), spec_mask.stride(0)
    n, lp_p = 0, (None, None, None)
    if logprobs is not None:
        n = logprobs.top.shape[2]
        _lp_buffers(lp, b, W, n, "stop_scan", ("logprobs.token", "logprobs.top", "logprobs.top_ids"))
        lp_p = (logprobs.token.data_ptr(), logprobs.top.data_ptr() if n else None, logprobs.top_ids.data_ptr() if n else None)
    _C.check(_C.load().ls_stop_scan(output_ids.data_ptr(), b, output_ids.stride(0), W, _len_i32(written, b, "written"),
                                    _len_i32(written_sub, b, "written_sub"), int(written_add), num_p, num_s, int(num_const),
                                    tab_p, STOP_TABLE_WORDS, stop_state.data_ptr(), int(fill), state_p, state_s, mask_p, mask_s,
                                    lp_p[0], lp_p[1], lp_p[2], n, _stream()), "ls_stop_scan")


def stop_ban_rows(logits: torch.Tensor, table: torch.Tensor, base: Optional[torch.Tensor] = None,
                  base_sub: Optional[torch.Tensor] = None, base_add: int = 0, depth: Optional[str] = None,
                  tree_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The ``min_tokens`` ban on TARGET logits [b, V] or [b, R, V] (16-bit, unit column stride, any row strides), IN PLACE
    (``ls_stop_ban_rows``, one launch): row r of batch z predicts column ``base[z] - base_sub[z] + base_add + depth(r)`` (int32
    [b] tensors on the device, None: 0), ``depth`` None: 0, ``"row"``: r, ``"tree"``: the row sum of ``tree_mask[z, r, 1:]``
    (int64 [b, R, C]).  Where that column is below the table's ``min_tokens``, the entries of its token ids become -inf; every
    other element keeps its bits.  Returns ``logits``."""
    _dev(logits, table, base, base_sub, tree_mask)
    x, b, R, V = _rule_rows(logits, "stop_ban_rows")
    tab_p = _stop_table(table, "stop_ban_rows")
    if depth not in (None, "row", "tree"):
        raise ValueError(f"stop_ban_rows: depth={depth!r} (None, 'row' or 'tree')")
    mode = {None: 0, "row": 1, "tree": 2}[depth]
    mask_p = mask_sb = mask_sr = mask_c = 0
    if mode == 2:
        if tree_mask is None or tree_mask.dtype != torch.int64 or tree_mask.dim() != 3 or tuple(tree_mask.shape[:2]) != (b, R) \
                or tree_mask.stride(2) != 1:
            raise TypeError(f"stop_ban_rows: tree_mask must be int64 [{b}, {R}, C] with unit column stride")
        mask_p, mask_sb, mask_sr, mask_c = tree_mask.data_ptr(), tree_mask.stride(0), tree_mask.stride(1), tree_mask.shape[2]
    _C.check(_C.load().ls_stop_ban_rows(x.data_ptr(), b, R, V, _dtype(x), x.stride(0), max(x.stride(1), V), tab_p, STOP_TABLE_WORDS,
                                        _len_i32(base, b, "base"), _len_i32(base_sub, b, "base_sub"), int(base_add), mode,
                                        mask_p or None, mask_sb, mask_sr, mask_c, _stream()), "ls_stop_ban_rows")
    return logits


BAN_TABLE_WORDS = 1093     # int32 words of a ban table (longspec_amd/ban.py, LS_BAN_TABLE_WORDS)
BAN_CHUNK = 1024           # text columns per workgroup of the no-repeat scan (LS_BAN_CHUNK)
BAN_MAX_EXTRA = 128        # columns of extra_ids (LS_BAN_MAX_EXTRA): a verification pass has at most 80 rows


def ban_rows(logits: torch.Tensor, table: torch.Tensor, output_ids: Optional[torch.Tensor], base: Optional[torch.Tensor] = None,
             base_sub: Optional[torch.Tensor] = None, base_add: int = 0, extra_ids: Optional[torch.Tensor] = None,
             extra_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Banned sequences and no-repeat n-grams on TARGET logits [b, V] or [b, R, V] (16-bit, unit column stride, any
    non-overlapping row strides), IN PLACE (``ls_ban_rows``, one launch; the definition is ``longspec_amd/ban.py``).  The text of
    row r of batch z is ``output_ids[z, :w]`` (int64 [b, W]; None: no columns), ``w = base[z] - base_sub[z] + base_add`` (int32
    [b] tensors on the device, None: 0; clamped to 0..W), followed by every ``extra_ids[z, c]`` (int64 [b, C]) with
    ``extra_mask[z, r, c] != 0`` (int64 [b, R, C], or [R, C] = one mask for the whole batch) in increasing ``c``.  The last
    token of every sequence of ``table`` (``Ban.table``) whose front ends that text, and every token that would complete an
    n-gram the text already holds, become -inf; every other element keeps its bits.  The grid is sized from W and C: nothing is
    read back.  Returns ``logits``."""
    _dev(logits, table, output_ids, base, base_sub, extra_ids, extra_mask)
    x, b, R, V = _rule_rows(logits, "ban_rows")
    if table.dtype != torch.int32 or table.dim() != 1 or table.numel() != BAN_TABLE_WORDS or not table.is_contiguous():
        raise TypeError(f"ban_rows: table must be a contiguous int32 [{BAN_TABLE_WORDS}] tensor (Ban.table)")
    out_p, out_sb, W = None, 0, 0
    if output_ids is not None:
        if output_ids.dtype != torch.int64 or output_ids.dim() != 2 or output_ids.shape[0] != b or output_ids.stride(1) != 1:
            raise TypeError(f"ban_rows: output_ids must be int64 [{b}, W] with contiguous rows")
        W = output_ids.shape[1]
        if b > 1 and output_ids.stride(0) < W:
            raise ValueError("ban_rows: output_ids rows must be at least W elements apart")
        out_p, out_sb = (output_ids.data_ptr(), max(output_ids.stride(0), W)) if W else (None, 0)
    ids_p, ids_sb, mask_p, mask_sb, mask_sr, C = _extras(extra_ids, extra_mask, b, R, "ban_rows", BAN_MAX_EXTRA)
    _C.check(_C.load().ls_ban_rows(x.data_ptr(), b, R, V, _dtype(x), x.stride(0), max(x.stride(1), V), table.data_ptr(),
                                   BAN_TABLE_WORDS, out_p, out_sb, W, _len_i32(base, b, "base"), _len_i32(base_sub, b, "base_sub"),
                                   int(base_add), ids_p, ids_sb, mask_p, mask_sb, mask_sr, C, _stream()), "ls_ban_rows")
    return logits


DRY_TABLE_WORDS = 101      # int32 words of a dry table (longspec_amd/dry.py, LS_DRY_TABLE_WORDS)
DRY_MAX_MATCH = 32         # the depth matches are measured to (LS_DRY_MAX_MATCH)


def dry_rows(logits: torch.Tensor, table: torch.Tensor, output_ids: Optional[torch.Tensor], scratch: torch.Tensor,
             base: Optional[torch.Tensor] = None, base_sub: Optional[torch.Tensor] = None, base_add: int = 0,
             extra_ids: Optional[torch.Tensor] = None, extra_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The DRY repetition penalty on TARGET logits [b, V] or [b, R, V] (16-bit, unit column stride, any non-overlapping row
    strides), IN PLACE (``ls_dry_rows``, two launches of one kernel; the definition is ``longspec_amd/dry.py``).  The text of a
    row -- ``output_ids``, ``base`` / ``base_sub`` / ``base_add``, ``extra_ids`` / ``extra_mask`` -- is that of ``ban_rows``.
    Every id whose emission would extend a repeat of at least ``allowed_length`` tokens loses ``pen[length]`` of ``table``
    (``Dry.table``); every other element keeps its bits.  ``scratch``: a contiguous int32 tensor of at least b * R * V
    elements that the CALLER owns, all zero on entry and all zero again on exit; nothing is allocated and nothing is read
    back.  Returns ``logits``."""
    _dev(logits, table, output_ids, scratch, base, base_sub, extra_ids, extra_mask)
    x, b, R, V = _rule_rows(logits, "dry_rows")
    if table.dtype != torch.int32 or table.dim() != 1 or table.numel() != DRY_TABLE_WORDS or not table.is_contiguous():
        raise TypeError(f"dry_rows: table must be a contiguous int32 [{DRY_TABLE_WORDS}] tensor (Dry.table)")
    if scratch.dtype != torch.int32 or not scratch.is_contiguous() or scratch.numel() < b * R * V:
        raise TypeError(f"dry_rows: scratch must be a contiguous int32 tensor of at least b * R * V = {b * R * V} elements")
    out_p, out_sb, W = None, 0, 0
    if output_ids is not None:
        if output_ids.dtype != torch.int64 or output_ids.dim() != 2 or output_ids.shape[0] != b or output_ids.stride(1) != 1:
            raise TypeError(f"dry_rows: output_ids must be int64 [{b}, W] with contiguous rows")
        W = output_ids.shape[1]
        if b > 1 and output_ids.stride(0) < W:
            raise ValueError("dry_rows: output_ids rows must be at least W elements apart")
        out_p, out_sb = (output_ids.data_ptr(), max(output_ids.stride(0), W)) if W else (None, 0)
    ids_p, ids_sb, mask_p, mask_sb, mask_sr, C = _extras(extra_ids, extra_mask, b, R, "dry_rows", BAN_MAX_EXTRA)
    _C.check(_C.load().ls_dry_rows(x.data_ptr(), b, R, V, _dtype(x), x.stride(0), max(x.stride(1), V), table.data_ptr(),
                                   DRY_TABLE_WORDS, out_p, out_sb, W, scratch.data_ptr(), scratch.numel(),
                                   _len_i32(base, b, "base"), _len_i32(base_sub, b, "base_sub"), int(base_add), ids_p, ids_sb,
                                   mask_p, mask_sb, mask_sr, C, _stream()), "ls_dry_rows")
    return logits


WATERMARK_TABLE_WORDS = 8  # int32 words of a watermark table (longspec_amd/watermark.py, LS_WATERMARK_TABLE_WORDS)
WATERMARK_MAX_CONTEXT = 8  # the tokens that key a position's green list, at the most (LS_WATERMARK_MAX_CONTEXT)


def _watermark_table(table: torch.Tensor, who: str):
    if table.dtype != torch.int32 or table.dim() != 1 or table.numel() != WATERMARK_TABLE_WORDS or not table.is_contiguous():
        raise TypeError(f"{who}: table must be a contiguous int32 [{WATERMARK_TABLE_WORDS}] tensor (Watermark.table)")


def watermark_rows(logits: torch.Tensor, table: torch.Tensor, output_ids: Optional[torch.Tensor], base: Optional[torch.Tensor] = None,
                   base_sub: Optional[torch.Tensor] = None, base_add: int = 0, extra_ids: Optional[torch.Tensor] = None,
                   extra_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The keyed green-list bias on TARGET logits [b, V] or [b, R, V] (16-bit, unit column stride, any non-overlapping row
    strides), IN PLACE (``ls_watermark_rows``, one launch; the definition is ``longspec_amd/watermark.py``).  The text of a row
    -- ``output_ids``, ``base`` / ``base_sub`` / ``base_add``, ``extra_ids`` / ``extra_mask`` -- is that of ``ban_rows``.  Every
    id that is green after the row's last ``h`` tokens gains ``delta`` of ``table`` (``Watermark.table``); a row of fewer than
    ``h`` tokens and every other element keep their bits.  Not idempotent: a second call adds ``delta`` again.  Nothing is
    allocated and nothing is read back.  Returns ``logits``."""
    _dev(logits, table, output_ids, base, base_sub, extra_ids, extra_mask)
    x, b, R, V = _rule_rows(logits, "watermark_rows")
    _watermark_table(table, "watermark_rows")
    out_p, out_sb, W = None, 0, 0
    if output_ids is not None:
        if output_ids.dtype != torch.int64 or output_ids.dim() != 2 or output_ids.shape[0] != b or output_ids.stride(1) != 1:
            raise TypeError(f"watermark_rows: output_ids must be int64 [{b}, W] with contiguous rows")
        W = output_ids.shape[1]
        if b > 1 and output_ids.stride(0) < W:
            raise ValueError("watermark_rows: output_ids rows must be at least W elements apart")
        out_p, out_sb = (output_ids.data_ptr(), max(output_ids.stride(0), W)) if W else (None, 0)
    ids_p, ids_sb, mask_p, mask_sb, mask_sr, C = _extras(extra_ids, extra_mask, b, R, "watermark_rows", BAN_MAX_EXTRA)
    _C.check(_C.load().ls_watermark_rows(x.data_ptr(), b, R, V, _dtype(x), x.stride(0), max(x.stride(1), V), table.data_ptr(),
                                         WATERMARK_TABLE_WORDS, out_p, out_sb, W, _len_i32(base, b, "base"),
                                         _len_i32(base_sub, b, "base_sub"), int(base_add), ids_p, ids_sb, mask_p, mask_sb, mask_sr, C,
                                         _stream()), "ls_watermark_rows")
    return logits


def watermark_score(ids: torch.Tensor, table: torch.Tensor, lengths: Optional[torch.Tensor] = None, want_flags: bool = True,
                    want_hashes: bool = False):
    """The watermark detector's counts for token ids int64 [n] or [b, n] (unit column stride, rows at least n apart)
    (``ls_watermark_score``, one launch; the definition is ``longspec_amd/watermark.py``).  ``lengths``: int32 [b] on the
    device or None, row z is ``ids[z, :lengths[z]]`` (clamped to 0..n).  Returns a namespace of ``counts`` int32 [b, 2] --
    scored and green positions --, ``flags`` int8 [b, n] (-1 not scored, 0 red, 1 green; None without ``want_flags``) and
    ``hashes`` uint64 [b, n] (``u`` of a scored position, 0 elsewhere; None without ``want_hashes``).  Nothing is read back."""
    _dev(ids, table, lengths)
    if ids.dtype != torch.int64 or ids.dim() not in (1, 2):
        raise TypeError("watermark_score: ids must be int64 [n] or [b, n]")
    x = ids if ids.dim() == 2 else ids.unsqueeze(0)
    b, n = x.shape
    if n > 0 and (x.stride(1) != 1 or (b > 1 and x.stride(0) < n)):
        raise ValueError("watermark_score: ids must have unit column stride and rows at least n elements apart")
    _watermark_table(table, "watermark_score")
    counts = torch.empty((b, 2), dtype=torch.int32, device=x.device)
    flags = torch.empty((b, n), dtype=torch.int8, device=x.device) if want_flags else None
    hashes = torch.empty((b, n), dtype=torch.uint64, device=x.device) if want_hashes else None
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    _C.check(_C.load().ls_watermark_score(ptr(x), b, n, max(x.stride(0), n) if n else 0, _len_i32(lengths, b, "lengths"),
                                          table.data_ptr(), WATERMARK_TABLE_WORDS, counts.data_ptr(), ptr(flags), ptr(hashes),
                                          _stream()), "ls_watermark_score")
    return SimpleNamespace(counts=counts, flags=flags, hashes=hashes)


GUIDE_HEADER_WORDS = 8     # int32 words in front of a guide table's class area (longspec_amd/guide.py, LS_GUIDE_HEADER_WORDS)
GUIDE_MAX_EXTRA = 128      # columns of extra_ids, and ids per guide_advance (LS_GUIDE_MAX_EXTRA)
GUIDE_SLICE = 8192         # ids per workgroup of guide_rows (LS_GUIDE_SLICE)


def _guide_table(table, who):
    if table.dtype != torch.int32 or table.dim() != 1 or table.numel() < GUIDE_HEADER_WORDS or not table.is_contiguous() \
            or table.data_ptr() % 16 != 0:
        raise TypeError(f"{who}: table must be a contiguous, 16-byte aligned int32 tensor of at least {GUIDE_HEADER_WORDS} words "
                        "(Guide.table)")
    return table.data_ptr(), table.numel()


def guide_rows(logits: torch.Tensor, table: torch.Tensor, state: torch.Tensor, extra_ids: Optional[torch.Tensor] = None,
               extra_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Guided decoding on TARGET logits [b, V] or [b, R, V] (16-bit, unit column stride, any non-overlapping row strides), IN
    PLACE (``ls_guide_rows``, one launch; the definition is ``longspec_amd/guide.py``).  Row r of batch z is in the state
    ``state[z]`` (int32 [b], the state behind the committed text) walked along every ``extra_ids[z, c]`` (int64 [b, C]) with
    ``extra_mask[z, r, c] != 0`` (int64 [b, R, C], or [R, C] = one mask for the whole batch) in increasing ``c``.  A dead row
    (state -1) keeps its bits; in a live one every token without a transition in ``table`` (``Guide.table``) becomes -inf and
    every other element keeps its bits.  The grid is sized from V: nothing is read back.  Returns ``logits``."""
    _dev(logits, table, state, extra_ids, extra_mask)
    x, b, R, V = _rule_rows(logits, "guide_rows")
    tab_p, tab_n = _guide_table(table, "guide_rows")
    if state.dtype != torch.int32 or tuple(state.shape) != (b,) or not state.is_contiguous():
        raise TypeError(f"guide_rows: state must be a contiguous int32 [{b}] tensor")
    ids_p, ids_sb, mask_p, mask_sb, mask_sr, C = _extras(extra_ids, extra_mask, b, R, "guide_rows", GUIDE_MAX_EXTRA)
    _C.check(_C.load().ls_guide_rows(x.data_ptr(), b, R, V, _dtype(x), x.stride(0), max(x.stride(1), V), tab_p, tab_n,
                                     state.data_ptr(), ids_p, ids_sb, mask_p, mask_sb, mask_sr, C, _stream()), "ls_guide_rows")
    return logits


def guide_advance(state: torch.Tensor, table: torch.Tensor, ids: torch.Tensor, num: Optional[torch.Tensor] = None) -> None:
    """Advance the guide state [b] int32 in place (``ls_guide_advance``): ``state[z]`` walks every ``ids[z, j]`` (int64 [b, n],
    n <= 128) with ``j < num[z]`` (``num`` [b] int64, None: all) through ``table`` (``Guide.table``).  An id outside the
    vocabulary or without a transition leaves -1, and -1 stays -1."""
    _dev(state, table, ids, num)
    if state.dtype != torch.int32 or state.dim() != 1 or not state.is_contiguous():
        raise TypeError("guide_advance: state must be a contiguous int32 [b] tensor")
    b = state.shape[0]
    tab_p, tab_n = _guide_table(table, "guide_advance")
    ids = _id_rows(ids, b, "guide_advance", most=GUIDE_MAX_EXTRA)
    num_p, num_s = _num(num, b, "guide_advance")
    _C.check(_C.load().ls_guide_advance(state.data_ptr(), b, tab_p, tab_n, ids.data_ptr(), ids.shape[1], ids.stride(0), num_p, num_s,
                                        _stream()), "ls_guide_advance")


GUIDE_LIFT_MAX_STATES = 16384   # S of a byte DFA the device lifts (LS_GUIDE_LIFT_MAX_STATES): its states are 16-bit table entries
GUIDE_MAX_CLASSES = 16384       # C of a guide (longspec_amd/guide.py, LS_GUIDE_MAX_CLASSES)


def _lift_operands(step, blob, offsets, who):
    """(step pointer, blob pointer, offsets pointer, blob bytes, T, S) of the lift's operands (``ls_guide_lift_*``)."""
    _dev(step, blob, offsets)
    if step.dtype != torch.int16 or step.dim() != 2 or step.shape[0] != 256 or not step.is_contiguous() \
            or not (1 <= step.shape[1] - 1 <= GUIDE_LIFT_MAX_STATES):
        raise TypeError(f"{who}: step must be a contiguous int16 [256, S + 1] tensor (byte-major, S = the dead state) with S in "
                        f"1..{GUIDE_LIFT_MAX_STATES}")
    if blob.dtype != torch.uint8 or blob.dim() != 1 or not blob.is_contiguous():
        raise TypeError(f"{who}: blob must be a contiguous uint8 [bytes] tensor")
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.numel() < 2 or not offsets.is_contiguous():
        raise TypeError(f"{who}: offsets must be a contiguous int32 [T + 1] tensor, T >= 1")
    # (an empty blob has no storage to point at: any valid address will do, nothing is read through it)
    return step.data_ptr(), blob.data_ptr() if blob.numel() else step.data_ptr(), offsets.data_ptr(), blob.numel(), \
        offsets.numel() - 1, step.shape[1] - 1


def guide_lift_hash(step: torch.Tensor, blob: torch.Tensor, offsets: torch.Tensor):
    """Two 64-bit hashes of every token's behaviour vector under a byte DFA and its alive flag (``ls_guide_lift_hash``, one
    launch): ``(hashes int64 [T, 2], alive uint8 [T])``.  ``step`` int16 [256, S + 1] byte-major with S the dead state, ``blob``
    uint8 the bytes of all tokens, ``offsets`` int32 [T + 1].  Equal vectors have equal hashes; an empty token is not alive."""
    sp, bp, op, nb, T, S = _lift_operands(step, blob, offsets, "guide_lift_hash")
    hashes = torch.empty((T, 2), dtype=torch.int64, device=step.device)
    alive = torch.empty((T,), dtype=torch.uint8, device=step.device)
    _C.check(_C.load().ls_guide_lift_hash(sp, bp, op, nb, T, S, hashes.data_ptr(), alive.data_ptr(), _stream()), "ls_guide_lift_hash")
    return hashes, alive


def guide_lift_cols(step: torch.Tensor, blob: torch.Tensor, offsets: torch.Tensor, ids: torch.Tensor,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The exact behaviour vectors of the tokens ``ids`` (contiguous int32 [n], n >= 1), int32 [n, S] with -1 = dead
    (``ls_guide_lift_cols``, one launch), into ``out`` (contiguous int32 [n, S]) where given."""
    sp, bp, op, nb, T, S = _lift_operands(step, blob, offsets, "guide_lift_cols")
    _dev(ids, out)
    if ids.dtype != torch.int32 or ids.dim() != 1 or ids.numel() < 1 or not ids.is_contiguous():
        raise TypeError("guide_lift_cols: ids must be a contiguous int32 [n] tensor, n >= 1")
    n = ids.numel()
    if out is None:
        out = torch.empty((n, S), dtype=torch.int32, device=step.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (n, S) or not out.is_contiguous():
        raise TypeError(f"guide_lift_cols: out must be a contiguous int32 [{n}, {S}] tensor")
    _C.check(_C.load().ls_guide_lift_cols(sp, bp, op, nb, T, S, ids.data_ptr(), n, out.data_ptr(), _stream()), "ls_guide_lift_cols")
    return out


def guide_lift_check(step: torch.Tensor, blob: torch.Tensor, offsets: torch.Tensor, reps: torch.Tensor,
                     group: torch.Tensor) -> torch.Tensor:
    """uint8 [T]: 1 where token t has ``group[t] >= 0`` (contiguous int32 [T]) and its behaviour vector is not
    ``reps[group[t]]`` (contiguous int32 [C, S], -1 = dead), else 0 (``ls_guide_lift_check``, one launch)."""
    sp, bp, op, nb, T, S = _lift_operands(step, blob, offsets, "guide_lift_check")
    _dev(reps, group)
    if reps.dtype != torch.int32 or reps.dim() != 2 or reps.shape[0] < 1 or reps.shape[1] != S or not reps.is_contiguous():
        raise TypeError(f"guide_lift_check: reps must be a contiguous int32 [C, {S}] tensor, C >= 1")
    if group.dtype != torch.int32 or tuple(group.shape) != (T,) or not group.is_contiguous():
        raise TypeError(f"guide_lift_check: group must be a contiguous int32 [{T}] tensor")
    mismatch = torch.empty((T,), dtype=torch.uint8, device=step.device)
    _C.check(_C.load().ls_guide_lift_check(sp, bp, op, nb, T, S, reps.data_ptr(), reps.shape[0], group.data_ptr(),
                                           mismatch.data_ptr(), _stream()), "ls_guide_lift_check")
    return mismatch


def guide_lift(step: torch.Tensor, blob: torch.Tensor, offsets: torch.Tensor, *, _hash_bits: int = 128, _stats=None):
    """The classes of a vocabulary under a byte DFA: ``(token_class int64 [T], vectors int64 [C, S])`` as numpy arrays on the
    host -- tokens with the same behaviour vector share a class, ``vectors[c]`` is the class's vector (-1 = dead), a token that
    is empty or dead from every state has class -1, and the classes are numbered as ``np.unique(axis=0)`` numbers the rows of
    the full [T, S] matrix (lexicographically), which is never built: the device hashes every vector (``guide_lift_hash``), the
    alive tokens are grouped by hash, one representative per group is walked exactly (``guide_lift_cols``), every token is
    checked against its group's representative (``guide_lift_check``), and a token that differs -- a hash collision -- is walked
    exactly and regrouped on the host.  ValueError where the groups outnumber ``GUIDE_MAX_CLASSES``.  ``_hash_bits`` below 128
    keeps only that many low bits of the first hash (0: one group): the tests' way into the collision path.  ``_stats``: a dict
    that receives ``groups`` and ``mismatches``."""
    import numpy as np
    _, _, _, _, T, S = _lift_operands(step, blob, offsets, "guide_lift")
    if isinstance(_hash_bits, bool) or not isinstance(_hash_bits, int) or not (0 <= _hash_bits <= 128):
        raise ValueError(f"guide_lift: _hash_bits must be 0..128, got {_hash_bits!r}")
    too_many = lambda n: ValueError(f"Guide: the vocabulary has {n} or more distinct behaviours under this DFA, more than "
                                    f"{GUIDE_MAX_CLASSES} classes")
    hashes, alive = guide_lift_hash(step, blob, offsets)
    alive_ids = alive.nonzero().view(-1)
    token_class = np.full(T, -1, dtype=np.int64)
    if _stats is not None:
        _stats.update(groups=0, mismatches=0)
    if alive_ids.numel() == 0:
        return token_class, np.zeros((0, S), dtype=np.int64)
    keys = hashes[alive_ids]
    if _hash_bits < 128:
        bits = min(_hash_bits, 64)
        low = keys[:, 0] & ((1 << bits) - 1 if bits < 63 else -1 if bits == 64 else 2 ** 63 - 1)
        keys = torch.stack([low, torch.zeros_like(low)], dim=1)
    _, inverse = torch.unique(keys, dim=0, return_inverse=True)
    G = int(inverse.max()) + 1
    if G > GUIDE_MAX_CLASSES:
        raise too_many(G)
    place = torch.arange(alive_ids.numel(), device=step.device)
    first = torch.full((G,), alive_ids.numel(), dtype=torch.int64, device=step.device).scatter_reduce_(0, inverse, place, "amin")
    reps = guide_lift_cols(step, blob, offsets, alive_ids[first].to(torch.int32))
    group = torch.full((T,), -1, dtype=torch.int32, device=step.device)
    group[alive_ids] = inverse.to(torch.int32)
    odd = guide_lift_check(step, blob, offsets, reps, group).nonzero().view(-1)
    vectors = reps.cpu().numpy()
    group = group.cpu().numpy().astype(np.int64)
    if _stats is not None:
        _stats.update(groups=G, mismatches=int(odd.numel()))
    if odd.numel():                                                # collisions: exact vectors, at most GUIDE_MAX_CLASSES at a time
        known = {v.tobytes(): c for c, v in enumerate(vectors)}
        extra = []
        for chunk in odd.split(GUIDE_MAX_CLASSES):
            vs = guide_lift_cols(step, blob, offsets, chunk.to(torch.int32)).cpu().numpy()
            for t, v in zip(chunk.cpu().tolist(), vs):
                c = known.get(v.tobytes())
                if c is None:
                    c = known[v.tobytes()] = len(known)
                    extra.append(v)
                    if len(known) > GUIDE_MAX_CLASSES:
                        raise too_many(len(known))
                group[t] = c
        vectors = np.concatenate([vectors, np.stack(extra)]) if extra else vectors
    vectors, rank = np.unique(vectors, axis=0, return_inverse=True)     # the numbering of np.unique on the full matrix
    rank = np.asarray(rank).reshape(-1)
    live = group >= 0
    token_class[live] = rank[group[live]]
    return token_class, vectors.astype(np.int64)


_ngram_ws = _Workspace()     # its own buffer, as _sample_ws: a captured round holds its address
NGRAM_CHUNK = 1024         # candidate ends per stage-1 workgroup of ngram_draft (LS_NGRAM_CHUNK)
NGRAM_MAX_GAMMA, NGRAM_MAX_N = 15, 8


def ngram_draft(prompt_ids: torch.Tensor, input_len: torch.Tensor, output_ids: torch.Tensor, cache_lens: torch.Tensor,
                len_bound: int, gamma: int, max_ngram: int, min_ngram: int, spec_buffer: torch.Tensor,
                info: Optional[torch.Tensor] = None, hist: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The drafter of prompt-lookup speculation (``ls_ngram_draft``, two launches; the definition is
    ``longspec_amd/lookup.py``).  The text of row z is ``prompt_ids[z, :input_len[z]] ++ output_ids[z, :cache_lens[z] -
    input_len[z] + 1]`` (int64 [b, P] / [b, W] with contiguous rows, any row stride; int32 [b] lengths on the device); the
    continuation of the most recent earlier occurrence of its longest suffix of ``min_ngram .. max_ngram`` tokens goes to
    ``spec_buffer[:, 1:]`` (contiguous int64 [b, gamma + 1]; column 0 is kept), ``hist[z, n] += 1`` (contiguous int64
    [b, max_ngram + 1], optional).  ``len_bound``: a HOST-side upper bound of the text lengths, which sizes the grid -- nothing
    is read from the device.  Returns ``info`` int32 [b, 2] = (n, e): the matched length and the end of the occurrence, or
    (0, -1)."""
    _dev(prompt_ids, input_len, output_ids, cache_lens, spec_buffer, info, hist)
    if not (1 <= gamma <= NGRAM_MAX_GAMMA and 1 <= max_ngram <= NGRAM_MAX_N and 1 <= min_ngram <= max_ngram):
        raise ValueError(f"ngram_draft: gamma={gamma} (1..{NGRAM_MAX_GAMMA}), max_ngram={max_ngram} (1..{NGRAM_MAX_N}), "
                         f"min_ngram={min_ngram} (1..max_ngram)")
    b, info = _ngram_buffers(prompt_ids, output_ids, len_bound, info, (2,), ((hist, "hist", max_ngram + 1),), "ngram_draft")
    if spec_buffer.dtype != torch.int64 or tuple(spec_buffer.shape) != (b, gamma + 1) or not spec_buffer.is_contiguous():
        raise TypeError(f"ngram_draft: spec_buffer must be a contiguous int64 [{b}, {gamma + 1}] tensor")
    lib = _C.load()
    need = lib.ls_ngram_workspace_bytes(b, int(len_bound))
    ws = _ngram_ws.get(output_ids.device, max(need, 1))
    _C.check(lib.ls_ngram_draft(prompt_ids.data_ptr(), max(prompt_ids.stride(0), prompt_ids.shape[1]), prompt_ids.shape[1],
                                _len_i32(input_len, b, "input_len"), output_ids.data_ptr(),
                                max(output_ids.stride(0), output_ids.shape[1]), output_ids.shape[1],
                                _len_i32(cache_lens, b, "cache_lens"), b, int(len_bound), gamma, max_ngram, min_ngram,
                                spec_buffer.data_ptr(), info.data_ptr(), hist.data_ptr() if hist is not None else None,
                                ws.data_ptr(), ws.numel(), _stream()), "ls_ngram_draft")
    return info


_ngram_tree_ws = _Workspace()     # (its records are LS_NGRAM_TOP times ngram_draft's: a buffer of its own)
NGRAM_TOP = 8              # candidates the tree drafter walks (LS_NGRAM_TOP)


def ngram_tree_draft(prompt_ids: torch.Tensor, input_len: torch.Tensor, output_ids: torch.Tensor, written: torch.Tensor,
                     len_bound: int, gamma: int, branches: int, max_ngram: int, min_ngram: int, all_spec: torch.Tensor,
                     tree_mask: torch.Tensor, info: Optional[torch.Tensor] = None, hist: Optional[torch.Tensor] = None,
                     hist_nb: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The tree drafter of prompt-lookup speculation (``ls_ngram_tree_draft``, two launches; the definition is
    ``longspec_amd/lookup.py``).  The text of row z is ``prompt_ids[z, :input_len[z]] ++ output_ids[z, :written[z]]``
    (``written`` int32 [b] on the device: the tree round's ``emitted_dev``).  Up to ``branches`` distinct continuations of the
    ``NGRAM_TOP`` best candidates go to ``all_spec[:, 1:]`` (contiguous int64 [b, F], F = 1 + branches * gamma, node
    1 + (d-1) * branches + j = depth d of branch j; column 0 is kept) and the rows 1.. of ``tree_mask`` (contiguous int64
    [b, F, F]; row 0 is kept) are written in full.  ``hist[z, n of slot 0] += 1`` (int64 [b, max_ngram + 1], optional),
    ``hist_nb[z, nb] += 1`` (int64 [b, branches + 1], optional).  ``len_bound``: a HOST-side upper bound of the text lengths.
    Returns ``info`` int32 [b, branches, 2] = (n, e) per slot, (0, -1) for the slots that copy slot 0."""
    _dev(prompt_ids, input_len, output_ids, written, all_spec, tree_mask, info, hist, hist_nb)
    if not (1 <= gamma <= NGRAM_MAX_GAMMA and 1 <= branches <= NGRAM_TOP and 1 <= max_ngram <= NGRAM_MAX_N
            and 1 <= min_ngram <= max_ngram):
        raise ValueError(f"ngram_tree_draft: gamma={gamma} (1..{NGRAM_MAX_GAMMA}), branches={branches} (1..{NGRAM_TOP}), "
                         f"max_ngram={max_ngram} (1..{NGRAM_MAX_N}), min_ngram={min_ngram} (1..max_ngram)")
    b, info = _ngram_buffers(prompt_ids, output_ids, len_bound, info, (branches, 2),
                             ((hist, "hist", max_ngram + 1), (hist_nb, "hist_nb", branches + 1)), "ngram_tree_draft")
    Fn = 1 + branches * gamma
    if all_spec.dtype != torch.int64 or tuple(all_spec.shape) != (b, Fn) or not all_spec.is_contiguous():
        raise TypeError(f"ngram_tree_draft: all_spec must be a contiguous int64 [{b}, {Fn}] tensor")
    if tree_mask.dtype != torch.int64 or tuple(tree_mask.shape) != (b, Fn, Fn) or not tree_mask.is_contiguous():
        raise TypeError(f"ngram_tree_draft: tree_mask must be a contiguous int64 [{b}, {Fn}, {Fn}] tensor")
    lib = _C.load()
    need = lib.ls_ngram_tree_workspace_bytes(b, int(len_bound))
    ws = _ngram_tree_ws.get(output_ids.device, max(need, 1))
    _C.check(lib.ls_ngram_tree_draft(prompt_ids.data_ptr(), max(prompt_ids.stride(0), prompt_ids.shape[1]), prompt_ids.shape[1],
                                     _len_i32(input_len, b, "input_len"), output_ids.data_ptr(),
                                     max(output_ids.stride(0), output_ids.shape[1]), output_ids.shape[1],
                                     _len_i32(written, b, "written"), b, int(len_bound), gamma, branches, max_ngram, min_ngram,
                                     all_spec.data_ptr(), tree_mask.data_ptr(), info.data_ptr(),
                                     hist.data_ptr() if hist is not None else None,
                                     hist_nb.data_ptr() if hist_nb is not None else None, ws.data_ptr(), ws.numel(), _stream()),
             "ls_ngram_tree_draft")
    return info


TOPK_CHUNK = 8192          # logits per stage-1 record (ls_topk_chunk(); checked at first use)


def topk_stage1(logits_local: Optional[torch.Tensor], rows: int, k: int, col_base: int, nslots: int, out: torch.Tensor, dtype=None):
    """Stage 1 of the vocabulary-parallel ``logprob_topk`` / ``argmax_rows``: this rank's slice of the lm_head output
    ``logits_local`` [rows, V_local] (global columns ``col_base`` ...; None when the rank owns no column) -> ``nslots`` chunk
    records [nslots, rows, 2 + 2k] fp32 written into ``out`` (flat, e.g. the exchange's send buffer).  Returns the record view."""
    lib = _C.load()
    assert lib.ls_topk_chunk() == TOPK_CHUNK
    rec = 2 + 2 * k
    n = nslots * rows * rec
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n
    if logits_local is None:
        v_local, ld, ptr = 0, 8, out.data_ptr()            # (never read: every slot is an empty record)
        dt = _C.LS_F16 if dtype in (None, torch.float16) else _C.LS_BF16
    else:
        _dev(logits_local)
        assert logits_local.dim() == 2 and logits_local.shape[0] == rows and logits_local.stride(1) == 1
        v_local, ld, ptr, dt = logits_local.shape[1], logits_local.stride(0), logits_local.data_ptr(), _dtype(logits_local)
    _C.check(lib.ls_topk_stage1(ptr, rows, v_local, ld, dt, k, col_base, nslots, out.data_ptr(), _stream()), "ls_topk_stage1")
    return out[:n].view(nslots, rows, rec)


def topk_stage2(records: torch.Tensor, rows: int, vocab: int, k: int, history: Optional[torch.Tensor], argmax: bool):
    """Stage 2: all ranks' records [slots, rows, 2 + 2k] in rank order (= global chunk order) -> what ``logprob_topk``
    (values [1, k], flat indices [1, k]) or ``argmax_rows`` (indices [rows]) return on the gathered logits, bit for bit."""
    _dev(records, history)
    assert records.dtype == torch.float32 and records.is_contiguous() and records.shape[1] == rows and records.shape[2] == 2 + 2 * k
    lib = _C.load()
    dev = records.device
    if argmax:
        idx = torch.empty((rows,), dtype=torch.int64, device=dev)
        _C.check(lib.ls_topk_stage2(records.data_ptr(), rows, vocab, 1, records.shape[0], None, 1, None, idx.data_ptr(), _stream()),
                 "ls_topk_stage2")
        return idx
    vals = torch.empty((1, k), dtype=torch.float32, device=dev)
    idx = torch.empty((1, k), dtype=torch.int64, device=dev)
    if history is not None:
        history = history.to(torch.float32).contiguous()
    _C.check(lib.ls_topk_stage2(records.data_ptr(), rows, vocab, k, records.shape[0], history.data_ptr() if history is not None else None,
                                0, vals.data_ptr(), idx.data_ptr(), _stream()), "ls_topk_stage2")
    return vals, idx


_linear_timing = None


def set_linear_timing(hook):
    """Profiling: ``hook(algorithmic_bytes) -> (start_event, stop_event) | None`` is asked for a torch event pair
    before every skinny-GEMM launch (recorded by the C ABI around the kernel, on the launch stream)."""
    global _linear_timing
    _linear_timing = hook


class NormFold:
    """An RMSNorm that has not been applied yet: ``h`` is the un-normalised residual stream, ``ssq`` [rows, hidden / 64]
    the fp32 partial sums of squares of its rows (written by the projection that produced ``h``, ``linear(...,
    ssq_out=True)``), ``weight`` / ``eps`` the norm's parameters.  The projections take it as ``norm=`` together with
    ``x = h`` and normalise on the way in -- bit-identical to ``rmsnorm`` followed by the plain call."""
    __slots__ = ("weight", "eps", "ssq")

    def __init__(self, weight, eps, ssq):
        self.weight, self.eps, self.ssq = weight, float(eps), ssq


PREFETCH_PROBE = 0       # measurement switch (tools/bench_l2_prefetch.py), 0 in the product


_PACK_BITS = {PackedWeight: 16, PackedWeight8: 8, PackedWeight4: 4}


def _linear_call(x, weights, biases, epilogue, n_splits=0, timing=None, rope=None, residual=None, norm=None, ssq_out=False):
    _dev(x)
    K = x.shape[-1]
    x2 = x.reshape(-1, K)
    if x2.stride(-1) != 1 or x2.stride(0) % 8 != 0 or x2.data_ptr() % 16 != 0:
        x2 = x2.contiguous()
    M = x2.shape[0]
    d = _C.LinearDesc()
    d.x = x2.data_ptr()
    n_tot = 0
    cls = type(weights[0])
    w8, w4 = cls is PackedWeight8, cls is PackedWeight4
    if cls not in _PACK_BITS:
        raise TypeError("linear: weights must be PackedWeight (ops.pack_weight(nn.Linear.weight)), PackedWeight8 or PackedWeight4")
    if any(type(w) in _PACK_BITS and type(w) is not cls for w in weights):
        raise ValueError("linear: one weight format per launch -- the segments of one call are all 4-bit, all 8-bit or all 16-bit "
                         "packed weights")
    if w8 or w4:
        bits = _PACK_BITS[cls]
        if norm is not None or ssq_out:
            raise ValueError(f"linear: the folded RMSNorm (norm=, ssq_out=) is not available with {bits}-bit weights")
        if weights[0].pair != (epilogue == _C.LS_EPI_SILU_MUL):
            raise ValueError(f"linear: mlp_gate_up takes pack_gate_up{bits}(...), every other call pack_weight{bits}(...)")
        if w8:
            scales = (C.c_void_p * 3)()
    for i, w in enumerate(weights):
        if type(w) is not cls:
            raise TypeError("linear: weights must be PackedWeight (ops.pack_weight(nn.Linear.weight)), PackedWeight8 or PackedWeight4")
        if w.k != K or (cls is PackedWeight and w.dtype != x.dtype):
            raise ValueError(f"packed weight [{w.n}, {w.k}] {w.dtype} does not match x [..., {K}] {x.dtype}")
        if w8:
            if w.pair:
                scales[0], scales[1] = w.scale[0].data_ptr(), w.scale[1].data_ptr()
            else:
                scales[i] = w.scale.data_ptr()
        if w.rope != (epilogue == _C.LS_EPI_QKV_ROPE and i < 2):
            raise ValueError("linear: q/k weights of linear_qkv_rope are packed with rope=True, every other weight without")
        d.w[i] = w.data.data_ptr()
        b = biases[i] if biases is not None else None
        if b is not None and (b.dtype != x.dtype or not b.is_contiguous() or b.numel() != w.n):
            raise ValueError("bias must be a contiguous [N] tensor of x's dtype")
        d.bias[i] = b.data_ptr() if b is not None else None
        d.n[i] = w.n
        n_tot += w.n
    d.n_seg = len(weights)
    n_out = weights[0].n if epilogue == _C.LS_EPI_SILU_MUL else n_tot
    y = torch.empty((M, n_out), dtype=x.dtype, device=x.device)
    d.y = y.data_ptr()
    d.M, d.K = M, K
    d.dtype = _dtype(x)
    d.epilogue = epilogue
    d.n_splits = n_splits
    d.ldx, d.ldy = x2.stride(0), n_out
    if residual is not None:
        _dev(residual)
        r2 = residual.reshape(-1, residual.shape[-1])
        if r2.shape != (M, n_out) or r2.dtype != x.dtype or r2.stride(-1) != 1 or r2.stride(0) % 4 != 0:
            raise ValueError("linear: residual must be [..., N] of x's dtype with contiguous rows")
        d.residual, d.ldr = r2.data_ptr(), r2.stride(0)
    if rope is not None:
        cos, sin = rope
        _dev(cos, sin)
        for t in (cos, sin):
            if t.dtype != x.dtype or not t.is_contiguous() or t.numel() != M * 128:
                raise ValueError("linear_qkv_rope: cos/sin must be contiguous [rows, 128] tables of x's dtype")
        d.rope_cos, d.rope_sin = cos.data_ptr(), sin.data_ptr()
    ssq = None
    if norm is not None:
        _dev(norm.weight, norm.ssq)
        if (norm.weight.dtype != x.dtype or norm.weight.numel() != K or not norm.weight.is_contiguous()
                or norm.ssq.dtype != torch.float32 or norm.ssq.dim() != 2 or norm.ssq.shape[0] != M or not norm.ssq.is_contiguous()):
            raise ValueError("linear: norm = NormFold(weight [K] of x's dtype, eps, ssq fp32 [rows, parts] contiguous)")
        d.norm_weight, d.norm_eps = norm.weight.data_ptr(), norm.eps
        d.ssq_in, d.ssq_parts = norm.ssq.data_ptr(), norm.ssq.shape[1]
    if ssq_out:
        if epilogue != _C.LS_EPI_NONE or len(weights) != 1 or n_out % 64:
            raise ValueError("linear: ssq_out goes with a single plain projection whose N is a multiple of 64")
        ssq = torch.empty((M, n_out // 64), dtype=torch.float32, device=x.device)
        d.ssq_out = ssq.data_ptr()
    if timing is None and _linear_timing is not None:
        rows_w = sum(w.n for w in weights) * (2 if epilogue == _C.LS_EPI_SILU_MUL else 1)
        w_bytes = rows_w * K if w8 else rows_w * K * 17 // 32 if w4 else rows_w * K * x.element_size()
        timing = _linear_timing(w_bytes + (M * K + M * n_out) * x.element_size())
    if timing is not None:          # (torch.cuda.Event, torch.cuda.Event), both already created by a record()
        d.ev_start, d.ev_stop = timing[0].cuda_event, timing[1].cuda_event
    lib = _C.load()
    key = (M, K, d.n[0], d.n[1], d.n[2], epilogue, n_splits, d.dtype, norm is not None, _PACK_BITS[cls])
    need = _linear_need.get(key)
    if need is None:
        need = (lib.ls_linear_w8_workspace_bytes(C.byref(d)) if w8 else lib.ls_linear_w4_workspace_bytes(C.byref(d)) if w4
                else lib.ls_linear_workspace_bytes(C.byref(d)))
        if need == 0:                                                                          # raises with the reason
            if w4:
                _C.check(lib.ls_linear_w4_fwd(C.byref(d), None, 0, _stream()), "ls_linear_w4_fwd")
            if w8:
                _C.check(lib.ls_linear_w8_fwd(C.byref(d), scales, None, 0, _stream()), "ls_linear_w8_fwd")
            _C.check(lib.ls_linear_fwd(C.byref(d), None, 0, _stream()), "ls_linear_fwd")
        _linear_need[key] = need
    stream = _stream()
    ws = _gemm_ws.get(x.device, need, stream)
    if w8:
        global W8_CALLS
        _C.check(lib.ls_linear_w8_fwd(C.byref(d), scales, ws.data_ptr(), ws.numel(), stream), "ls_linear_w8_fwd")
        W8_CALLS += 1
        return y
    if w4:
        global W4_CALLS
        _C.check(lib.ls_linear_w4_fwd(C.byref(d), ws.data_ptr(), ws.numel(), stream), "ls_linear_w4_fwd")
        W4_CALLS += 1
        return y
    if PREFETCH_PROBE > 0:          # tools/bench_l2_prefetch.py: what an L2-resident head of the weight stream is worth
        ev = (d.ev_start, d.ev_stop)
        d.ev_start, d.ev_stop = None, None
        _C.check(lib.ls_linear_prefetch(C.byref(d), PREFETCH_PROBE, ws.data_ptr(), ws.numel(), stream), "ls_linear_prefetch")
        d.ev_start, d.ev_stop = ev
    _C.check(lib.ls_linear_fwd(C.byref(d), ws.data_ptr(), ws.numel(), stream), "ls_linear_fwd")
    return (y, ssq) if ssq_out else y


def linear(x: torch.Tensor, weight: PackedWeight, bias: Optional[torch.Tensor] = None, n_splits: int = 0, timing=None,
           residual: Optional[torch.Tensor] = None, norm: Optional[NormFold] = None, ssq_out: bool = False):
    """``F.linear(x, weight, bias)`` for M <= 80 token rows: ``[..., K] -> [..., N]``; with ``residual`` [..., N]:
    ``residual + F.linear(...)`` (the projection rounded first, as the two separate operators do).
    ``norm``: ``F.linear(rmsnorm(x), ...)`` (see NormFold).  ``ssq_out``: returns ``(y, ssq)`` with the partial sums of
    squares of y's rows, the input of the NormFold of the projection that consumes y."""
    out = _linear_call(x, [weight], [bias], _C.LS_EPI_NONE, n_splits, timing, residual=residual, norm=norm, ssq_out=ssq_out)
    if ssq_out:
        return out[0].view(*x.shape[:-1], weight.n), out[1]
    return out.view(*x.shape[:-1], weight.n)


def linear_multi(x: torch.Tensor, weights, biases=None, n_splits: int = 0, timing=None, norm: Optional[NormFold] = None):
    """Several linears of the same input in ONE launch (q|k|v): returns views ``[..., n_i]`` of one
    ``[M, sum n_i]`` buffer."""
    weights = list(weights)
    biases = list(biases) if biases is not None else [None] * len(weights)
    y = _linear_call(x, weights, biases, _C.LS_EPI_NONE, n_splits, timing, norm=norm)
    outs, o = [], 0
    for w in weights:
        outs.append(y[:, o:o + w.n].unflatten(0, x.shape[:-1]))
        o += w.n
    return outs


def linear_qkv_rope(x: torch.Tensor, weights, biases, cos: torch.Tensor, sin: torch.Tensor, n_splits: int = 0, timing=None,
                    norm: Optional[NormFold] = None):
    """``apply_rotary_pos_emb(q_proj(x), k_proj(x), cos, sin)`` and ``v_proj(x)`` (``llama.py:371-378``) in ONE launch:
    the rotation runs in the projection's epilogue on the rounded outputs, with the roundings of ``rope_apply_``.
    ``weights`` = [q] or [q, k] or [q, k, v] (q, k packed with ``rope=True``); cos/sin [rows, 128]."""
    weights = list(weights)
    biases = list(biases) if biases is not None else [None] * len(weights)
    y = _linear_call(x, weights, biases, _C.LS_EPI_QKV_ROPE, n_splits, timing, rope=(cos, sin), norm=norm)
    outs, o = [], 0
    for w in weights:
        outs.append(y[:, o:o + w.n].unflatten(0, x.shape[:-1]))
        o += w.n
    return outs


def mlp_gate_up(x: torch.Tensor, gate_up: PackedWeight, n_splits: int = 0, timing=None, norm: Optional[NormFold] = None):
    """``act_fn(gate_proj(x)) * up_proj(x)`` (SiLU) with the reference's roundings: both projections and the
    activation are rounded to the storage dtype before the product (qwen2.py:229).  ``gate_up`` = pack_gate_up(...)."""
    y = _linear_call(x, [gate_up], None, _C.LS_EPI_SILU_MUL, n_splits, timing, norm=norm)
    return y.view(*x.shape[:-1], gate_up.n)


def causal_mask_bits(n: int, device) -> torch.Tensor:
    """Packed lower-triangular mask [1, n, words]: row r sees new keys j <= r."""
    key = (n, device.index)
    t = _causal_bits.get(key)
    if t is None:
        words = (n + 31) // 32
        rows = []
        for r in range(n):
            v = (1 << (r + 1)) - 1
            rows.append([(v >> (32 * w)) & 0xFFFFFFFF for w in range(words)])
        t = torch.tensor(rows, dtype=torch.int64).to(torch.int32).view(1, n, words).to(device)   # wraps to the same bits
        _causal_bits[key] = t
    return t


def pack_tree_mask(tree_mask: torch.Tensor) -> torch.Tensor:
    """int64 [b,M,N] 0/1 mask -> packed uint32 [b,M,ceil(N/32)] (stored as int32)."""
    _dev(tree_mask)
    if tree_mask.dtype != torch.int64:
        tree_mask = tree_mask.to(torch.int64)
    tree_mask = tree_mask.contiguous()
    b, M, N = tree_mask.shape
    words = (N + 31) // 32
    bits = torch.empty((b, M, words), dtype=torch.int32, device=tree_mask.device)
    lib = _C.load()
    _C.check(lib.ls_pack_tree_mask(tree_mask.data_ptr(), b, M, N, bits.data_ptr(), words, _stream()), "ls_pack_tree_mask")
    return bits


def _check_qkv(q, k_cache, v_cache):
    if q.dim() != 4 or q.shape[-1] != 128:
        raise ValueError(f"q must be [b,sq,H,128], got {tuple(q.shape)}")
    if k_cache.dim() != 4 or k_cache.shape[-1] != 128 or k_cache.shape != v_cache.shape:
        raise ValueError("k_cache/v_cache must be [b,S,Hkv,128] and equal-shaped")
    if q.stride(-1) != 1 or k_cache.stride(-1) != 1 or v_cache.stride(-1) != 1:
        raise ValueError("innermost dimension must be contiguous")
    if k_cache.stride() != v_cache.stride():
        raise ValueError("k_cache and v_cache must share strides")
    if k_cache.dtype != q.dtype or v_cache.dtype != q.dtype:
        raise TypeError("q/k_cache/v_cache dtypes differ")


def _desc(q, k_cache, v_cache, cache_seqlens, kv_len_hint, k_new=None, v_new=None, mask_bits=None, out=None,
          lse=None, new_mode=LS_NEW_NONE, n_new=0, n_new_cached=0, scatter_new=0, causal=False, window_left=-1,
          n_app=0, prescale_q=False, softmax_scale=None, n_splits=0, timing=None) -> AttnDesc:
    b, sq, H, D = q.shape
    Hkv = k_cache.shape[2]
    d = AttnDesc()
    d.q = q.data_ptr()
    d.k_cache = k_cache.data_ptr()
    d.v_cache = v_cache.data_ptr()
    d.k_new = k_new.data_ptr() if k_new is not None else None
    d.v_new = v_new.data_ptr() if v_new is not None else None
    if cache_seqlens.dtype != torch.int32:
        cache_seqlens = cache_seqlens.to(torch.int32)
    d._keep = (cache_seqlens,)          # keep the converted tensor alive for the launch
    d.cache_seqlens = cache_seqlens.data_ptr()
    d.mask_bits = mask_bits.data_ptr() if mask_bits is not None else None
    d.out = out.data_ptr() if out is not None else None
    d.lse = lse.data_ptr() if lse is not None else None
    if timing is not None:          # (torch.cuda.Event, torch.cuda.Event), both already created by a record()
        d.ev_start, d.ev_stop = timing[0].cuda_event, timing[1].cuda_event
    d.b, d.sq, d.H, d.Hkv = b, sq, H, Hkv
    d.dtype = _dtype(q)
    d.new_mode = new_mode
    d.n_new = n_new
    d.n_new_cached = n_new_cached
    d.mask_words = mask_bits.shape[-1] if mask_bits is not None else 0
    d.scatter_new = int(scatter_new)
    d.causal = int(causal)
    d.window_left = int(window_left)
    d.n_app = int(n_app)
    d.prescale_q = int(prescale_q)
    d.kv_len_hint = int(kv_len_hint)
    d.n_splits = int(n_splits)
    d.softmax_scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    d.q_stride_b, d.q_stride_s, d.q_stride_h = q.stride(0), q.stride(1), q.stride(2)
    d.kc_stride_b, d.kc_stride_s, d.kc_stride_h = k_cache.stride(0), k_cache.stride(1), k_cache.stride(2)
    if k_new is not None:
        if k_new.stride() != v_new.stride() or k_new.stride(-1) != 1:
            raise ValueError("k_new/v_new must share strides and be contiguous in the last dim")
        d.kn_stride_b, d.kn_stride_s, d.kn_stride_h = k_new.stride(0), k_new.stride(1), k_new.stride(2)
    if out is not None:
        d.out_stride_b, d.out_stride_s, d.out_stride_h = out.stride(0), out.stride(1), out.stride(2)
    return d


def _hint(cache_seqlens, kv_len_hint, k_cache):
    if kv_len_hint is None:
        # no host-side bound known: size the grid for the whole cache allocation (no sync)
        return int(k_cache.shape[1])
    return int(kv_len_hint)


def _run(d: AttnDesc, device):
    lib = _C.load()
    nbytes = lib.ls_attn_workspace_bytes(C.byref(d))
    if nbytes == 0:
        _C.check(-1, "ls_attn_workspace_bytes")
    ws = _ws.get(device, nbytes)
    _C.check(lib.ls_attn_fwd(C.byref(d), ws.data_ptr(), ws.numel(), _stream()), "ls_attn_fwd")


def attn_kernel_name(M: int, verify: bool = True) -> str:
    """Name of the stage-1 kernel a verification call with ``M = (H / Hkv) * sq`` rows per kv head is served by
    (benchmark labels; ``ls_attn_kernel_name``)."""
    d = AttnDesc()
    d.b, d.sq, d.H, d.Hkv, d.dtype = 1, M, 1, 1, LS_F16
    d.window_left = -1
    d.q = d.k_cache = d.v_cache = d.cache_seqlens = 1            # non-null placeholders: nothing is dereferenced
    d.q_stride_s = d.q_stride_h = d.kc_stride_s = d.kc_stride_h = 128
    if verify:
        d.new_mode, d.n_new, d.mask_words, d.mask_bits, d.k_new, d.v_new = LS_NEW_TARGET, min(M, 74), 3, 1, 1, 1
    name = _C.load().ls_attn_kernel_name(C.byref(d))
    return name.decode() if name else "?"


def kvcache_attention(q, k_cache, v_cache, k=None, v=None, cache_seqlens=None, causal=False, window_size=(-1, -1),
                      return_softmax_lse=False, softmax_scale=None, kv_len_hint: Optional[int] = None, n_splits=0):
    """``flash_attn_with_kvcache`` as the reference uses it.  New
    ``k``/``v`` rows are appended IN PLACE at ``cache_seqlens`` and attended causally
    (the reference only appends with ``causal=True``)."""
    _dev(q, k_cache, v_cache, k, v, cache_seqlens)
    _check_qkv(q, k_cache, v_cache)
    b, sq, H, D = q.shape
    if window_size[1] not in (-1, 0):
        raise NotImplementedError("right window other than -1/0")
    out = torch.empty((b, sq, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((b, H, sq), dtype=torch.float32, device=q.device) if return_softmax_lse else None
    hint = _hint(cache_seqlens, kv_len_hint, k_cache)
    if k is not None:
        if not causal:
            raise NotImplementedError("append without causal=True is not a reference call pattern")
        n = k.shape[1]
        if n != sq:
            raise ValueError("appended rows must equal query rows")
        bits = causal_mask_bits(n, q.device).expand(b, -1, -1).contiguous()
        d = _desc(q, k_cache, v_cache, cache_seqlens, hint, k_new=k, v_new=v, mask_bits=bits, out=out, lse=lse,
                  new_mode=LS_NEW_FLASH, n_new=n, scatter_new=1, causal=True, window_left=window_size[0], n_app=n,
                  softmax_scale=softmax_scale, n_splits=n_splits)
    else:
        d = _desc(q, k_cache, v_cache, cache_seqlens, hint, out=out, lse=lse, causal=causal or window_size[1] == 0,
                  window_left=window_size[0], softmax_scale=softmax_scale, n_splits=n_splits)
    _run(d, q.device)
    return (out, lse) if return_softmax_lse else out


PREFILL_CHUNK = 64


def prefill_attention(q, k, v, k_cache, v_cache, window_left: int = -1, start: int = 0, total: Optional[int] = None):
    """Prompt attention (K13) through the decode kernels: the prompt is appended to the (empty)
    caches ``PREFILL_CHUNK`` rows at a time with the causal(+window) append form of
    ``kvcache_attention`` -- the same function as ``flash_attn_func(causal=True[, window])``
    (``llama.py:218``, ``llama_glide.py:227``), evaluated block-wise.  [b,L,H,128] -> [b,L,H,128];
    fills ``k_cache/v_cache[:, start:start + L]``.  ``start`` > 0: the rows are positions [start, start + L) of a
    prompt of ``total`` rows whose first ``start`` rows are already in the caches (sequence-sharded prefill).  The chunk
    size follows from the WHOLE prompt and chunk boundaries sit at multiples of it counted from global row 0, so a rank
    of a sharded prefill makes the very calls the single-GPU prefill makes for its rows -- except for the one chunk a shard
    boundary cuts in two (<= chunk rows per boundary: same function, other block split, equal within the fp16 tolerance)."""
    b, L, H, D = q.shape
    total = start + L if total is None else int(total)
    CH = prefill_chunk(total, H // k.shape[2], window_left)
    head = min(L, (-start) % CH)                 # rows up to the next global chunk boundary
    outs = []
    if head:
        lens = torch.full((b,), start, dtype=torch.int32, device=q.device)
        outs.append(kvcache_attention(q[:, :head], k_cache, v_cache, k[:, :head], v[:, :head], cache_seqlens=lens,
                                      causal=True, window_size=(window_left, -1), kv_len_hint=start))
    if b == 1 and (L - head) // CH >= 2:
        outs.append(_prefill_attention_batched(q[:, head:], k[:, head:], v[:, head:], k_cache, v_cache, window_left, start + head, CH))
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)
    for s0 in range(head, L, CH):
        s1 = min(L, s0 + CH)
        lens = torch.full((b,), start + s0, dtype=torch.int32, device=q.device)
        outs.append(kvcache_attention(q[:, s0:s1], k_cache, v_cache, k[:, s0:s1], v[:, s0:s1], cache_seqlens=lens,
                                      causal=True, window_size=(window_left, -1), kv_len_hint=start + s0))
    return torch.cat(outs, dim=1)


def prefill_chunk(total: int, g: int, window_left: int) -> int:
    """Prompt rows per chunk, a function of the WHOLE prompt (``total`` rows) only.  Long prompts of GQA models (g = H / Hkv
    >= 4) use g * chunk = 257..320 rows, which puts the prefix part of every chunk on the streaming MFMA kernel (ws_eligible:
    append chunks with kv_len_hint >= 4096); short prompts, windows and small groups keep 64 (the chunking the
    reference-generated goldens were checked against)."""
    if window_left < 0 and g >= 4 and total >= 8192 and 320 // g >= 32:
        return 320 // g
    return PREFILL_CHUNK


PREFILL_GROUP = 512       # prompt chunks per launch (bounds the fp32 workspace: 3 x group x 64 rows x H x 512 B)
PREFILL_SPLITS = 2        # key splits per chunk: with ONE, the ~32 chunks resident at a time walk the same K/V lines in lock
                          # step (measured 0.34 s per layer at 128k against 0.18 s); an ODD count leaves two of the eight XCDs
                          # with the light new-block workgroups only (grid.x = splits + 1, XCD = linear id % 8)


def _prefill_attention_batched(q, k, v, k_cache, v_cache, window_left, start, CH=PREFILL_CHUNK):
    """The same chunk-wise evaluation with the chunks of a prompt as the BATCH of one call: chunk c is batch element c
    with ``cache_seqlens[c] = start + 64 c`` over the one shared cache (batch stride 0; the prompt's K/V rows are copied
    into it first, so nothing is scattered by the launch), its 64 rows are the appended block with the causal mask.  One
    two key splits per element (thousands of workgroups as it is): no per-chunk launches, 16x fewer split partials -- a
    128k prompt is 4 launches per layer instead of 4096.  One layer (tools/bench_prefill.py): 16k 0.0046 s (0.0092 chunk
    by chunk), 64k 0.049 (0.060), 128k 0.181 (0.191)."""
    _dev(q, k, v, k_cache, v_cache)
    _check_qkv(q, k_cache, v_cache)
    b, L, H, D = q.shape
    Hkv = k.shape[2]
    n_full = L // CH
    k_cache[:, start:start + L] = k
    v_cache[:, start:start + L] = v
    out = torch.empty((b, L, H, D), dtype=q.dtype, device=q.device)
    bits1 = causal_mask_bits(CH, q.device)
    kc = k_cache.as_strided((1, k_cache.shape[1], Hkv, D), (0, k_cache.stride(1), k_cache.stride(2), 1))
    vc = v_cache.as_strided((1, v_cache.shape[1], Hkv, D), (0, v_cache.stride(1), v_cache.stride(2), 1))
    for c0 in range(0, n_full, PREFILL_GROUP):
        n = min(PREFILL_GROUP, n_full - c0)
        r0 = c0 * CH

        def chunks(t):      # [1, L, h, D] rows r0 .. r0 + n*CH as [n, CH, h, D] without a copy
            return t.as_strided((n, CH, t.shape[2], D), (CH * t.stride(1), t.stride(1), t.stride(2), 1),
                                t.storage_offset() + r0 * t.stride(1))
        lens = (torch.arange(n, dtype=torch.int32, device=q.device) * CH + (start + r0))
        d = _desc(chunks(q), kc.expand(n, -1, -1, -1), vc.expand(n, -1, -1, -1), lens, start + r0 + n * CH, k_new=chunks(k),
                  v_new=chunks(v), mask_bits=bits1.expand(n, -1, -1).contiguous(), out=chunks(out), new_mode=LS_NEW_FLASH,
                  n_new=CH, scatter_new=0, causal=True, window_left=window_left, n_app=CH, n_splits=PREFILL_SPLITS)
        _run(d, q.device)
    if n_full * CH < L:       # the ragged tail: one ordinary call
        s0 = n_full * CH
        lens = torch.full((b,), start + s0, dtype=torch.int32, device=q.device)
        out[:, s0:] = kvcache_attention(q[:, s0:], k_cache, v_cache, k[:, s0:], v[:, s0:], cache_seqlens=lens, causal=True,
                                        window_size=(window_left, -1), kv_len_hint=start + s0)
    return out


def verify_attention(q, k_new, v_new, k_cache, v_cache, cache_lens, mask_bits, last_layer: bool,
                     softmax_scale: float = 1.0 / (128 ** 0.5), kv_len_hint: Optional[int] = None, n_splits=0, timing=None):
    """Hybrid tree-verification attention of one target layer (K1+K2+K3 fused):
    prefix flash-decoding over ``cache[:, :cache_lens]`` + scatter of the R new K/V rows at
    ``cache_lens`` + tree-masked part + fp16 merge.  ``mask_bits`` = ``pack_tree_mask`` of
    the [b,R,R] verification mask.  Returns [b,R,H,128]."""
    _dev(q, k_new, v_new, k_cache, v_cache, cache_lens, mask_bits)
    _check_qkv(q, k_cache, v_cache)
    b, R, H, D = q.shape
    out = torch.empty((b, R, H, D), dtype=q.dtype, device=q.device)
    d = _desc(q, k_cache, v_cache, cache_lens, _hint(cache_lens, kv_len_hint, k_cache), k_new=k_new, v_new=v_new,
              mask_bits=mask_bits, out=out, new_mode=LS_NEW_TARGET, n_new=R, scatter_new=1, prescale_q=last_layer,
              softmax_scale=softmax_scale, n_splits=n_splits, timing=timing)
    _run(d, q.device)
    return out


def draft_tree_attention(q, k_new, v_new, k_cache, v_cache, cache_lens, mask_bits, N: int, window: int = 512,
                         kv_len_hint: Optional[int] = None):
    """Draft self-attention of a tree step (K5+K6 fused): window prefix over rows [0,p) +
    scatter of the M new rows at ``p + [N-M, N)`` + tree-masked part over rows ``p + [0,N)``
    + fp32 merge.  ``cache_lens`` = p.  Returns [b,M,H,128]."""
    _dev(q, k_new, v_new, k_cache, v_cache, cache_lens, mask_bits)
    _check_qkv(q, k_cache, v_cache)
    b, M, H, D = q.shape
    out = torch.empty((b, M, H, D), dtype=q.dtype, device=q.device)
    d = _desc(q, k_cache, v_cache, cache_lens, _hint(cache_lens, kv_len_hint, k_cache), k_new=k_new, v_new=v_new,
              mask_bits=mask_bits, out=out, new_mode=LS_NEW_DRAFT, n_new=N, n_new_cached=N - M, scatter_new=1,
              window_left=window)
    _run(d, q.device)
    return out


def tree_attention(q, k, v, tree_mask, sm_scale=None):
    """``triton_tree_attn.attention(q, k, v, tree_mask)`` (``longspec/test/triton_tree_attn.py:19-77``):
    q [B,H,M,128], k/v [B,Hkv,N,128], tree_mask [B,M,N] (non-zero = visible) -> (o [B,H,M,128], L [B,H,M] fp32).
    Runs the draft-mode new-block path over an empty prefix."""
    _dev(q, k, v, tree_mask)
    B, H, M, D = q.shape
    Hkv, N = k.shape[1], k.shape[2]
    qt = q.permute(0, 2, 1, 3).contiguous()
    kt = k.permute(0, 2, 1, 3).contiguous()
    vt = v.permute(0, 2, 1, 3).contiguous()
    out = torch.empty((B, M, H, D), dtype=q.dtype, device=q.device)
    L = torch.empty((B, H, M), dtype=torch.float32, device=q.device)
    zeros = torch.zeros((B,), dtype=torch.int32, device=q.device)
    bits = pack_tree_mask(tree_mask)
    # the keys double as an (unread) one-row-per-key "cache": cache_seqlens = 0 makes the prefix empty
    d = _desc(qt, kt, vt, zeros, 0, k_new=kt, v_new=vt, mask_bits=bits, out=out, lse=L, new_mode=LS_NEW_DRAFT, n_new=N,
              softmax_scale=sm_scale)
    _run(d, q.device)
    return out.permute(0, 2, 1, 3), L


def lse_merge(parts_o: torch.Tensor, parts_lse: torch.Tensor, dtype=None, want_o32=False):
    """parts_o [W,b,sq,H,128] fp32, parts_lse [W,b,H,sq] fp32 -> merged out (dtype) and/or (o32, lse)."""
    _dev(parts_o, parts_lse)
    W, b, sq, H, D = parts_o.shape
    parts_o = parts_o.contiguous()
    parts_lse = parts_lse.contiguous()
    out = torch.empty((b, sq, H, D), dtype=dtype, device=parts_o.device) if dtype is not None else None
    o32 = torch.empty((b, sq, H, D), dtype=torch.float32, device=parts_o.device) if want_o32 else None
    lse = torch.empty((b, H, sq), dtype=torch.float32, device=parts_o.device)
    lib = _C.load()
    _C.check(lib.ls_lse_merge(parts_o.data_ptr(), parts_lse.data_ptr(), W, b, sq, H,
                              _DT[dtype] if dtype is not None else 0,
                              out.data_ptr() if out is not None else None,
                              o32.data_ptr() if o32 is not None else None, lse.data_ptr(), _stream()), "ls_lse_merge")
    return out, o32, lse


# ---- multi-GPU building blocks (sequence-sharded prefix KV) -------------------------------------
class ShardedAttnCall:
    """Stage 1 / exchange / stage 2 of one attention call whose prefix KV is sharded by sequence
    over ranks.  ``partial(sendbuf)`` writes this rank's normalised prefix partial
    ``[o32 (b*sq*H*128) | lse (b*H*sq)]`` into ``sendbuf`` (fp32); after an all-gather of those
    records, ``finish(gathered)`` merges the W records in rank order (deterministic, identical on
    every rank) with the locally computed new-block part."""

    def __init__(self, desc: AttnDesc, out: torch.Tensor, device):
        self.d = desc
        self.out = out
        self.device = device
        lib = _C.load()
        nbytes = lib.ls_attn_workspace_bytes(C.byref(desc))
        if nbytes == 0:
            _C.check(-1, "ls_attn_workspace_bytes")
        self.ws = _ws.get(device, nbytes)       # stream-ordered: stage 2 runs before the next call reuses it
        self.n_o = desc.b * desc.sq * desc.H * 128
        self.n_lse = desc.b * desc.H * desc.sq
        self.xchg_timing = None                 # optional (start, stop) torch events around the exchange + merge (bench.py)

    @property
    def record_floats(self) -> int:
        return self.n_o + self.n_lse

    def partial(self, sendbuf: torch.Tensor) -> torch.Tensor:
        lib = _C.load()
        d = self.d
        assert sendbuf.dtype == torch.float32 and sendbuf.numel() >= self.record_floats and sendbuf.is_contiguous()
        _C.check(lib.ls_attn_partial(C.byref(d), self.ws.data_ptr(), self.ws.numel(), _stream()), "ls_attn_partial")
        _C.check(lib.ls_attn_reduce_local(C.byref(d), self.ws.data_ptr(), self.ws.numel(), sendbuf.data_ptr(),
                                          sendbuf.data_ptr() + 4 * self.n_o, _stream()), "ls_attn_reduce_local")
        return sendbuf

    def attend_peer(self, xchg) -> torch.Tensor:
        """partial -> reduce + peer stores -> wait + merge: the exchange rides inside the two combine kernels
        (``xchg`` = the ``ls_xchg*`` of ``dist.PeerExchange``).  Kernel launches only: graph-capturable."""
        lib = _C.load()
        d = self.d
        ws, n, st = self.ws.data_ptr(), self.ws.numel(), _stream()
        _C.check(lib.ls_attn_partial(C.byref(d), ws, n, st), "ls_attn_partial")
        if self.xchg_timing is not None:
            self.xchg_timing[0].record()
        _C.check(lib.ls_attn_reduce_push(C.byref(d), ws, n, xchg, st), "ls_attn_reduce_push")
        _C.check(lib.ls_attn_finish_xchg(C.byref(d), xchg, ws, n, st), "ls_attn_finish_xchg")
        if self.xchg_timing is not None:
            self.xchg_timing[1].record()
        return self.out

    def finish(self, gathered: torch.Tensor) -> torch.Tensor:
        """gathered: fp32 [W, record_floats] (row w = rank w's record)."""
        lib = _C.load()
        assert gathered.dtype == torch.float32 and gathered.is_contiguous() and gathered.shape[1] >= self.record_floats
        W, stride = gathered.shape[0], gathered.stride(0)
        _C.check(lib.ls_attn_finish(C.byref(self.d), gathered.data_ptr(), gathered.data_ptr() + 4 * self.n_o, W, stride,
                                    stride, self.ws.data_ptr(), self.ws.numel(), _stream()), "ls_attn_finish")
        return self.out


def sharded_verify_attention(q, k_new, v_new, k_cache, v_cache, local_lens, mask_bits, last_layer,
                             softmax_scale=1.0 / (128 ** 0.5), kv_len_hint=None, timing=None) -> ShardedAttnCall:
    """Like ``verify_attention`` but ``k_cache/v_cache`` hold only this rank's prefix rows
    (``local_lens`` valid rows); the new rows are scattered at ``local_lens`` of the LOCAL cache
    (only the tail-owning rank's copy is ever read back as prefix)."""
    _dev(q, k_new, v_new, k_cache, v_cache, local_lens, mask_bits)
    _check_qkv(q, k_cache, v_cache)
    b, R, H, D = q.shape
    out = torch.empty((b, R, H, D), dtype=q.dtype, device=q.device)
    d = _desc(q, k_cache, v_cache, local_lens, _hint(local_lens, kv_len_hint, k_cache), k_new=k_new, v_new=v_new,
              mask_bits=mask_bits, out=out, new_mode=LS_NEW_TARGET, n_new=R, scatter_new=1, prescale_q=last_layer,
              softmax_scale=softmax_scale, timing=timing)
    return ShardedAttnCall(d, out, q.device)


def sharded_prefix_attention(q, k_cache, v_cache, local_lens, causal=False, kv_len_hint=None) -> ShardedAttnCall:
    """Prefix attention over a local KV shard (draft cross-attention, K7).  ``causal`` only on the
    rank that owns the tail of the sequence (all keys of the other shards precede every query)."""
    _dev(q, k_cache, v_cache, local_lens)
    _check_qkv(q, k_cache, v_cache)
    b, R, H, D = q.shape
    out = torch.empty((b, R, H, D), dtype=q.dtype, device=q.device)
    d = _desc(q, k_cache, v_cache, local_lens, _hint(local_lens, kv_len_hint, k_cache), out=out, causal=causal)
    return ShardedAttnCall(d, out, q.device)


# ---- RMSNorm / RoPE ----------------------------------------------------------------------------------
def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float, residual: Optional[torch.Tensor] = None):
    """y = LlamaRMSNorm(x [+ residual]).  With ``residual`` returns (y, x + residual)."""
    _dev(x, weight, residual)
    hidden = x.shape[-1]
    xc = x.contiguous()
    rows = xc.numel() // hidden
    y = torch.empty_like(xc)
    lib = _C.load()
    if residual is not None:
        rc = residual.contiguous()
        s = torch.empty_like(xc)
        _C.check(lib.ls_rmsnorm_fwd(xc.data_ptr(), rc.data_ptr(), weight.data_ptr(), y.data_ptr(), s.data_ptr(), rows,
                                    hidden, eps, _dtype(x), _stream()), "ls_rmsnorm_fwd")
        return y.view(x.shape), s.view(x.shape)
    _C.check(lib.ls_rmsnorm_fwd(xc.data_ptr(), None, weight.data_ptr(), y.data_ptr(), None, rows, hidden, eps,
                                _dtype(x), _stream()), "ls_rmsnorm_fwd")
    return y.view(x.shape)


def rope_cos_sin(position_ids: torch.Tensor, inv_freq: torch.Tensor, attention_scaling: float, dtype):
    """position_ids [b,R] int64, inv_freq [64] fp32 -> cos, sin [b,R,128] dtype."""
    _dev(position_ids, inv_freq)
    pos = position_ids.to(torch.int64).contiguous()
    b, R = pos.shape
    cos = torch.empty((b, R, 128), dtype=dtype, device=pos.device)
    sin = torch.empty((b, R, 128), dtype=dtype, device=pos.device)
    lib = _C.load()
    _C.check(lib.ls_rope_cos_sin(pos.data_ptr(), inv_freq.data_ptr(), float(attention_scaling), cos.data_ptr(),
                                 sin.data_ptr(), b * R, _DT[dtype], _stream()), "ls_rope_cos_sin")
    return cos, sin


def rope_apply_(q: torch.Tensor, k: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor):
    """In-place apply_rotary_pos_emb(unsqueeze_dim=2) on q [b,R,Hq,128], k [b,R,Hk,128]
    (views into a fused QKV buffer are fine: only the row stride must be uniform)."""
    _dev(q, k, cos, sin)
    b, R, Hq, D = q.shape
    Hk = k.shape[2]
    for t in (q, k):
        if t.stride(-1) != 1 or t.stride(2) != 128 or (b > 1 and t.stride(0) != R * t.stride(1)):
            raise ValueError("rope_apply_: heads must be packed (stride 128) and rows uniformly strided")
    # the kernel reads one cos / sin row per (batch, position) row: a table of one batch row -- a batched prefill, whose
    # position_ids are [1, R] -- is broadcast over the batch as apply_rotary_pos_emb does, never read past its end
    if cos.shape != sin.shape or cos.dtype != q.dtype or sin.dtype != q.dtype or cos.numel() not in (R * 128, b * R * 128):
        raise ValueError(f"rope_apply_: cos / sin must be [1 or {b}, {R}, 128] tables of q's dtype, got {tuple(cos.shape)}")
    if cos.numel() != b * R * 128:
        cos, sin = cos.reshape(1, R, 128).expand(b, R, 128), sin.reshape(1, R, 128).expand(b, R, 128)
    cos, sin = cos.contiguous(), sin.contiguous()
    lib = _C.load()
    _C.check(lib.ls_rope_apply(q.data_ptr(), k.data_ptr(), cos.data_ptr(), sin.data_ptr(), b * R, Hq, Hk, q.stride(1),
                               k.stride(1), _dtype(q), _stream()), "ls_rope_apply")
    return q, k


def tree_positions(tree_mask: torch.Tensor, base: Optional[torch.Tensor]) -> torch.Tensor:
    """position_ids = tree_mask.sum(-1) - 1 + base[:, None]  (llama.py:575-577)."""
    _dev(tree_mask, base)
    tm = tree_mask.to(torch.int64).contiguous()
    b, M, N = tm.shape
    pos = torch.empty((b, M), dtype=torch.int64, device=tm.device)
    if base is not None and base.dtype != torch.int32:
        base = base.to(torch.int32)
    lib = _C.load()
    _C.check(lib.ls_tree_positions(tm.data_ptr(), base.data_ptr() if base is not None else None, b, M, N,
                                   pos.data_ptr(), _stream()), "ls_tree_positions")
    return pos


def _tree_state(tree_mask, all_spec, logp_sum=None):
    """The in-place tree operators work on the round's state tensors as they are."""
    b, Fn = all_spec.shape
    if tree_mask.dtype != torch.int64 or all_spec.dtype != torch.int64 or tuple(tree_mask.shape) != (b, Fn, Fn):
        raise TypeError("tree state: tree_mask [b,F,F] and all_spec [b,F] must be int64")
    if not (tree_mask.is_contiguous() and all_spec.is_contiguous()):
        raise ValueError("tree state tensors must be contiguous")
    if logp_sum is not None and (logp_sum.dtype != torch.float32 or tuple(logp_sum.shape) != (b, Fn) or not logp_sum.is_contiguous()):
        raise TypeError("tree state: logp_sum must be contiguous fp32 [b,F]")
    return b, Fn


def _len_i32(t, b, name):
    if t is None:
        return None
    if t.dtype != torch.int32 or t.numel() != b or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous int32 [b] tensor (it is updated in place)")
    return t.data_ptr()


def tree_grow(tree_mask, all_spec, logp_sum, topk_vals, topk_idx, vocab: int, lo: int, mid: int,
              base: Optional[torch.Tensor] = None, base_add: int = 0, want_next: bool = True):
    """One more tree level, in place on the round's state (``llama_glide.py:1021-1027``, ``:1056-1075``):
    node mid+j = child of node ``lo + topk_idx[j] // vocab`` with token ``topk_idx[j] % vocab`` and cumulative
    log-prob ``topk_vals[j]``; its mask row = the father's row + the diagonal.  Returns (position_ids [b,k],
    packed mask bits [b,k,words]) of the new level for the draft pass that runs next (None, None when
    ``want_next`` is False); ``base`` [b] int32 is the draft cache length and is advanced by ``base_add`` first."""
    _dev(tree_mask, all_spec, logp_sum, topk_vals, topk_idx, base)
    b, Fn = _tree_state(tree_mask, all_spec, logp_sum)
    k = topk_idx.shape[-1]
    vals = topk_vals.to(torch.float32).contiguous().view(b, k)
    idx = topk_idx.to(torch.int64).contiguous().view(b, k)
    pos = bits = None
    words = (mid + k + 31) // 32
    if want_next:
        pos = torch.empty((b, k), dtype=torch.int64, device=idx.device)
        bits = torch.empty((b, k, words), dtype=torch.int32, device=idx.device)
    lib = _C.load()
    _C.check(lib.ls_tree_grow(tree_mask.data_ptr(), all_spec.data_ptr(), logp_sum.data_ptr(), vals.data_ptr(), idx.data_ptr(),
                              b, Fn, k, int(vocab), lo, mid, _len_i32(base, b, "base"), base_add,
                              pos.data_ptr() if want_next else None, bits.data_ptr() if want_next else None, words, _stream()),
             "ls_tree_grow")
    return pos, bits


def tree_verify_inputs(acc_ids, a: int, all_spec, tree_mask, cache_lens, R: int, bump: Optional[torch.Tensor] = None,
                       bump_add: int = 0):
    """Token ids, position ids and packed tree mask of the R-row verification pass (``llama_glide.py:1078-1086``):
    rows = [a accepted tokens | the F-1 tree nodes | pads].  ``bump`` [b] int32 += ``bump_add`` (:1076)."""
    _dev(acc_ids, all_spec, tree_mask, cache_lens, bump)
    b, Fn = _tree_state(tree_mask, all_spec)
    if acc_ids.dtype != torch.int64 or acc_ids.dim() != 2 or acc_ids.shape[1] < a or acc_ids.stride(1) != 1:
        raise TypeError("acc_ids must be int64 [b, >=a] with a contiguous last dimension")
    dev = all_spec.device
    words = (R + 31) // 32
    veri = torch.empty((b, R), dtype=torch.int64, device=dev)
    pos = torch.empty((b, R), dtype=torch.int64, device=dev)
    bits = torch.empty((b, R, words), dtype=torch.int32, device=dev)
    lib = _C.load()
    _C.check(lib.ls_tree_verify_inputs(acc_ids.data_ptr(), acc_ids.stride(0), a, all_spec.data_ptr(), tree_mask.data_ptr(), b, Fn,
                                       R, _len_i32(cache_lens, b, "cache_lens"), veri.data_ptr(), pos.data_ptr(),
                                       bits.data_ptr(), words, _len_i32(bump, b, "bump"), bump_add, _stream()),
             "ls_tree_verify_inputs")
    return veri, pos, bits


def tree_collapse(all_spec, all_llm_pred, tree_mask, cache_lens, non_leaf_len: int, max_acc: int,
                  k_cache: Optional[torch.Tensor] = None, v_cache: Optional[torch.Tensor] = None, cache_len_add: int = 0,
                  out_acc_ids: Optional[torch.Tensor] = None):
    """Accept/reject tree collapse + last-layer KV row move, one launch, no host sync.
    Returns (acc_ids [b,max_acc] int64 zero-padded, acc_num [b] int64, double_input [b] int32,
    index_mapping [b,max_acc] int64, -1 padded).  The moved rows start at ``cache_lens + cache_len_add``.
    ``out_acc_ids``: a persistent [b,max_acc] int64 buffer to write the accepted ids into."""
    _dev(all_spec, all_llm_pred, tree_mask, cache_lens, k_cache, v_cache)
    b, Fn = all_spec.shape
    dev = all_spec.device
    spec = all_spec.to(torch.int64).contiguous()
    pred = all_llm_pred.to(torch.int64).contiguous()
    tm = tree_mask.to(torch.int64).contiguous()
    cl = cache_lens.to(torch.int32).contiguous()
    if out_acc_ids is not None:
        if out_acc_ids.dtype != torch.int64 or tuple(out_acc_ids.shape) != (b, max_acc) or not out_acc_ids.is_contiguous():
            raise TypeError("tree_collapse: out_acc_ids must be a contiguous int64 [b, max_acc] tensor")
        acc_ids = out_acc_ids
    else:
        acc_ids = torch.empty((b, max_acc), dtype=torch.int64, device=dev)
    acc_num = torch.empty((b,), dtype=torch.int64, device=dev)
    dbl = torch.empty((b,), dtype=torch.int32, device=dev)
    imap = torch.empty((b, max_acc), dtype=torch.int64, device=dev)
    lib = _C.load()
    if k_cache is not None:
        if k_cache.stride() != v_cache.stride() or k_cache.stride(3) != 1 or k_cache.stride(2) != k_cache.shape[3]:
            raise ValueError("tree_collapse: cache rows must be contiguous [Hkv*D]")
        row_elems = k_cache.shape[2] * k_cache.shape[3]
        _C.check(lib.ls_tree_collapse(spec.data_ptr(), pred.data_ptr(), tm.data_ptr(), cl.data_ptr(), cache_len_add, b, Fn,
                                      non_leaf_len, max_acc, acc_ids.data_ptr(), acc_num.data_ptr(), dbl.data_ptr(),
                                      imap.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.stride(0),
                                      k_cache.stride(1), row_elems, _dtype(k_cache), _stream()), "ls_tree_collapse")
    else:
        _C.check(lib.ls_tree_collapse(spec.data_ptr(), pred.data_ptr(), tm.data_ptr(), cl.data_ptr(), cache_len_add, b, Fn,
                                      non_leaf_len, max_acc, acc_ids.data_ptr(), acc_num.data_ptr(), dbl.data_ptr(),
                                      imap.data_ptr(), None, None, 0, 0, 0, 0, _stream()), "ls_tree_collapse")
    return acc_ids, acc_num, dbl, imap


MT_WORDS = 512           # raw Mersenne-Twister words handed to a stochastic verification (a walk uses <= ~3 per child drawn)


def tree_verify_stochastic(all_spec, tree_mask, llm_logits, spec_logp, temperature: float, mt_words, exp_noise, max_acc: int):
    """``LlamaGlide.verify_stochastic`` (``llama_glide.py:1177-1245``) on the device with pre-drawn randomness
    (``ls_tree_verify_stochastic``): returns (acc_ids [b,max_acc], acc_num [b], words_used [b] int32)."""
    _dev(all_spec, tree_mask, llm_logits, spec_logp, mt_words, exp_noise)
    b, Fn = all_spec.shape
    V = llm_logits.shape[-1]
    if llm_logits.stride(-1) != 1 or spec_logp.stride(-1) != 1 or spec_logp.dtype != torch.float32:
        raise ValueError("logits must be contiguous in the vocabulary, draft log-probs fp32")
    if mt_words.dtype != torch.int32 and mt_words.dtype != torch.uint32:
        raise TypeError("mt_words: 32-bit words")
    all_spec, tree_mask = all_spec.contiguous(), tree_mask.contiguous()
    exp_noise = exp_noise.to(llm_logits.dtype).contiguous()
    dev = all_spec.device
    acc_ids = torch.empty((b, max_acc), dtype=torch.int64, device=dev)
    acc_num = torch.empty((b,), dtype=torch.int64, device=dev)
    used = torch.empty((b,), dtype=torch.int32, device=dev)
    ws = torch.empty((b, V), dtype=torch.float32, device=dev)
    _C.check(_C.load().ls_tree_verify_stochastic(
        all_spec.data_ptr(), tree_mask.data_ptr(), llm_logits.data_ptr(), llm_logits.stride(0), llm_logits.stride(1),
        spec_logp.data_ptr(), spec_logp.stride(0), spec_logp.stride(1), b, Fn, spec_logp.shape[1], V, _dtype(llm_logits),
        float(temperature), mt_words.data_ptr(), mt_words.shape[-1], exp_noise.data_ptr(), acc_ids.data_ptr(), max_acc,
        acc_num.data_ptr(), used.data_ptr(), ws.data_ptr(), _stream()), "ls_tree_verify_stochastic")
    return acc_ids, acc_num, used


stochastic_noise_fn = None     # tests replay the reference's CPU generator: fn(V, dtype, device) -> Exponential(1) row


def verify_stochastic(input_ids, tree_mask, p_llm, p_ssm, temperature: float):
    """``LlamaGlide.verify_stochastic(input_ids, tree_mask, p_llm, p_ssm, temperature)`` (``llama_glide.py:1177-1245``).
    The randomness is the reference's: Python's ``random`` stream (choice / random) and one ``exponential_`` row per batch
    element from torch (what ``torch.multinomial(p, 1)`` draws); the walk itself runs on the device.  After the launch
    Python's generator is advanced by exactly the words the walk consumed.  One host read per batch row."""
    import random
    import numpy as np
    b, Fn = input_ids.shape
    V = p_llm.shape[-1]
    width = int(tree_mask.sum(-1).max()) + 1                      # :1193 (a host read in the reference too)
    acc_ids = input_ids.new_zeros((b, width))
    acc_num = input_ids.new_zeros((b,))
    for z in range(b):
        state = random.getstate()
        words = np.array([random.getrandbits(32) for _ in range(MT_WORDS)], dtype=np.uint32).view(np.int32)
        mt = torch.from_numpy(words).to(input_ids.device)[None]
        if stochastic_noise_fn is not None:
            noise = stochastic_noise_fn(V, p_llm.dtype, p_llm.device)
        else:
            noise = torch.empty((V,), dtype=p_llm.dtype, device=p_llm.device).exponential_(1)
        ids, num, used = tree_verify_stochastic(input_ids[z:z + 1], tree_mask[z:z + 1], p_llm[z:z + 1], p_ssm[z:z + 1],
                                                temperature, mt, noise[None], max(width, 2))
        used = int(used[0])
        random.setstate(state)
        if used < 0:                      # Python's generator stays where it was before the call
            raise RuntimeError("verify_stochastic: the pre-drawn random words were exhausted")
        for _ in range(used):
            random.getrandbits(32)
        acc_ids[z] = ids[0, :width]
        acc_num[z] = num[0]
    return acc_ids, acc_num


def tree_commit(acc_ids, acc_num, output_ids, emitted: int, eos: Optional[int], tree_mask, all_spec, logp_sum,
                target_lens: Optional[torch.Tensor] = None, target_add: int = 0,
                draft_kv_lens: Optional[torch.Tensor] = None, emitted_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """End of a round (``llama_glide.py:1093-1121``) in one launch: the accepted ids go to
    ``output_ids[:, emitted:]``, the tree state is reset for the next round (mask = root column, all_spec[0] =
    the last accepted id, log-prob sums = 0), ``target_lens += target_add``, ``draft_kv_lens += acc_num``.
    Returns state [b,2] int64 = (acc_num, whole-buffer EOS hit) -- the round's one host read.  ``emitted_dev`` [b]
    int32: the write offset lives on the device (read instead of ``emitted``, advanced by acc_num)."""
    _dev(acc_ids, acc_num, output_ids, tree_mask, all_spec, logp_sum, target_lens, draft_kv_lens, emitted_dev)
    b, Fn = _tree_state(tree_mask, all_spec, logp_sum)
    if output_ids.dtype != torch.int64 or output_ids.stride(1) != 1 or not acc_ids.is_contiguous() or acc_ids.dtype != torch.int64:
        raise TypeError("tree_commit: output_ids / acc_ids must be int64 with contiguous rows")
    state = torch.empty((b, 2), dtype=torch.int64, device=all_spec.device)
    lib = _C.load()
    _C.check(lib.ls_tree_commit(acc_ids.data_ptr(), acc_num.data_ptr(), b, acc_ids.shape[1], output_ids.data_ptr(),
                                output_ids.stride(0), output_ids.shape[1], emitted, _len_i32(emitted_dev, b, "emitted_dev"),
                                0 if eos is None else 1,
                                0 if eos is None else int(eos), state.data_ptr(), tree_mask.data_ptr(), all_spec.data_ptr(),
                                logp_sum.data_ptr(), Fn, _len_i32(target_lens, b, "target_lens"), target_add,
                                _len_i32(draft_kv_lens, b, "draft_kv_lens"), _stream()), "ls_tree_commit")
    return state


def tree_commit_stochastic(acc_ids, acc_num, words_used, output_ids, cache_lens, input_len, gamma: int, eos: Optional[int],
                           tree_mask, all_spec, logp_sum, draft_kv_lens, acc_pad) -> torch.Tensor:
    """End of a round at temperature > 0 (``llama_glide.py:1094-1121``) in one launch (``ls_tree_commit_stochastic``): the whole
    zero-padded ``acc_ids`` row goes to ``output_ids`` at column ``cache_lens - input_len``, ``draft_kv_lens += acc_num``, the
    tree state is reset (mask = root column, all_spec[0] = the last accepted id, log-prob sums = 0) and ``acc_pad = acc_ids``.
    Returns state [b,4] int64 = (acc_num, whole-buffer EOS hit, words_used, ``cache_lens + acc_num - input_len + gamma + 2 >
    output_ids.size(1)``) -- the round's one host read.  ``cache_lens`` is read, not advanced (:1094 runs before the walk)."""
    _dev(acc_ids, acc_num, words_used, output_ids, cache_lens, input_len, tree_mask, all_spec, logp_sum, draft_kv_lens, acc_pad)
    b, Fn = _tree_state(tree_mask, all_spec, logp_sum)
    for t, name in ((acc_ids, "acc_ids"), (acc_pad, "acc_pad")):
        if t.dtype != torch.int64 or t.dim() != 2 or t.shape[0] != b or not t.is_contiguous():
            raise TypeError(f"tree_commit_stochastic: {name} must be a contiguous int64 [b, width] tensor")
    if output_ids.dtype != torch.int64 or output_ids.stride(1) != 1 or acc_num.dtype != torch.int64 or not acc_num.is_contiguous():
        raise TypeError("tree_commit_stochastic: output_ids / acc_num must be int64 with contiguous rows")
    if words_used.dtype != torch.int32 or words_used.numel() != b or not words_used.is_contiguous():
        raise TypeError("tree_commit_stochastic: words_used must be a contiguous int32 [b] tensor")
    if acc_pad.shape[1] < acc_ids.shape[1]:
        raise ValueError("tree_commit_stochastic: acc_pad is narrower than acc_ids")
    state = torch.empty((b, 4), dtype=torch.int64, device=all_spec.device)
    _C.check(_C.load().ls_tree_commit_stochastic(
        acc_ids.data_ptr(), acc_num.data_ptr(), words_used.data_ptr(), b, acc_ids.shape[1], output_ids.data_ptr(),
        output_ids.stride(0), output_ids.shape[1], _len_i32(cache_lens, b, "cache_lens"), _len_i32(input_len, b, "input_len"),
        gamma + 2, 0 if eos is None else 1, 0 if eos is None else int(eos), state.data_ptr(), tree_mask.data_ptr(),
        all_spec.data_ptr(), logp_sum.data_ptr(), Fn, _len_i32(draft_kv_lens, b, "draft_kv_lens"), acc_pad.data_ptr(),
        acc_pad.shape[1], _stream()), "ls_tree_commit_stochastic")
    return state


stochastic_uniform_fn = None   # tests replay the reference's CPU generator: fn(shape, device) -> U[0,1) fp32
stochastic_chain_noise_fn = None   # fn(shape, dtype, device) -> Exponential(1) of the model dtype


def chain_accept_stochastic(spec_logits, llm_verify_logits, spec_buffer, llm_verify_output):
    """The temperature > 0 branch of ``spec_generate`` (``llama_glide.py:715-736``): accept drafted token i with probability
    ``min(1, p_i / q_i)`` (q = soft-max of the draft's fp32 logits, p = soft-max of the target's logits in the model dtype,
    neither divided by the temperature -- as the reference), a rejected position takes one draw from p
    (``Categorical(p).sample()`` = ``argmax(p / p.sum / Exponential(1))``).  Rewrites ``llm_verify_output[:, :-1]`` in
    place and returns it with the accept mask [b, gamma] int64 for ``chain_commit``.  A handful of library kernels on
    gamma x V elements: this branch is not on the metric's path."""
    _dev(spec_logits, llm_verify_logits, spec_buffer, llm_verify_output)
    b, g1, V = llm_verify_logits.shape
    gamma = g1 - 1
    q_probs = torch.softmax(spec_logits[:, 1:, :], dim=-1)
    p_probs = torch.softmax(llm_verify_logits[:, :-1, :], dim=-1)
    idx = spec_buffer[:, 1:].unsqueeze(-1)
    alpha = torch.clip((torch.gather(p_probs, -1, idx).squeeze(-1) + 1e-9) / (torch.gather(q_probs, -1, idx).squeeze(-1) + 1e-9), 0.0, 1.0)
    u = stochastic_uniform_fn(alpha.shape, alpha.device) if stochastic_uniform_fn is not None else torch.rand_like(alpha)
    accept = u.lt(alpha)
    p2 = p_probs.reshape(-1, V)
    pn = p2 / p2.sum(-1, keepdim=True)
    nz = (stochastic_chain_noise_fn(pn.shape, pn.dtype, pn.device) if stochastic_chain_noise_fn is not None
          else torch.empty_like(pn).exponential_(1))
    resample = (pn / nz).argmax(dim=-1).reshape(b, gamma)
    llm_verify_output[:, :-1] = torch.where(accept, spec_buffer[:, 1:], resample)
    return llm_verify_output, accept.to(torch.int64).contiguous()


def chain_commit(llm_verify_output, spec_buffer, output_ids, cache_lens, draft_cache_lens, input_len, next_spec_start_token,
                 eos: Optional[int], accept_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """End of a chain-speculation round (``llama_glide.py:738-770``) in one launch: acceptance by cumulative match (or, at
    temperature > 0, by the cumulative product of ``accept_mask``, ``:732``), the verified ids + bonus token into
    ``output_ids``, the length bookkeeping and the next round's start tokens, in place.
    Returns state [b,2] int64 = (correct_len, EOS hit) -- the round's one host read."""
    _dev(llm_verify_output, spec_buffer, output_ids, cache_lens, draft_cache_lens, input_len, next_spec_start_token)
    b, g1 = llm_verify_output.shape
    for t, name in ((llm_verify_output, "llm_verify_output"), (spec_buffer, "spec_buffer"), (next_spec_start_token, "next_spec_start_token")):
        if t.dtype != torch.int64 or not t.is_contiguous():
            raise TypeError(f"chain_commit: {name} must be a contiguous int64 tensor")
    if tuple(spec_buffer.shape) != (b, g1) or tuple(next_spec_start_token.shape) != (b, 2):
        raise ValueError("chain_commit: spec_buffer [b, gamma+1], next_spec_start_token [b, 2]")
    if output_ids.dtype != torch.int64 or output_ids.stride(1) != 1:
        raise TypeError("chain_commit: output_ids must be int64 with contiguous rows")
    if accept_mask is not None and (accept_mask.dtype != torch.int64 or not accept_mask.is_contiguous() or tuple(accept_mask.shape) != (b, g1 - 1)):
        raise TypeError("chain_commit: accept_mask must be a contiguous int64 [b, gamma] tensor")
    state = torch.empty((b, 2), dtype=torch.int64, device=output_ids.device)
    lib = _C.load()
    _C.check(lib.ls_chain_commit(llm_verify_output.data_ptr(), spec_buffer.data_ptr(), b, g1 - 1, output_ids.data_ptr(),
                                 output_ids.stride(0), output_ids.shape[1], _len_i32(cache_lens, b, "cache_lens"),
                                 _len_i32(draft_cache_lens, b, "draft_cache_lens"), _len_i32(input_len, b, "input_len"),
                                 next_spec_start_token.data_ptr(), 0 if eos is None else 1, 0 if eos is None else int(eos),
                                 state.data_ptr(), accept_mask.data_ptr() if accept_mask is not None else None, _stream()),
             "ls_chain_commit")
    return state


EMBED_MAX_ROWS = 128
# one launch for embedding gather + RoPE table + first input norm of a decode pass (ls_pass_head); LONGSPEC_PASS_HEAD=0 keeps the
# three operators (A/B measurements; the results are bit-identical either way)
PASS_HEAD = os.environ.get("LONGSPEC_PASS_HEAD", "1") != "0"


def embed_supported(ids: torch.Tensor, weight: torch.Tensor) -> bool:
    """Short passes gather their embedding rows with ``ls_embed_rows``; prefill-sized inputs use the library."""
    return (ids.is_cuda and weight.is_cuda and 0 < ids.numel() <= EMBED_MAX_ROWS and weight.dtype in (torch.float16, torch.bfloat16)
            and weight.is_contiguous() and weight.shape[1] % 8 == 0)


def pass_head(weight: torch.Tensor, ids: torch.Tensor, inv_freq: torch.Tensor, attention_scaling: float, norm_weight: torch.Tensor,
              eps: float, position_ids: Optional[torch.Tensor] = None, pos_base: Optional[torch.Tensor] = None, pos_add: int = 0):
    """Head of a decode pass in one launch: ``embed_tokens(ids)``, the pass's RoPE table and the first layer's
    ``input_layernorm`` (``llama.py:579-580`` + ``LlamaDecoderLayer.forward``; ``llama_glide.py:1003-1006,1030-1033,437``).
    ids [b,q] int64; positions = ``position_ids`` [b,q] int64, or ``arange(q) + pos_base[:, None] + pos_add`` (pos_base [b] int32).
    Returns (embeds [b,q,hidden], normed [b,q,hidden], (cos, sin) [b,q,128]); bit-identical to the three separate operators."""
    _dev(weight, ids, inv_freq, norm_weight, position_ids, pos_base)
    b, q = ids.shape
    flat = ids.to(torch.int64).contiguous().view(-1)
    hidden = weight.shape[1]
    dev = weight.device
    buf = torch.empty((2, b, q, hidden), dtype=weight.dtype, device=dev)
    cs = torch.empty((2, b, q, 128), dtype=weight.dtype, device=dev)
    if position_ids is not None:
        pos = position_ids.to(torch.int64).contiguous()
        if pos.numel() != b * q:
            raise ValueError(f"pass_head: {pos.numel()} positions for {b * q} token rows")
        pos_p, base_p = pos.data_ptr(), None
    else:
        if pos_base is None or pos_base.numel() != b:
            raise ValueError("pass_head: position_ids [b,q] int64 or pos_base [b] int32")
        pos_base = pos_base if pos_base.dtype == torch.int32 else pos_base.to(torch.int32)
        pos_base = pos_base.contiguous()
        pos_p, base_p = None, pos_base.data_ptr()
    lib = _C.load()
    _C.check(lib.ls_pass_head(weight.data_ptr(), weight.shape[0], hidden, _dtype(weight), flat.data_ptr(), b * q, pos_p, base_p, q,
                              int(pos_add), inv_freq.data_ptr(), float(attention_scaling), norm_weight.data_ptr(), float(eps),
                              buf[0].data_ptr(), buf[1].data_ptr(), cs[0].data_ptr(), cs[1].data_ptr(), _stream()), "ls_pass_head")
    return buf[0], buf[1], (cs[0], cs[1])


def pass_head_supported(ids: torch.Tensor, weight: torch.Tensor, norm_weight: torch.Tensor) -> bool:
    return (embed_supported(ids, weight) and ids.dim() == 2 and ids.numel() <= 128 and weight.shape[1] // 8 <= 4096
            and norm_weight.dtype == weight.dtype and norm_weight.is_cuda)


def embed_rows(weight: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """``embed_tokens(ids)`` (``llama.py:579``): out[..., :] = weight[ids]."""
    _dev(weight, ids)
    flat = ids.to(torch.int64).contiguous().view(-1)
    out = torch.empty((flat.numel(), weight.shape[1]), dtype=weight.dtype, device=weight.device)
    lib = _C.load()
    _C.check(lib.ls_embed_rows(weight.data_ptr(), weight.shape[0], weight.shape[1], _dtype(weight), flat.data_ptr(), flat.numel(),
                               out.data_ptr(), _stream()), "ls_embed_rows")
    return out.view(*ids.shape, weight.shape[1])
