"""Draft ("glide") layer and the speculative-decoding loops -- host-side mirror of
``longspec/test/llama_glide.py``: same classes, method names, argument meaning and
return tuples, same draft-checkpoint tensor names (20 tensors, q/k/v with
bias), driven by the HIP operator layer.

Differences from the reference that are deliberate and invisible to callers:
* every attention / norm / rotary / tree-collapse operator is a hand-written HIP kernel
  (``longspec_amd.ops``); there is no flash-attn, Triton or torch.compile dependency;
* the round loop reads ONE scalar per round from the device (``acc_num``) instead of the
  reference's several implicit synchronisations (``llama_glide.py:1069-1089,1118-1121,1149``);
* the host keeps an upper bound of every cache length so kernels can size their grids
  without reading device memory.
"""
from __future__ import annotations

import time
from functools import partial
from types import SimpleNamespace
from typing import List, Optional

import torch
from torch import nn

from .graphs import GraphReplayer
from .target_rules import TargetRules
from .lookup import check as _lookup_check
from .llama import (DecodeLinear, LlamaForCausalLM, LlamaMLP, LlamaRMSNorm, chunked_causal_prefill,
                    project_qkv, _default_ops)


class GlideAttention(nn.Module):
    """``GlideAttention`` (``llama_glide.py:23-385``): draft self-attention with a sliding
    window of 512 over its own KV cache, and cross-attention over the target's last-layer KV."""

    WINDOW = 512
    CACHE_PAD = 128      # extra draft-cache rows at prefill (llama_glide.py:218-219); 0 in the Qwen2 twin (qwen2_glide.py:217-218)

    def __init__(self, config, layer_idx: Optional[int] = None, ops=None):
        super().__init__()
        self.config = config
        self.layer_idx = layer_idx
        self.hidden_size = config.hidden_size
        self.num_heads = config.num_attention_heads
        self.head_dim = self.hidden_size // self.num_heads
        self.num_key_value_heads = config.num_key_value_heads
        self.num_key_value_groups = self.num_heads // self.num_key_value_heads
        self.q_proj = DecodeLinear(self.hidden_size, self.num_heads * self.head_dim, bias=True, ops=ops)     # bias=True even for Llama (:49-52)
        self.k_proj = DecodeLinear(self.hidden_size, self.num_key_value_heads * self.head_dim, bias=True, ops=ops)
        self.v_proj = DecodeLinear(self.hidden_size, self.num_key_value_heads * self.head_dim, bias=True, ops=ops)
        self.o_proj = DecodeLinear(self.num_heads * self.head_dim, self.hidden_size, bias=False, ops=ops)
        self.K_Cache = None
        self.V_Cache = None
        self.max_len = 512
        self.softmax_scale = 1 / (self.head_dim ** 0.5)
        self.ops = ops
        self.kv_len_hint = None          # bound of the draft cache length
        self.llm_kv_len_hint = None      # bound of the target last-layer KV length
        self.shard = None                # dist.KVShard: the target KV this layer cross-attends is sequence-sharded

    def forward(self, hidden_states, position_embeddings, cache_lens=None, flex_attn=None, exec_type="training",
                k_cache=None, v_cache=None, llm_kv_len=None, tree_mask=None, tree_mask_bits=None):
        if exec_type in ["prefill", "sa_prefill"]:
            y = self.prefill(hidden_states, position_embeddings)
        elif exec_type == "sa_decoding":
            y = self.decoding(hidden_states, position_embeddings, cache_lens, K_Cache=None, V_Cache=None)
        elif exec_type in ["decoding", "ca_decoding", "ca_prefill"]:
            y = self.decoding(hidden_states, position_embeddings, cache_lens, k_cache, v_cache, llm_kv_len)
        elif exec_type in ["sa_tree_decoding"]:
            y = self.tree_decoding(hidden_states, position_embeddings, cache_lens, None, None, llm_kv_len, tree_mask, tree_mask_bits)
        elif exec_type in ["ca_tree_decoding"]:
            y = self.tree_decoding(hidden_states, position_embeddings, cache_lens, k_cache, v_cache, llm_kv_len, tree_mask, tree_mask_bits)
        else:
            raise ValueError(f"Unknown inference_type: {exec_type}")
        return y

    def _qkv(self, hidden_states, position_embeddings, need_kv=True):
        if need_kv:
            return project_qkv(self.ops, hidden_states, self.q_proj, self.k_proj, self.v_proj, position_embeddings,
                               self.num_heads, self.num_key_value_heads, self.head_dim)
        # cross-attention: the reference projects k/v it never uses (:248-249 vs :265); skip them
        q, _, _ = project_qkv(self.ops, hidden_states, self.q_proj, None, None, position_embeddings,
                              self.num_heads, self.num_key_value_heads, self.head_dim)
        return q, None, None

    def _cross(self, q, K_Cache, V_Cache, llm_kv_len, causal: bool):
        """Cross-attention over the target's last-layer KV (K7), whole or sequence-sharded."""
        if self.shard is None:
            return self.ops.kvcache_attention(q, K_Cache, V_Cache, causal=causal, cache_seqlens=llm_kv_len.int(),
                                              kv_len_hint=self.llm_kv_len_hint)
        sh = self.shard
        # bottom-right causal alignment only matters on the rank that owns the tail of the sequence
        call = self.ops.sharded_prefix_attention(q, K_Cache, V_Cache, sh.pass_len(llm_kv_len),
                                                 causal=causal and sh.is_tail, kv_len_hint=sh.local_hint(self.llm_kv_len_hint))
        return sh.attend(call)

    def prefill(self, hidden_states, position_embeddings):                      # :206-233
        bsz, q_len, _ = hidden_states.size()
        q, k, v = self._qkv(hidden_states, position_embeddings)
        self.K_Cache = q.new_zeros((bsz, q_len + self.max_len + self.CACHE_PAD, self.num_key_value_heads, self.head_dim))
        self.V_Cache = q.new_zeros((bsz, q_len + self.max_len + self.CACHE_PAD, self.num_key_value_heads, self.head_dim))
        attn = chunked_causal_prefill(self.ops, q, k, v, self.K_Cache, self.V_Cache, window_left=self.WINDOW)
        return self.o_proj(attn.reshape(bsz, q_len, self.hidden_size))

    def prefill_cache_only(self, hidden_states, position_embeddings):
        """What the draft's prefill leaves behind: the K/V rows of the prompt.  The layer's outputs are discarded by
        every caller (:968-975), and these rows are a row-wise function of the token ids -- so the sequence-sharded path,
        where no rank holds the whole target KV the cross-attention would read, fills the cache with just this."""
        bsz, q_len, _ = hidden_states.size()
        _, k, v = self._qkv(hidden_states, position_embeddings)
        shape = (bsz, q_len + self.max_len + self.CACHE_PAD, self.num_key_value_heads, self.head_dim)
        self.K_Cache, self.V_Cache = k.new_zeros(shape), v.new_zeros(shape)
        self.K_Cache[:, :q_len], self.V_Cache[:, :q_len] = k, v

    def decoding(self, hidden_states, position_embeddings, cache_lens, K_Cache, V_Cache, llm_kv_len=None):   # :235-270
        bsz, q_len, _ = hidden_states.size()
        if K_Cache is None:
            q, k, v = self._qkv(hidden_states, position_embeddings)
            attn = self.ops.kvcache_attention(q, self.K_Cache, self.V_Cache, k, v, window_size=(self.WINDOW, -1), causal=True,
                                              cache_seqlens=cache_lens.int(), kv_len_hint=self.kv_len_hint)
        else:
            q, _, _ = self._qkv(hidden_states, position_embeddings, need_kv=False)
            attn = self._cross(q, K_Cache, V_Cache, llm_kv_len, causal=True)
        return self.o_proj(attn.view(bsz, q_len, self.hidden_size))

    def tree_decoding(self, hidden_states, position_embeddings, cache_lens, K_Cache, V_Cache, llm_kv_len=None,
                      tree_mask=None, tree_mask_bits=None):                     # :272-329
        bsz, q_len, _ = hidden_states.size()
        if K_Cache is not None:
            q, _, _ = self._qkv(hidden_states, position_embeddings, need_kv=False)
            attn = self._cross(q, K_Cache, V_Cache, llm_kv_len, causal=False)
        else:
            q, k, v = self._qkv(hidden_states, position_embeddings)
            if tree_mask_bits is None:
                tree_mask_bits = self.ops.pack_tree_mask(tree_mask)
            attn = self.ops.draft_tree_attention(q, k, v, self.K_Cache, self.V_Cache, cache_lens, tree_mask_bits,
                                                 tree_mask.size(-1), window=self.WINDOW, kv_len_hint=self.kv_len_hint)
        return self.o_proj(attn.view(bsz, q_len, self.hidden_size).to(hidden_states.dtype))


class LlamaGlideDecoderLayer(nn.Module):
    """``LlamaGlideDecoderLayer`` (``llama_glide.py:388-468``): norm -> self-attn -> +res ->
    norm -> cross-attn -> +res -> norm -> MLP -> +res; no final norm."""

    ATTENTION_CLS = GlideAttention

    def __init__(self, config, ops=None):
        super().__init__()
        self.config = config
        self.ops = ops if ops is not None else _default_ops()
        self.hidden_size = config.hidden_size
        self.layer_idx = 0
        self.self_attn = self.ATTENTION_CLS(config, self.layer_idx, ops=self.ops)
        self.cross_attn = self.ATTENTION_CLS(config, self.layer_idx, ops=self.ops)
        self.mlp = LlamaMLP(config, ops=self.ops)
        self.input_layernorm = LlamaRMSNorm(config.hidden_size, eps=config.rms_norm_eps, ops=self.ops)
        self.post_self_attention_layernorm = LlamaRMSNorm(config.hidden_size, eps=config.rms_norm_eps, ops=self.ops)
        self.post_cross_attention_layernorm = LlamaRMSNorm(config.hidden_size, eps=config.rms_norm_eps, ops=self.ops)

    def set_max_gen_len(self, max_gen_len):
        self.self_attn.max_len = max_gen_len

    def prefill_cache_only(self, hidden_states, position_embeddings):
        self.self_attn.prefill_cache_only(self.input_layernorm(hidden_states), position_embeddings)

    def forward(self, hidden_states, position_embeddings, llm_kv, cache_lens=None, exec_type=None, llm_kv_len=None,
                tree_mask=None, tree_mask_bits=None, prenormed=None):
        """``tree_mask_bits``: the packed ``tree_mask`` when the caller already has it (``ops.tree_grow``);
        ``prenormed``: ``input_layernorm(hidden_states)`` when the pass's head launch (``ops.pass_head``) already formed it."""
        bits = tree_mask_bits
        if bits is None and tree_mask is not None:
            bits = self.ops.pack_tree_mask(tree_mask)
        if self.cross_attn.shard is not None:
            self.cross_attn.shard.begin_pass()
        residual = hidden_states
        hidden_states = self.input_layernorm(hidden_states) if prenormed is None else prenormed
        hidden_states = self.self_attn(hidden_states=hidden_states, position_embeddings=position_embeddings,
                                       cache_lens=cache_lens, exec_type="sa_" + exec_type, tree_mask=tree_mask,
                                       tree_mask_bits=bits)
        hidden_states, residual = self.post_self_attention_layernorm(hidden_states, residual=residual)   # + residual, norm
        hidden_states = self.cross_attn(hidden_states=hidden_states, position_embeddings=position_embeddings,
                                        cache_lens=cache_lens, exec_type="ca_" + exec_type, k_cache=llm_kv[0],
                                        v_cache=llm_kv[1], llm_kv_len=llm_kv_len, tree_mask=tree_mask, tree_mask_bits=bits)
        hidden_states, residual = self.post_cross_attention_layernorm(hidden_states, residual=residual)  # + residual, norm
        return self.mlp(hidden_states, residual=residual)           # `hidden_states = residual + mlp(...)` (:466)


class _DecodeState(SimpleNamespace):
    """State of a decode loop.  ``use_graphs`` is the caller's switch, honoured at every call; what the loop's
    ``GraphReplayer`` (``replayer``) has done is read off it."""
    graphs = property(lambda self: False if self.replayer.disabled else self.replayer.entries)   # `is not False`: replay still on
    graph_tiers = property(lambda self: self.replayer.tiers)
    graph_captures = property(lambda self: self.replayer.captures)


DRAFT_HEAD_ENV = "LONGSPEC_DRAFT_HEAD"         # "fp8" / "fp4": quantize_draft_head_ at the first draft pass; unset: the shared lm_head
_ENV_DRAFT_HEAD = {"fp8": "fp8", "fp4": "mxfp4"}


def _env_draft_head():
    import os
    mode = os.environ.get(DRAFT_HEAD_ENV, "")
    if mode and mode not in _ENV_DRAFT_HEAD:
        raise ValueError(f"{DRAFT_HEAD_ENV}={mode!r}: expected one of {sorted(_ENV_DRAFT_HEAD)}")
    return _ENV_DRAFT_HEAD.get(mode)


def _sync(t: torch.Tensor):
    if t.is_cuda:
        torch.cuda.synchronize(t.device)


def _chain_round_host(st, state) -> bool:
    """The host half of a chain-shaped round (``chain_round``, ``lookup_round``): the round's ONE host read, state [bsz, 2] =
    (correct_len, EOS hit | 2 * stop hit), onto the host mirrors.  False = stop: the buffer cannot take another round, or a
    hit (a ``stop=`` match leaves the counters as they are)."""
    state = state.tolist()
    n_ok, hit = state[0][0], any(row[1] for row in state)
    st.stopped = any(row[1] & 2 for row in state)                     # ops.stop_scan raised bit 1
    st.count += n_ok - 1
    st.num += st.bsz
    st.emitted += n_ok
    if st.emitted - 1 + st.gamma + 2 > st.output_ids.size(1):
        return False
    return not hit


def _tree_round_host(st, state) -> bool:
    """The host half of a tree-shaped round (``tree_round``, ``_lookup_tree_round``): the round's ONE host read, state [bsz, 2]
    = (acc_num, EOS hit | 2 * stop hit), onto the host mirrors; False as above (:1118, :1120)."""
    state = state.tolist()
    a, hit = state[0][0], any(row[1] for row in state)
    st.stopped = any(row[1] & 2 for row in state)
    st.acc_ids = st.acc_pad[:, :a]
    st.a = a
    st.emitted += a
    st.count += a - 1
    st.num += st.bsz
    if st.emitted + st.gamma + 2 > st.output_ids.size(1):
        return False
    return not hit


class LlamaGlide(LlamaForCausalLM):
    """``LlamaGlide`` (``llama_glide.py:471-1245``).  ``LlamaGlide(config, target_model_path,
    glide_path=None)`` -- the reference's signature -- loads the target and the draft checkpoint (local
    directories or hub ids, safetensors / .bin, sharded or not) in fp16 onto the current GPU, as the
    reference's ``from_pretrained(..., torch_dtype=torch.float16, device_map="auto")`` does (``:474,480``);
    ``config`` may be a ``transformers`` config object or any attribute namespace.
    ``target_model_path=None`` builds random-init modules (tests, synthetic benchmarks).  ``device`` /
    ``dtype`` / ``ops`` are extensions: with the default HIP operator layer the model lives on
    ``torch.cuda.current_device()``; an injected ``ops`` (the CPU oracle of the host-logic tests) keeps
    it where it is."""

    GLIDE_LAYER_CLS = LlamaGlideDecoderLayer

    def __init__(self, config, target_model_path=None, glide_path=None, ops=None, dtype=torch.float16, device=None):
        super().__init__(config, ops=ops)
        self.glide = self.GLIDE_LAYER_CLS(config, ops=self.ops)
        for m in self.glide.modules():
            if isinstance(m, DecodeLinear):
                m.quant_scope = "draft"        # quantize_weights_("draft") / LONGSPEC_WEIGHT_QUANT=fp8-draft, fp4-draft
        self.draft_lm_head = None              # quantize_draft_head_ / LONGSPEC_DRAFT_HEAD: the draft passes' own lm_head
        self._draft_head_env = _env_draft_head()
        self._draft_head_env_key = None
        if target_model_path is not None or glide_path is not None:
            from .checkpoint import load_draft_checkpoint, load_target_checkpoint
            if target_model_path is not None:
                load_target_checkpoint(self, target_model_path)
            if glide_path is not None:
                load_draft_checkpoint(self.glide, glide_path)
        self.to(dtype)
        if device is None and ops is None and torch.cuda.is_available():
            device = torch.device("cuda", torch.cuda.current_device())
        if device is not None:
            self.to(device)
        for p in self.parameters():
            p.requires_grad = False
        self.eval()

    GRAPH_ROUNDS = True      # capture tree rounds into HIP graphs (one per accepted-token count), see tree_round
    GRAPH_AFTER = 256        # ... once a generation has run this many rounds: a capture costs ~10 ms and a replay saves
                             # <= 0.1 ms on a fast host (more on a slow or busy one), so only long generations
                             # (LongSpec's long-CoT case) pay it back; benchmarks capture up front (prepare_tree_graphs)
    GRAPH_STOCHASTIC = True  # ... the rounds at temperature > 0 too (tree_round_stochastic); False: launch by launch
    GRAPH_TIER = 4096        # a captured round / step is sized (host-side bounds of the KV lengths -> launch grids, split
                             # counts, kernel choice) for the tokens emitted so far rounded up to the next multiple of this;
                             # a generation that outgrows its tier drops its graphs and captures the next tier's (a 20 000-token
                             # long-CoT generation: five tiers, ~12 captures of ~10 ms).  Sizing every graph for the whole
                             # budget instead made a 1k-token prompt with a 20k budget run 21k-row launch shapes from round 1.

    # ------------------------------------------------------------------------------------------
    def __setattr__(self, name, value):
        # the draft head is NOT a registered sub-module: parameters(), state_dict() and .to() do not see it
        if name == "draft_lm_head":
            if value is not None and not isinstance(value, DecodeLinear):
                raise TypeError("draft_lm_head is a DecodeLinear or None")
            object.__setattr__(self, name, value)
        else:
            super().__setattr__(name, value)

    def _apply(self, fn, *args, **kwargs):
        # .to() / .half() / .cuda(): the unregistered draft head follows the model (its pack is rebuilt, and the weight rounded
        # again -- to the same values -- at its next use: DecodeLinear keys both on the weight's device, dtype and version)
        out = super()._apply(fn, *args, **kwargs)
        head = getattr(self, "draft_lm_head", None)
        if head is not None:
            head._apply(fn, *args, **kwargs)
        return out

    @torch.no_grad()
    def quantize_draft_head_(self, fmt: str = "fp8"):
        """A low-precision copy of the lm_head for the DRAFT passes only (no counterpart in the reference): ``draft_lm_head``
        becomes a ``DecodeLinear`` that holds ``lm_head.weight`` as it is now, rounded to ``fmt`` (``"fp8"`` or ``"mxfp4"``,
        ``DecodeLinear.quantize_weight_``), and streams the 8-bit / 4-bit pack.  ``lm_head`` itself is not touched and the
        copy is not a registered module (``state_dict()`` keeps its keys).

        Used by the lm_head calls of the glide draft passes: the tree rounds' step-0 and level calls and the chain drafter's
        calls.  It changes what the draft proposes, and with it the acceptance length, never what the target accepts:
        prefill's first token, every verify pass, ``vanilla_generate`` and MagicDec's self-draft keep multiplying
        ``lm_head``, and so does the vocabulary-sharded ``head_select`` path (16-bit, draft passes included).
        ``model.draft_lm_head = None`` restores the shared head.  ``model.to(...)`` / ``.half()`` / ``.cuda()`` move the copy
        with the model (``_apply``), although ``parameters()`` and ``state_dict()`` do not list it."""
        src = self.lm_head
        # (the generate loops run under inference_mode: the copy must be an ordinary tensor, whose version DecodeLinear tracks)
        with torch.inference_mode(False), torch.no_grad():
            if src._quant_due():
                src.quantize_weight_()
            with torch.device("meta"):         # (no [vocab, hidden] fp32 initialisation on the host: the parameters follow)
                head = DecodeLinear(src.in_features, src.out_features, bias=src.bias is not None, ops=self.ops)
            head.weight = torch.nn.Parameter(src.weight.detach().clone(), requires_grad=False)
            if src.bias is not None:
                head.bias = torch.nn.Parameter(src.bias.detach().clone(), requires_grad=False)
            head._env_scopes = ()              # the copy's format is this call's, not the process-wide default's
            head.quantize_weight_(fmt)
            if head.weight.is_cuda and (head._q8 is not None or head._q4 is not None):
                head.packed()                  # before the first warm-up round: a captured graph only replays launches
        self.draft_lm_head = head
        return self

    def _head_of_draft_passes(self):
        """The lm_head of the glide draft passes: ``draft_lm_head`` when set (``quantize_draft_head_``, or built here at the
        first use under LONGSPEC_DRAFT_HEAD -- a benchmark may fill the weights in place after constructing the model --
        and again when ``lm_head.weight`` has changed since), else ``lm_head``."""
        if self._draft_head_env and self._draft_head_env_key != self.lm_head._key():
            if self.draft_lm_head is None or self._draft_head_env_key is not None:     # (never over a head the caller set)
                self.quantize_draft_head_(self._draft_head_env)
                self._draft_head_env_key = self.lm_head._key()
        return self.draft_lm_head if self.draft_lm_head is not None else self.lm_head

    def set_max_gen_len(self, max_gen_len):
        super().set_max_gen_len(max_gen_len)

    def _set_hints(self, target_bound: Optional[int], draft_bound: Optional[int]):
        """Host-side upper bounds of the KV lengths the next kernels will see."""
        self.model.set_kv_len_hint(target_bound)
        self.glide.self_attn.kv_len_hint = draft_bound
        self.glide.cross_attn.llm_kv_len_hint = target_bound

    def _draft_head(self, ids, position_ids=None, pos_base=None, pos_add: int = 0):
        """Head of a draft pass: ``embed_tokens(ids)``, the RoPE table of its positions (``position_ids`` [b,q] int64, or
        ``arange(q) + pos_base[:, None] + pos_add``) and the draft layer's ``input_layernorm`` (``llama_glide.py:1003-1006,
        1030-1033,437``).  One launch on the HIP operator layer (``ops.pass_head``), three operators otherwise (the CPU oracle
        of the host-logic tests); returns (embeds, normed or None, position_embeddings)."""
        ops, ln, rot = self.ops, self.glide.input_layernorm, self.model.rotary_emb
        if (getattr(ops, "pass_head", None) is not None and getattr(ops, "PASS_HEAD", True)
                and ops.pass_head_supported(ids, self.model.embed_tokens.weight, ln.weight)):
            if rot.inv_freq.device != ids.device:
                rot.inv_freq = rot.inv_freq.to(ids.device)
            return ops.pass_head(self.model.embed_tokens.weight, ids, rot.inv_freq, rot.attention_scaling, ln.weight,
                                 ln.variance_epsilon, position_ids=position_ids, pos_base=pos_base, pos_add=pos_add)
        hidden_states = self.model.embed_tokens(ids)
        if position_ids is None:
            position_ids = torch.arange(ids.size(1), device=ids.device)[None, :] + pos_base[:, None] + pos_add
        return hidden_states, None, self.model.rotary_emb(hidden_states, position_ids)

    def _rules(self, device, temperature, shard, head_sharded=False, **keywords):
        """The ``TargetRules`` (``target_rules.py``) of a loop on this model from its request ``keywords``: resolved,
        refused or built -- tables included -- before any forward."""
        return TargetRules(self.ops, self.lm_head.out_features, device, temperature, shard, head_sharded, **keywords)

    def _stop_id(self, eos_id, loop: str):
        """Token whose appearance ends a loop.  The Llama twin tests ``self.config.eos_token_id`` in all
        three loops (llama_glide.py:578,767,1120) and ignores the ``eos_id`` argument for that."""
        return getattr(self.config, "eos_token_id", None)

    def _tree_output_fill(self, eos_id):
        """Initial content of ``output_ids`` in tree_spec_generate (llama_glide.py:937: eos_id, G8)."""
        return eos_id

    def _last_kv(self):
        attn = self.model.layers[-1].self_attn
        return attn.K_Cache, attn.V_Cache

    # ------------------------------------------------------------------------------------------
    def _clear_shard(self):
        """A shard set by an earlier ``tree_spec_generate(shard=...)`` on this object must not leak into loops that
        prefill a full, unsharded cache."""
        for layer in self.model.layers:
            layer.self_attn.shard = None
        self.glide.cross_attn.shard = None

    def _prefill_target(self, input_ids, prompt_length, exec_type="prefill"):
        """The target's prefill of every front door (:954-960): returns (the logits of each row's last prompt token, int32
        ``cache_lens`` [bsz] = ``prompt_length``, a tensor of the caller's own)."""
        bsz, P = input_ids.size(0), int(input_ids.size(1))
        self._set_hints(P, P)
        hidden_states = self.model.forward(input_ids, exec_type=exec_type).last_hidden_state
        rows = torch.arange(bsz, device=input_ids.device)
        logits = self.lm_head(hidden_states[rows, prompt_length - 1, :])
        return logits, input_ids.new_zeros((bsz)).int() + prompt_length.to(input_ids.device).int()

    def _prefill_draft(self, input_ids, lens):
        """The glide prefill (:968-975) over the target's last-layer KV of ``lens`` [bsz] int32 rows; ``lens=None``: the
        draft cache's prompt rows alone (``_sharded_prefill``)."""
        hidden_states = self.model.embed_tokens(input_ids)
        position_ids = torch.arange(0, input_ids.size(1), device=input_ids.device)[None, :]
        position_embeddings = self.model.rotary_emb(hidden_states, position_ids)
        if lens is None:
            return self.glide.prefill_cache_only(hidden_states, position_embeddings)
        self.glide(hidden_states=hidden_states, position_embeddings=position_embeddings, llm_kv=self._last_kv(),
                   cache_lens=lens.clone(), llm_kv_len=lens.clone(), exec_type="prefill")

    @torch.inference_mode()
    def vanilla_generate(self, input_ids, prompt_length, max_gen_len=64, eos_id=151645, sampling=None,
                         penalties=None, logprobs=None, stop=None, ban=None, guide=None, dry=None, watermark=None, cut=None):                                      # :552-585
        """``sampling`` / ``penalties`` / ``logprobs`` / ``stop`` / ``ban`` / ``guide``: the rules on the target's logits
        (``target_rules.py``), on every step's one row; with ``sampling`` this loop is the denominator of a sampled speculative
        run, and with the same seed the same text.  The log-probs are published as ``self.last_logprobs``, the stop result as
        ``self.last_stop`` (None without the keyword); the return tuple is unchanged.  Under ``stop`` the loop ends when every
        row has stopped (tested where the EOS test is, every 16th step) and the elapsed time is cut back to the step of the
        last row's stop; the built-in EOS test runs alongside, unchanged."""
        assert input_ids is not None, "please give the input"
        rules = self._rules(input_ids.device, None, None, sampling=sampling, penalties=penalties, logprobs=logprobs, stop=stop,
                            ban=ban, guide=guide, dry=dry, watermark=watermark, cut=cut)
        self._clear_shard()
        bsz, P = input_ids.size(0), int(input_ids.size(1))
        output_ids = input_ids.new_zeros((bsz, max_gen_len))
        self.set_max_gen_len(max_gen_len)
        input_len = prompt_length
        logits, cache_lens = self._prefill_target(input_ids, input_len)
        output_ids[:, 0] = rules.first_token(logits, input_len, input_ids)
        num = 0
        eos = self._stop_id(eos_id, "vanilla")
        _sync(input_ids)
        start_time = time.time()
        on_gpu = input_ids.is_cuda
        marks = []                      # per-step completion marks: the time of steps decoded past the first EOS is not counted
        if on_gpu:
            ev0 = torch.cuda.Event(enable_timing=True)
            ev0.record()
        vs = self.begin_vanilla_decode(output_ids, cache_lens, input_len.int(), P, prompt_ids=input_ids, rules=rules)
        self.last_logprobs = vs.logprobs
        self.last_stop = vs.last_stop
        for step in range(1, max_gen_len):
            self.vanilla_step(vs)
            num += bsz
            if on_gpu:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
                marks.append(ev)
            else:
                marks.append(time.time() - start_time)
            # the reference reads the EOS test back after every token (:578); here every 16th, and the result is then cut
            # back to what the reference would have returned -- tokens, `num` AND elapsed time
            if vs.stop is not None and (step % 16 == 0 or step == max_gen_len - 1):
                # the same poll, still ONE host read: (EOS anywhere, every row has stopped)
                hit = output_ids[:, :step + 1].eq(eos).any() if eos is not None else vs.stop_state.new_zeros((), dtype=torch.bool)
                if any(torch.stack([hit, vs.stop_state[:, 0].ge(0).all()]).tolist()):
                    break
            elif eos is not None and (step % 16 == 0 or step == max_gen_len - 1):
                if bool((output_ids[:, :step + 1].eq(eos)).any()):
                    break
        _sync(input_ids)
        elapsed_time = time.time() - start_time
        if eos is not None:
            output_ids, num, stop = _truncate_after_eos_vanilla(output_ids, num, eos, bsz)
            if stop is not None and vs.logprobs is not None:          # the cut of output_ids, on its columns
                lp = vs.logprobs
                lp.token[:, stop + 1:], lp.top_ids[:, stop + 1:], lp.top[:, stop + 1:] = float("nan"), -1, float("-inf")
            if stop is not None and stop < len(marks):
                elapsed_time = ev0.elapsed_time(marks[stop - 1]) * 1e-3 if on_gpu else marks[stop - 1]
                marks = marks[:stop]
        if vs.stop is not None:
            lengths = vs.stop_state[:, 0].tolist()
            if min(lengths) >= 0:                                     # every row stopped: step s wrote column s
                last = max(max(lengths) - 1, 1)
                if last < len(marks):
                    elapsed_time = ev0.elapsed_time(marks[last - 1]) * 1e-3 if on_gpu else marks[last - 1]
        return output_ids, num, elapsed_time

    # ------------------------------------------------------------------------------------------
    def begin_vanilla_decode(self, output_ids, cache_lens, input_len, prompt_bound: int, sampling=None, penalties=None,
                             prompt_ids=None, logprobs=None, stop=None, ban=None, guide=None, dry=None, watermark=None, cut=None, rules=None):
        """State of the vanilla loop (``llama_glide.py:566-583``): ``output_ids`` [bsz, max_gen] with the first
        token in place, ``cache_lens`` [bsz] int32 valid rows of every cache, ``input_len`` [bsz] int32.  The nine keywords:
        ``target_rules.py`` (``rules``: the ``TargetRules`` the caller has built from them already, for the first token);
        ``prompt_ids[z, :input_len[z]]`` is the prompt the penalty state starts from (None: no prompt flags).  Every step rules
        its one row, which predicts column ``cache_lens - input_len + 1``.  A row that has stopped keeps decoding with the
        batch, and every step erases what it wrote."""
        dev = output_ids.device
        if rules is None:
            rules = self._rules(dev, None, self.model.layers[-1].self_attn.shard, sampling=sampling, penalties=penalties,
                                logprobs=logprobs, stop=stop, ban=ban, guide=guide, dry=dry, watermark=watermark, cut=cut)
        vs = _DecodeState(output_ids=output_ids, cache_lens=cache_lens, input_len=input_len, P=prompt_bound, step=0,
                          rows=torch.arange(output_ids.size(0), device=dev))
        rules.bind(vs, output_ids[:, 0], prompt_ids, input_len, (cache_lens, input_len, 1, 0))
        vs.use_graphs = bool(dev.type == "cuda" and self.model.layers[-1].self_attn.shard is None and self.GRAPH_ROUNDS)
        P = prompt_bound                                   # (the replayer holds no reference to the state that holds it)
        vs.replayer = GraphReplayer(self, lambda bound: (P + bound, P + bound), output_ids.size(1), "vanilla step")
        return vs

    def _vanilla_device(self, vs):
        """One token, device work only: the step has no host-side parameter at all."""
        out, cl, il, rows, rules = vs.output_ids, vs.cache_lens, vs.input_len, vs.rows, vs.rules
        cur = out[rows, (cl - il).long()].view(out.size(0), -1)
        hidden_states = self.model.forward(cur, cache_lens=cl, exec_type="decoding").last_hidden_state
        logits = rules.apply(self.lm_head(hidden_states[:, -1, :]))
        # (sampling: the row was rotated to position cl, the length before this step's increment)
        llm_output = rules.tokens(logits, cl)
        pending = rules.pending(logits, llm_output)          # the token's row -> the column it is about to be written to
        cl += 1
        out[rows, (cl - il).long()] = llm_output.view(-1)
        rules.record(pending)
        rules.advance(llm_output.view(out.size(0), 1))

    def vanilla_step(self, vs):
        """Decode one token.  On a GPU the step is captured into a HIP graph after GRAPH_AFTER eager steps and replayed."""
        vs.step += 1
        if vs.use_graphs and vs.step > self.GRAPH_AFTER:
            rp = vs.replayer
            rp.run(None, partial(self._vanilla_device, vs), vs.step + 1, same_call=True)     # (step s reads s rows past the prompt)
            if not rp.failed:
                return
            vs.use_graphs = False
            if rp.issued:                                             # the warm-up step already produced this call's token
                return
            # any other failure has not decoded this call's token: fall through to the eager step
        self._set_hints(vs.P + vs.step, vs.P + vs.step)
        self._vanilla_device(vs)

    # ------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def spec_generate(self, input_ids, prompt_length, gamma=4, max_gen_len=64, eos_id=151645, temperature=0.0,
                      sampling=None, penalties=None, logprobs=None, stop=None, ban=None, guide=None, dry=None, watermark=None, cut=None):                          # :621-774
        return self._chain_generate(input_ids, prompt_length, gamma, max_gen_len, eos_id, temperature, drafter="glide",
                                    sampling=sampling, penalties=penalties, logprobs=logprobs, stop=stop, ban=ban, guide=guide, dry=dry, watermark=watermark, cut=cut)

    @torch.inference_mode()
    def magicdec_generate(self, input_ids, prompt_length, gamma=4, max_gen_len=64, eos_id=151645, temperature=0.0,
                          sampling=None, penalties=None, logprobs=None, stop=None, ban=None, guide=None, dry=None, watermark=None, cut=None):                      # :776-913
        """The MagicDec baseline of the reference's harness (``--method magicdec``): chain speculation where the
        drafter is the TARGET itself attending to a StreamingLLM cache (32 sink rows + the last 1024 prompt rows +
        what it generates), verified exactly like ``spec_generate``.  Same return tuple."""
        return self._chain_generate(input_ids, prompt_length, gamma, max_gen_len, eos_id, temperature, drafter="magicdec",
                                    sampling=sampling, penalties=penalties, logprobs=logprobs, stop=stop, ban=ban, guide=guide, dry=dry, watermark=watermark, cut=cut)

    @torch.inference_mode()
    def vanilla_torch_generate(self, input_ids, prompt_length, max_gen_len=64, eos_id=151645):                      # :587-619
        """``--method vanilla_torch``: the reference's autoregressive loop over its dense-PyTorch attention twins
        (``prefill_torch`` / ``decoding_torch``, llama.py:132-197).  There is one attention implementation here,
        so this is ``vanilla_generate`` (the twins compute the same function; they exist in the reference to
        time flash-attn against eager attention)."""
        return self.vanilla_generate(input_ids, prompt_length, max_gen_len=max_gen_len, eos_id=eos_id)

    def _chain_generate(self, input_ids, prompt_length, gamma, max_gen_len, eos_id, temperature, drafter, sampling=None,
                        penalties=None, logprobs=None, stop=None, ban=None, guide=None, dry=None, watermark=None, cut=None):
        assert input_ids is not None, "please give the input"
        rules = self._rules(input_ids.device, temperature, None, sampling=sampling, penalties=penalties, logprobs=logprobs,
                            stop=stop, ban=ban, guide=guide, dry=dry, watermark=watermark, cut=cut)
        magic = drafter == "magicdec"      # (temperature > 0: the same rejection block in both loops, :715-736 = :854-875)
        self._clear_shard()
        bsz, P = input_ids.size(0), int(input_ids.size(1))
        assert bsz == 1, "the reference's hot path is batch 1 (SURVEY section 1)"
        self.set_max_gen_len(max_gen_len + 128)
        if not magic:
            self.glide.set_max_gen_len(max_gen_len + 128)
        input_len = prompt_length
        logits, cache_lens = self._prefill_target(input_ids, input_len, "magicdec_prefill" if magic else "prefill")
        if not magic:
            self._prefill_draft(input_ids, cache_lens)
        first = rules.first_token(logits, input_len, input_ids)
        st = self.begin_chain_decode(first, cache_lens, input_len, P, gamma, max_gen_len, eos_id, temperature, drafter,
                                     first_logits=logits, prompt_ids=input_ids, rules=rules)
        self.last_logprobs = st.logprobs
        self.last_stop = st.last_stop
        _sync(input_ids)
        start_time = time.time()
        for out_index in range(1, max_gen_len):
            if not self.chain_round(st):
                break
        _sync(input_ids)
        elapsed_time = time.time() - start_time
        return st.output_ids, st.count, st.num, elapsed_time, st.spec_mask

    def begin_chain_decode(self, first_token, cache_lens, input_len, prompt_bound: int, gamma=4, max_gen_len=64, eos_id=151645,
                           temperature=0.0, drafter="glide", first_logits=None, sampling=None, penalties=None, prompt_ids=None,
                           logprobs=None, stop=None, ban=None, guide=None, dry=None, watermark=None, cut=None, rules=None):
        """State of the chain-speculation loop right after the prefills (``llama_glide.py:641-668``): ``first_token`` [bsz]
        = the target's first generated token, ``cache_lens`` [bsz] int32 = valid rows of every cache (the draft's included),
        ``input_len`` [bsz] = prompt length, ``prompt_bound`` = host-side bound of it.  Also the entry point of benchmarks
        that time ``chain_round`` on synthetic KV (bench.py --method seq).  The nine keywords: ``target_rules.py`` (``rules``:
        the ``TargetRules`` the caller has built from them already); ``prompt_ids[z, :input_len[z]]`` is the prompt the penalty
        state starts from (None: no prompt flags).  A round rules the gamma + 1 verification rows: row i follows the text so
        far plus the i draft tokens in front of it and predicts column ``cache_lens - input_len + 1 + i``; the rows a round
        accepts fill their log-prob columns.  A ``stop=`` match ends the loop with that round; the host counters ``count`` /
        ``num`` / ``emitted`` are not rolled back."""
        bsz = first_token.size(0)
        if rules is None:
            rules = self._rules(first_token.device, temperature, self.model.layers[-1].self_attn.shard, sampling=sampling,
                                penalties=penalties, logprobs=logprobs, stop=stop, ban=ban, guide=guide, dry=dry, watermark=watermark, cut=cut)
        if drafter != "magicdec":
            self._head_of_draft_passes()                # the draft passes' head and its pack exist before the first round
        st = SimpleNamespace(gamma=gamma, magic=drafter == "magicdec", temperature=temperature, bsz=bsz, P=int(prompt_bound),
                             max_gen_len=max_gen_len, double_flag=False)
        # temperature > 0 (:639-640,704,709): the draft's fp32 logits of every step, for the rejection test of :716-736
        st.spec_logits = None
        if temperature > 0:
            assert first_logits is not None
            st.spec_logits = first_logits.new_zeros((bsz, gamma + 1, first_logits.size(-1)), dtype=torch.float32)
            st.spec_logits[:, 0] = first_logits
        st.stream_rows = self.model.layers[0].self_attn.STREAM_SINK + self.model.layers[0].self_attn.STREAM_WINDOW
        self._chain_state(st, first_token, cache_lens, input_len, eos_id, prompt_ids, rules)
        st.next_spec_start_token[:, 0] = st.output_ids[:, 0]       # the first draft pass starts from it
        return st

    def _chain_state(self, st, first_token, cache_lens, input_len, eos_id, prompt_ids, rules):
        """What the states of the chain-shaped loops (``begin_chain_decode``, ``begin_lookup_decode``) share, onto ``st``
        (``gamma``, ``bsz``, ``max_gen_len`` set): the text and its mask, gamma columns wider than the budget, the round's
        ``spec_buffer``, the lengths, what ``chain_commit`` keeps for the next round, the host counters and the rules."""
        bsz, gamma = st.bsz, st.gamma
        st.count, st.num, st.emitted = 0, 0, 1
        st.output_ids = first_token.new_zeros((bsz, st.max_gen_len + gamma))
        st.spec_mask = first_token.new_zeros((bsz, st.max_gen_len + gamma))
        st.output_ids[:, 0] = first_token
        st.cache_lens = cache_lens
        st.draft_cache_lens = cache_lens.clone()            # (a drafter without a cache of its own: chain_commit's scratch)
        st.input_len = input_len
        st.input_len_i32 = input_len.to(device=first_token.device, dtype=torch.int32).view(bsz).contiguous()
        st.spec_buffer = st.output_ids.new_zeros((bsz, gamma + 1))
        st.spec_buffer[:, 0] = st.output_ids[:, 0]
        st.next_spec_start_token = st.output_ids.new_zeros((bsz, 2))
        st.eos = self._stop_id(eos_id, "spec")
        rules.bind(st, first_token, prompt_ids, input_len, (st.cache_lens, st.input_len_i32, 1, 0), gamma=gamma)
        return st

    def _tree_state(self, st, first_token, cache_lens, prompt_len, width: int, eos_id, prompt_ids, rules):
        """What the states of the tree-shaped loops (``begin_tree_decode``, ``_begin_lookup_tree``) share, onto ``st``
        (``gamma``, ``Fn``, ``bsz``, ``dev``, ``num`` set): the filled text of ``width`` columns (:937, G8) and its mask, the
        tree (``all_spec``, ``tree_mask``, ``history_logp_sum``: tree_commit resets them together), the accepted ids of the
        last round, the host mirrors, an int32 ``cache_lens`` of the state's own (the tree operators advance the lengths in
        place) and the rules."""
        bsz, Fn, dev = st.bsz, st.Fn, st.dev
        st.fill = self._tree_output_fill(eos_id)
        st.output_ids = torch.full((bsz, width), st.fill, dtype=torch.int64, device=dev)
        st.spec_mask = torch.zeros((bsz, width), dtype=torch.int64, device=dev)
        st.output_ids[:, 0] = first_token
        st.cache_lens = cache_lens.to(torch.int32).clone()
        st.count = 0
        st.all_spec = torch.zeros((bsz, Fn), dtype=torch.int64, device=dev)
        st.all_spec[:, 0] = first_token
        st.tree_mask = torch.zeros((bsz, Fn, Fn), dtype=torch.int64, device=dev)
        st.tree_mask[:, :, 0] = 1
        st.history_logp_sum = torch.zeros((bsz, Fn), dtype=torch.float32, device=dev)
        st.acc_pad = torch.zeros((bsz, st.gamma + 1), dtype=torch.int64, device=dev)
        st.acc_pad[:, 0] = first_token
        st.acc_ids = st.acc_pad[:, :1]
        st.a = 1                              # host mirror of acc_num (G9: the pad id is outside the vocab)
        st.emitted = 1                        # host mirror of emitted_dev: columns of output_ids written so far
        st.emitted_dev = torch.ones((bsz,), dtype=torch.int32, device=dev)
        st.eos = self._stop_id(eos_id, "tree")
        rules.bind(st, first_token, prompt_ids, prompt_len, (st.emitted_dev, None, 0, st.fill))
        return st

    def chain_round(self, st) -> bool:
        """One round of ``spec_generate`` / ``magicdec_generate`` (``llama_glide.py:670-770``): gamma draft steps, one
        (gamma + 1)-row target pass, acceptance by cumulative match.  False = stop (EOS, a ``stop=`` match or the buffer is
        full); on a state a ``stop=`` match has ended, False at once."""
        if st.stopped:
            return False
        gamma, magic, P = st.gamma, st.magic, st.P
        dev = st.output_ids.device
        cache_lens, draft_cache_lens = st.cache_lens, st.draft_cache_lens
        spec_buffer, spec_logits, next_spec_start_token = st.spec_buffer, st.spec_logits, st.next_spec_start_token
        bound = P + st.emitted + gamma + 2
        self._set_hints(bound, bound)
        draft_head = self.lm_head if magic else self._head_of_draft_passes()      # MagicDec: the target drafts with its own head
        for spec_steps in range(0, gamma):
            if spec_steps == 0:
                if st.double_flag:
                    draft_ids = next_spec_start_token[:, 0:2]
                    position_ids = torch.arange(0, 2, device=dev)[None, :] + draft_cache_lens[:, None]
                else:
                    draft_ids = next_spec_start_token[:, 0, None]
                    position_ids = draft_cache_lens[:, None]
            else:
                draft_ids = spec_buffer[:, spec_steps, None]
                position_ids = draft_cache_lens[:, None]
            prenormed = None
            if magic:
                hidden_states = self.model.embed_tokens(draft_ids)
                position_embeddings = self.model.rotary_emb(hidden_states, position_ids)
            else:
                hidden_states, prenormed, position_embeddings = self._draft_head(draft_ids, position_ids=position_ids)
            if magic:        # the target drafts for itself over its streaming cache (:830-836)
                stream_lens = (draft_cache_lens - st.input_len.int() + st.stream_rows).to(torch.int32)
                self.model.set_kv_len_hint(st.stream_rows + st.emitted + gamma + 2)
                hidden_states = self.model.forward(draft_ids, position_embeddings=position_embeddings, cache_lens=stream_lens,
                                                   exec_type="magicdec_decoding").last_hidden_state
                self.model.set_kv_len_hint(bound)
            else:
                hidden_states = self.glide(hidden_states=hidden_states, position_embeddings=position_embeddings,
                                           llm_kv=self._last_kv(), cache_lens=draft_cache_lens,
                                           llm_kv_len=cache_lens, exec_type="decoding", prenormed=prenormed)
            if st.double_flag and spec_steps == 0:
                draft_cache_lens += 2                    # 1 + double_input (batch 1: the host knows the flag)
                current_logp = draft_head(hidden_states[:, -2:, :])
                spec_buffer[:, spec_steps + 1] = self.ops.argmax_rows(current_logp)[:, 1]
                if spec_logits is not None:
                    spec_logits[:, spec_steps + 1, :] = current_logp[:, 1, :]
            else:
                draft_cache_lens += 1
                current_logp = draft_head(hidden_states[:, -1, :])
                spec_buffer[:, spec_steps + 1] = self.ops.argmax_rows(current_logp).view(-1,)
                if spec_logits is not None:
                    spec_logits[:, spec_steps + 1, :] = current_logp
        emitted = st.emitted
        go_on = _chain_round_host(st, self._chain_verify(st, spec_logits))
        st.double_flag = st.emitted - emitted == gamma + 1      # every draft token was accepted
        return go_on

    # ------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def lookup_generate(self, input_ids, prompt_length, gamma=7, max_ngram=3, min_ngram=1, max_gen_len=64, eos_id=151645,
                        sampling=None, penalties=None, logprobs=None, stop=None, branches=1, ban=None, guide=None, dry=None, watermark=None, cut=None):
        """Prompt-lookup (n-gram) speculation (no counterpart in the reference): chain speculation whose drafter is the text
        itself -- the ``gamma`` tokens that followed the most recent earlier occurrence of the last ``min_ngram .. max_ngram``
        tokens of prompt + output (``lookup.py``) -- verified exactly like ``spec_generate``.  No draft weights, no draft KV,
        no draft prefill and no draft pass: the glide layer is never called, so a model without a draft checkpoint can use
        it.  A round is one ``ops.ngram_draft`` and one (gamma + 1)-row target pass.  Same return tuple as ``spec_generate``;
        ``sampling`` / ``penalties`` / ``logprobs`` / ``stop`` / ``ban`` / ``guide`` act on the verification rows as they do there
        (``self.last_logprobs``, ``self.last_stop``); ``self.last_lookup`` holds ``hist`` [bsz, max_ngram + 1] int64 -- how many
        rounds matched at which length, [:, 0] = none -- and ``info`` [bsz, 2] int32 = (n, e) of the last round, both on the
        device.  There is no ``temperature=``: the reference's T > 0 rejection needs the draft logits a lookup does not have.

        ``branches=B`` (2..8; ``B * gamma + gamma + 1 <= 80`` rows): a round drafts up to B distinct continuations
        (``ops.ngram_tree_draft``, ``lookup.py``) as a level-major tree and verifies them in ONE pass with the verification and
        accept halves of ``tree_round``.  ``output_ids`` / ``spec_mask`` are then [bsz, max_gen_len + gamma + 1], filled like
        ``tree_spec_generate``'s, and the loop ends by its rules; ``last_lookup`` also holds ``branches``, ``hist_nb``
        [bsz, B + 1] (rounds by the number of distinct continuations found) and ``won`` [bsz, B] (rounds by the branch of the
        deepest accepted node, counted when a draft token was accepted), and its ``info`` is [bsz, B, 2].  ``branches=1`` is
        the chain loop above, unchanged."""
        assert input_ids is not None, "please give the input"
        gamma, max_ngram, min_ngram = _lookup_check(gamma, max_ngram, min_ngram, branches)
        rules = self._rules(input_ids.device, None, None, sampling=sampling, penalties=penalties, logprobs=logprobs, stop=stop,
                            ban=ban, guide=guide, dry=dry, watermark=watermark, cut=cut)
        self._clear_shard()
        bsz, P = input_ids.size(0), int(input_ids.size(1))
        assert bsz == 1, "the reference's hot path is batch 1 (SURVEY section 1)"
        self.set_max_gen_len(max_gen_len + (128 if branches == 1 else 256))     # (a tree pass appends up to 80 rows)
        input_len = prompt_length
        logits, cache_lens = self._prefill_target(input_ids, input_len)
        first = rules.first_token(logits, input_len, input_ids)
        st = self.begin_lookup_decode(first, cache_lens, input_len, P, input_ids, gamma, max_ngram, min_ngram, max_gen_len, eos_id,
                                      branches=branches, rules=rules)
        self.last_logprobs = st.logprobs
        self.last_stop = st.last_stop
        self.last_lookup = st.last_lookup
        _sync(input_ids)
        start_time = time.time()
        for out_index in range(1, max_gen_len):
            if not self.lookup_round(st):
                break
        _sync(input_ids)
        elapsed_time = time.time() - start_time
        return st.output_ids, st.count, st.num, elapsed_time, st.spec_mask

    def begin_lookup_decode(self, first_token, cache_lens, input_len, prompt_bound: int, prompt_ids, gamma=7, max_ngram=3,
                            min_ngram=1, max_gen_len=64, eos_id=151645, sampling=None, penalties=None, logprobs=None, stop=None,
                            branches=1, ban=None, guide=None, dry=None, watermark=None, cut=None, rules=None):
        """State of the prompt-lookup loop right after the target's prefill: the arguments of ``begin_chain_decode`` that have
        a meaning without a drafter, plus ``prompt_ids`` [bsz, P] -- here not optional: ``prompt_ids[z, :input_len[z]]`` is the
        front of the text the drafter searches (and, under ``penalties``, the source of the prompt flags).  Also the entry point
        of benchmarks that time ``lookup_round`` on synthetic KV.  ``st.hist`` / ``st.info`` (``st.last_lookup``) are what
        ``ops.ngram_draft`` keeps; ``st.replayer`` replays the round from one HIP graph per tier (``lookup_round``).
        ``branches >= 2``: the state of the tree round instead (``_begin_lookup_tree``)."""
        gamma, max_ngram, min_ngram = _lookup_check(gamma, max_ngram, min_ngram, branches)
        bsz = first_token.size(0)
        dev = first_token.device
        if rules is None:
            rules = self._rules(dev, None, self.model.layers[-1].self_attn.shard, sampling=sampling, penalties=penalties,
                                logprobs=logprobs, stop=stop, ban=ban, guide=guide, dry=dry, watermark=watermark, cut=cut)
        if branches > 1:
            return self._begin_lookup_tree(first_token, cache_lens, input_len, int(prompt_bound), prompt_ids, gamma, branches,
                                           max_ngram, min_ngram, max_gen_len, eos_id, rules)
        st = _DecodeState(gamma=gamma, max_ngram=max_ngram, min_ngram=min_ngram, bsz=bsz, P=int(prompt_bound),
                          max_gen_len=max_gen_len, rounds=0)
        st.prompt_ids = prompt_ids.to(device=dev, dtype=torch.int64)
        if st.prompt_ids.stride(-1) != 1:
            st.prompt_ids = st.prompt_ids.contiguous()
        st.info = torch.zeros((bsz, 2), dtype=torch.int32, device=dev)
        st.hist = torch.zeros((bsz, max_ngram + 1), dtype=torch.int64, device=dev)
        st.last_lookup = SimpleNamespace(hist=st.hist, info=st.info)
        self._chain_state(st, first_token, cache_lens, input_len, eos_id, prompt_ids, rules)
        st.use_graphs = bool(dev.type == "cuda" and bsz == 1 and self.model.layers[-1].self_attn.shard is None and self.GRAPH_ROUNDS)
        P, rows = st.P, gamma + 2                          # (the replayer holds no reference to the state that holds it)
        st.replayer = GraphReplayer(self, lambda bound: (P + bound + rows, P + bound + rows), st.output_ids.size(1), "lookup round")
        return st

    def _chain_verify(self, st, spec_logits=None):
        """The verification half of a chain-shaped round (``chain_round``, ``_lookup_device``), device work only: the
        (gamma + 1)-row target pass over ``spec_buffer``, the rules on its rows (row i follows the text and i draft tokens),
        the arg-max or draw, ``chain_commit`` and the rules' commits.  ``spec_logits``: the draft's logits, for the reference's
        rejection test at temperature > 0 (:715-736).  Returns state [bsz, 2] = (correct_len, EOS hit | 2 * stop hit)."""
        gamma, rules, cache_lens, spec_buffer = st.gamma, st.rules, st.cache_lens, st.spec_buffer
        hidden_states = self.model.forward(spec_buffer, cache_lens=cache_lens, exec_type="decoding").last_hidden_state
        llm_verify_logits = rules.apply(self.lm_head(hidden_states[:, -gamma - 1:, :]), spec_buffer[:, 1:], rules.chain_mask,
                                        depth="row")
        # (sampling: verification row i was rotated to position cache_lens + i, models' forward :571-577)
        llm_verify_output = rules.tokens(llm_verify_logits,
                                         cache_lens[:, None] + rules.arange_v if rules.sampling is not None else None)
        # every verification row's log-probs; the commit keeps a prefix of them, at the columns behind the text as it stands
        # BEFORE chain_commit advances it
        pending = rules.pending(llm_verify_logits, llm_verify_output)
        accept = {}
        if spec_logits is not None:
            llm_verify_output, mask = self.ops.chain_accept_stochastic(spec_logits, llm_verify_logits, spec_buffer, llm_verify_output)
            accept = {"accept_mask": mask}
        # acceptance by cumulative match, verified ids + bonus token -> output_ids, cache_lens += correct_len, the next
        # round's start tokens and draft_cache_lens = cache_lens - double_input (:738-770): one launch, one host read
        state = self.ops.chain_commit(llm_verify_output, spec_buffer, st.output_ids, cache_lens, st.draft_cache_lens,
                                      st.input_len_i32, st.next_spec_start_token, st.eos, **accept)
        rules.record(pending, state[:, 0])                   # the correct_len tokens this round wrote, before the host read
        rules.advance(llm_verify_output, state[:, 0], state)
        return state

    def _lookup_device(self, st):
        """The device work of one lookup round (no host read inside, no host-side parameter): the draft from the text, then
        the verification half of ``chain_round``.  The drafter's grid is sized from the bound the round's attention launches
        are sized from (``_set_hints``: the eager round's, or the graph tier's)."""
        bound = self.model.layers[-1].self_attn.kv_len_hint or st.P + st.output_ids.size(1)
        self.ops.ngram_draft(st.prompt_ids, st.input_len_i32, st.output_ids, st.cache_lens, bound, st.gamma, st.max_ngram,
                             st.min_ngram, st.spec_buffer, info=st.info, hist=st.hist)
        return self._chain_verify(st)

    def lookup_round(self, st) -> bool:
        """One round of ``lookup_generate``: the draft from the text, one (gamma + 1)-row target pass, acceptance by cumulative
        match.  False = stop (EOS, a ``stop=`` match or the buffer is full); on a state a ``stop=`` match has ended, False at
        once.  Unlike the glide chain round this one has a static shape -- no ``double_flag``, no draft cache --, so on a GPU
        it is captured into ONE HIP graph per tier after GRAPH_AFTER eager rounds and replayed, as ``vanilla_step`` is."""
        if st.stopped:
            return False
        if getattr(st, "branches", 1) > 1:
            return self._lookup_tree_round(st)
        state = None
        if st.use_graphs and st.rounds >= self.GRAPH_AFTER:
            state = st.replayer.run(None, partial(self._lookup_device, st), st.emitted, same_call=True)
            if st.replayer.failed:
                st.use_graphs = False
        if state is None:
            bound = st.P + st.emitted + st.gamma + 2
            self._set_hints(bound, bound)
            state = self._lookup_device(st)
        st.rounds += 1
        return _chain_round_host(st, state)

    def _begin_lookup_tree(self, first_token, cache_lens, input_len, P: int, prompt_ids, gamma, branches, max_ngram, min_ngram,
                           max_gen_len, eos_id, rules):
        """State of the lookup loop with ``branches >= 2``: ``begin_tree_decode``'s without anything that belongs to a draft
        layer -- ``all_spec`` / ``tree_mask`` of the static level-major tree (Fn = 1 + branches * gamma nodes), ``acc_pad``
        [bsz, gamma + 1], ``a``, ``emitted_dev``, int32 ``cache_lens``, R = Fn - 1 + gamma + 1 verification rows -- and the
        drafter's ``info`` / ``hist`` / ``hist_nb`` / ``won``.  ``output_ids`` (filled and EOS-tested as the tree loop's) is
        max_gen_len + gamma + 1 columns wide: under the tree loop's rule -- stop when ``emitted + gamma + 2`` exceeds the width
        -- the loop does not end before max_gen_len columns are written, and a round's gamma + 1 tokens always fit."""
        bsz = first_token.shape[0]
        dev = first_token.device
        Fn = 1 + branches * gamma
        R = Fn - 1 + gamma + 1
        width = max_gen_len + gamma + 1
        st = _DecodeState(gamma=gamma, branches=branches, max_ngram=max_ngram, min_ngram=min_ngram, Fn=Fn, R=R, P=P, dev=dev,
                          bsz=bsz, max_gen_len=max_gen_len, rounds=0, num=0)
        st.prompt_ids = prompt_ids.to(device=dev, dtype=torch.int64)
        if st.prompt_ids.stride(-1) != 1:
            st.prompt_ids = st.prompt_ids.contiguous()
        st.input_len = input_len
        st.input_len_i32 = input_len.to(device=dev, dtype=torch.int32).view(bsz).contiguous()
        st.info = torch.zeros((bsz, branches, 2), dtype=torch.int32, device=dev)
        st.hist = torch.zeros((bsz, max_ngram + 1), dtype=torch.int64, device=dev)
        st.hist_nb = torch.zeros((bsz, branches + 1), dtype=torch.int64, device=dev)
        st.won = torch.zeros((bsz, branches), dtype=torch.int64, device=dev)
        st.last_lookup = SimpleNamespace(hist=st.hist, info=st.info, branches=branches, hist_nb=st.hist_nb, won=st.won)
        self._tree_state(st, first_token, cache_lens, input_len, width, eos_id, prompt_ids, rules)
        st.use_graphs = bool(dev.type == "cuda" and bsz == 1 and self.model.layers[-1].self_attn.shard is None and self.GRAPH_ROUNDS)
        st.replayer = GraphReplayer(self, lambda bound: (P + bound + R, P + bound + R), width, "lookup tree round")
        return st

    def _tree_verify_pass(self, st, a: int, **bump):
        """The V step of a tree-shaped round (:1078-1091), device work only: one R-row target pass over [a accepted | Fn - 1
        tree nodes | pads].  ``bump`` / ``bump_add``: a length that ``tree_verify_inputs`` advances in its launch.  Returns
        (the hidden states of rows a-1 .. a+Fn-2, position_ids)."""
        veri_spec, position_ids, mask_bits = self.ops.tree_verify_inputs(st.acc_pad[:, :a], a, st.all_spec, st.tree_mask,
                                                                         st.cache_lens, st.R, **bump)
        hidden_states = self.model.forward(veri_spec, position_ids=position_ids, cache_lens=st.cache_lens,
                                           exec_type="tree_decoding", tree_mask_bits=mask_bits).last_hidden_state
        return hidden_states[:, a - 1:a + st.Fn - 1], position_ids

    def _tree_accept(self, st, a: int, llm_logits, position_ids, collapse, commit, pred=None):
        """The accept half of a tree-shaped round (``_round_device``, ``_lookup_tree_device``), device work only, from the
        target's logits of rows a-1 .. a+Fn-2: the rules (row j follows the committed text, the root included, and the nodes on
        node j's path -- the trees grow level by level, so increasing column is increasing depth -- and predicts column
        emitted + depth(j)), the arg-max or draw at the positions RoPE saw, ``tree_collapse(..., *collapse)``,
        ``tree_commit(..., **commit)`` and the rules' commits.  ``pred``: the tokens, where a ``vocab_parallel`` shard's
        ``head_select`` took them and no row of logits exists.  Returns (state [bsz, 2] = (acc_num, EOS hit | 2 * stop hit),
        acc_num, index_mapping)."""
        ops, rules, all_spec, tree_mask = self.ops, st.rules, st.all_spec, st.tree_mask
        pending = None
        if pred is None:
            llm_logits = rules.apply(llm_logits, all_spec[:, 1:], tree_mask[:, :, 1:], depth="tree", tree_mask=tree_mask)
            pred = rules.tokens(llm_logits, position_ids[:, a - 1:a + st.Fn - 1] if rules.sampling is not None else None)
            pending = rules.pending(llm_logits, pred)
        acc_pad, acc_num_t, _, index_mapping = ops.tree_collapse(all_spec, pred, tree_mask, *collapse, out_acc_ids=st.acc_pad)
        # the accepted rows' log-probs -> the columns tree_commit is about to write, behind emitted_dev as it stands now
        rules.record(pending, acc_num_t, index_mapping)
        # emitted tokens -> output_ids (at the device-side offset), the EOS test on the whole buffer as the reference
        # does (:1120, G8), the tree state reset and the length bookkeeping (:1104-1117): one launch; its result is the round's
        # ONE host read for (acc_num, eos flag)
        state = ops.tree_commit(acc_pad, acc_num_t, st.output_ids, 0, st.eos, tree_mask, all_spec, st.history_logp_sum,
                                target_lens=st.cache_lens, target_add=a, emitted_dev=st.emitted_dev, **commit)
        rules.advance(acc_pad, acc_num_t, state)             # the accepted tokens, inside the round (and its graph)
        return state, acc_num_t, index_mapping

    def _lookup_tree_device(self, st, a: int):
        """The device work of one lookup round with ``branches >= 2`` (no host read inside; ``a``, the tokens the last round
        accepted, is its only host-side parameter): the tree from the text, then the V and A halves of ``_round_device``
        without a draft cache to keep.  Returns state [bsz, 2] = (acc_num, EOS hit | 2 * stop hit)."""
        gamma, B = st.gamma, st.branches
        bound = self.model.layers[-1].self_attn.kv_len_hint or st.P + st.output_ids.size(1)
        self.ops.ngram_tree_draft(st.prompt_ids, st.input_len_i32, st.output_ids, st.emitted_dev, bound, gamma, B, st.max_ngram,
                                  st.min_ngram, st.all_spec, st.tree_mask, info=st.info, hist=st.hist, hist_nb=st.hist_nb)
        hidden_states, position_ids = self._tree_verify_pass(st, a)                       # ---- V
        # ---- A: the deepest branch that verifies; no KV row moves (the next pass feeds the accepted tokens again)
        state, acc_num_t, index_mapping = self._tree_accept(st, a, self.lm_head(hidden_states), position_ids,
                                                            (st.cache_lens, 1 + B * (gamma - 1), gamma + 1), {})
        # the branch of the deepest accepted node (node = 1 + (d-1) * B + j), where a draft token was accepted at all
        n = acc_num_t.view(-1, 1).to(torch.int64)
        last = index_mapping.gather(1, (n - 1).clamp(min=0))
        st.won.scatter_add_(1, (last - 1).clamp(min=0) % B, n.ge(2).to(torch.int64))
        return state

    def _lookup_tree_round(self, st) -> bool:
        """``lookup_round`` with ``branches >= 2``: the host side of ``tree_round`` -- one HIP graph per ``a`` and tier after
        GRAPH_AFTER eager rounds, ONE host read -- around ``_lookup_tree_device``."""
        a = st.a
        state = None
        if st.use_graphs and not st.replayer.disabled and st.rounds >= self.GRAPH_AFTER:
            state = st.replayer.run(a, partial(self._lookup_tree_device, st, a), st.emitted)
        if state is None:
            bound = st.P + st.emitted + st.R
            self._set_hints(bound, bound)
            state = self._lookup_tree_device(st, a)
        st.rounds += 1
        return _tree_round_host(st, state)

    # ------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def tree_spec_generate(self, input_ids, prompt_length, tree_shape: Optional[List[int]] = None, max_gen_len=64,
                           eos_id=151645, temperature=0.0, shard=None, sampling=None, penalties=None,
                           logprobs=None, stop=None, ban=None, guide=None, dry=None, watermark=None, cut=None):                                               # :915-1126
        """``shard`` (``dist.KVShard``, every rank of the group calls with the same arguments): the prompt is prefilled
        and its KV kept sequence-sharded over the ranks (``_sharded_prefill``); decoding then runs replicated with one
        exchange per attention call.  Returns the same values on every rank.  The nine keywords: ``target_rules.py``, on every
        verification row; the log-probs are published as ``self.last_logprobs``, the stop result as ``self.last_stop``.  With
        a ``vocab_parallel`` shard all of them but a ``stop`` without ``min_tokens`` are refused."""
        assert input_ids is not None, "please give the input"
        rules = self._rules(input_ids.device, temperature, shard, head_sharded=True, sampling=sampling, penalties=penalties,
                            logprobs=logprobs, stop=stop, ban=ban, guide=guide, dry=dry, watermark=watermark, cut=cut)
        bsz = input_ids.size(0)
        assert bsz == 1, "the reference's hot path is batch 1 (SURVEY section 1)"
        dev = input_ids.device
        self.set_max_gen_len(max_gen_len + 256)
        self.glide.set_max_gen_len(max_gen_len + 256)
        P = int(input_ids.size(1))
        input_len = prompt_length
        for layer in self.model.layers:                    # a model object may be reused with and without a shard
            layer.self_attn.shard = shard
        self.glide.cross_attn.shard = shard
        if shard is not None:
            if dev.type == "cuda" and not shard.peer_tried:
                # a mailbox slot holds the record of the widest pass: 128 rows x heads x (128 + 1) floats
                heads = max(self.config.num_attention_heads, self.glide.config.num_attention_heads)
                shard.enable_peer_exchange(bsz * 128 * heads * 129, dev)
            lens = input_len.to(device=dev, dtype=torch.int32).view(bsz)
            first = self._sharded_prefill(input_ids, input_len, shard, rules)
        else:
            logits, lens = self._prefill_target(input_ids, input_len)
            first = rules.first_token(logits, input_len, input_ids)
            self._prefill_draft(input_ids, lens)
        st = self.begin_tree_decode(first, lens, P, tree_shape, max_gen_len, eos_id, temperature=temperature, prompt_ids=input_ids,
                                    rules=rules)
        self.last_logprobs = st.logprobs
        self.last_stop = st.last_stop
        _sync(input_ids)
        start_time = time.time()
        for out_index in range(1, max_gen_len):
            if not (self.tree_round_stochastic(st) if temperature > 0 else self.tree_round(st)):
                break
            if shard is not None and out_index % 32 == 0:
                shard.raise_if_exchange_failed()
        _sync(input_ids)
        elapsed_time = time.time() - start_time
        if shard is not None:
            # a wait that gave up latches the exchange's error flag and every later wait returns at once: the rounds since
            # then merged stale mailbox records.  Never hand such tokens back (the peers fail the same way: a rank that
            # raises stops pushing, and their next wait times out)
            shard.raise_if_exchange_failed()
        return st.output_ids, st.count, st.num, elapsed_time, st.spec_mask

    def _sharded_prefill(self, input_ids, input_len, shard, rules):
        """Sequence-sharded prefill: rank r runs the target model on prompt rows [r*Ls, (r+1)*Ls) only
        (one all-gather of the layer's K/V rows per layer, ``LlamaAttention.sharded_prefill``) and keeps that slice of the
        KV; the tail rank computes the first token (``rules.first_token``: under ``logprobs`` its log-prob rows too) and broadcasts it.  The
        draft layer's cache is filled on every rank (its rows depend on the token ids only).  Work per rank: 1/W of the projections / MLP, between 1/W^2 (rank 0)
        and (2W-1)/W^2 (tail) of the attention."""
        bsz, P = input_ids.shape
        assert bsz == 1 and int(input_len.view(-1)[0]) == P, "sharded prefill: batch 1, unpadded prompt"
        lo = shard.start
        hi = P if shard.is_tail else min(P, lo + shard.Ls)
        assert hi > lo and (shard.world - 1) * shard.Ls < P <= shard.world * shard.Ls, \
            "sharded prefill: shard_rows must be ceil(prompt / world)-like (every rank owns at least one row)"
        for layer in self.model.layers:
            layer.self_attn.shard = shard
        self.glide.cross_attn.shard = shard
        shard.prefill_ctx = (lo, hi - lo, P)
        try:
            self._set_hints(P, P)
            hidden_states = self.model.forward(input_ids[:, lo:hi], exec_type="prefill",
                                               position_ids=torch.arange(lo, hi, device=input_ids.device)[None, :]).last_hidden_state
        finally:
            shard.prefill_ctx = None
        dev = input_ids.device
        first = torch.zeros((bsz,), dtype=torch.int64, device=dev)
        if rules.top_n is not None:
            rules.first_logprobs = (torch.zeros((bsz, 1), dtype=torch.float32, device=dev),
                                    torch.zeros((bsz, 1, rules.top_n), dtype=torch.float32, device=dev),
                                    torch.zeros((bsz, 1, rules.top_n), dtype=torch.int64, device=dev))
        if shard.is_tail:
            first = rules.first_token(self.lm_head(hidden_states[:, hi - lo - 1, :]), input_len, input_ids)
        shard.broadcast_from_tail(first)
        for t in rules.first_logprobs or ():
            if t.numel():
                shard.broadcast_from_tail(t)
        self._prefill_draft(input_ids, None)
        return first

    def begin_tree_decode(self, first_token, cache_lens, prompt_bound: int, tree_shape=None, max_gen_len=64, eos_id=151645,
                          temperature=0.0, sampling=None, penalties=None, prompt_ids=None, logprobs=None, stop=None, ban=None,
                          guide=None, dry=None, watermark=None, cut=None, rules=None):
        """State of the round loop right after the two prefills (``llama_glide.py:927-991``).
        ``first_token`` [bsz] = the target's first generated token, ``cache_lens`` [bsz] int32 = valid
        rows of every KV cache, ``prompt_bound`` = host-side bound of it.  Also the entry point of
        synthetic-KV benchmarks, which fill the caches themselves instead of prefilling.  The nine keywords:
        ``target_rules.py`` (``rules``: the ``TargetRules`` the caller has built from them already);
        ``prompt_ids[z, :cache_lens[z]]`` is the prompt the penalty state starts from (None: no prompt flags).  A round is the
        temperature-0 round with its Fn verification rows ruled inside the round and its graph: row j follows the committed
        text plus the nodes on node j's path and predicts column emitted + depth(j); the rows on the accepted path fill their
        log-prob columns.  A ``stop=`` match ends the loop with that round; the host counters ``count`` / ``num`` /
        ``emitted`` are not rolled back."""
        dev = first_token.device
        if rules is None:
            rules = self._rules(dev, temperature, self.model.layers[-1].self_attn.shard, head_sharded=True, sampling=sampling,
                                penalties=penalties, logprobs=logprobs, stop=stop, ban=ban, guide=guide, dry=dry, watermark=watermark, cut=cut)
        bsz = first_token.shape[0]
        cand = [4, 16, 16, 16, 16] if tree_shape is None else list(tree_shape)
        acc_n = [1]
        for c in cand:
            acc_n.append(acc_n[-1] + c)
        Fn = acc_n[-1]                       # tree nodes incl. the root
        gamma = len(cand)
        R = Fn - 1 + gamma + 1               # verification rows: [a accepted | F-1 tree | pads]
        self._head_of_draft_passes()                    # the draft passes' head and its pack exist before the first warm-up round
        st = _DecodeState(cand=cand, acc_n=acc_n, Fn=Fn, gamma=gamma, R=R, P=prompt_bound, dev=dev, bsz=bsz, num=bsz)
        cache_lens = cache_lens.to(torch.int32)              # the tree operators advance the three lengths in place
        self._tree_state(st, first_token, cache_lens, cache_lens, max_gen_len, eos_id, prompt_ids, rules)
        st.target_cache_lens_for_draft = cache_lens.clone()
        st.draft_cache_lens = cache_lens.clone()
        # HIP graphs of the round, one per `a`: on a GPU; under a KV shard only when its exchange is the peer-store one
        # (kernel launches only: dist.PeerExchange) -- callers that bracket kernels with events switch it off per round
        sh = self.model.layers[-1].self_attn.shard
        st.use_graphs = bool(dev.type == "cuda" and (sh is None or sh.graph_safe) and self.GRAPH_ROUNDS)
        st.graphs_forced = False                               # prepare_tree_graphs: replay from the first round on
        # the captured rounds are sized for the tier of the first token; st.graph_tiers / st.graph_captures are diagnostics
        # (tools/e2e_longgen.py, the soak test)
        P = prompt_bound                                       # (the replayer holds no reference to the state that holds it)
        st.replayer = GraphReplayer(self, lambda bound: (P + bound + R, P + bound + Fn), max_gen_len, "decode round",
                                    bound=self._tier_bound(1, max_gen_len), tiers=1, share_pool=True)
        st.arange_g = torch.arange(gamma + 2, device=dev)[None, :]
        st.temperature = float(temperature)
        if temperature > 0:
            # stochastic verification (:1093-1102): the draft's log-probs of every tree node are kept (`spec_logits`, :964),
            # up to gamma + 2 tokens come back per round.  Rounds run launch by launch (host reads inside) until the
            # generation is GRAPH_AFTER rounds old, then from HIP graphs keyed by (a, d0_rows): batch 1 only
            st.spec_logits = None                      # allocated at the first lm_head call (vocabulary size)
            st.acc_pad = torch.zeros((bsz, gamma + 2), dtype=torch.int64, device=dev)
            st.acc_pad[:, 0] = first_token
            st.acc_ids = st.acc_pad[:, :1]
            st.use_graphs = bool(st.use_graphs and self.GRAPH_STOCHASTIC and bsz == 1)
            st.fused_logp = False                      # the graph path: spec_logits is written by ops.logprob_topk
            st.mt_host = st.mt_words = st.noise = None  # ... and the round's random draws live in persistent buffers
            st.input_len = cache_lens.clone()
            st.d0_rows = 1                             # rows of the next draft step 0 = width of the last acc_ids
        return st

    def tree_round(self, st) -> bool:
        """One draft-then-verify round (``llama_glide.py:997-1121``): 1 + (gamma-1) draft passes growing
        the beam tree, one R-row target pass, accept/collapse.  Returns False when generation must stop.

        Everything between two host reads is device work whose only host-side parameter is ``a``, the number of
        tokens accepted by the previous round (1..gamma+1).  With ``st.use_graphs`` the round is captured once per
        value of ``a`` into a HIP graph and replayed: the ~370 launches of a round (most of them 4-20 us draft
        kernels the host cannot issue fast enough) become one."""
        if st.stopped:                                                # a stop= match ended this state: no device work
            return False
        a = st.a
        state = None
        if st.use_graphs and not st.replayer.disabled and (st.graphs_forced or st.num >= self.GRAPH_AFTER * st.bsz):
            state = st.replayer.run(a, partial(self._round_device, st, a), st.emitted)
        if state is None:
            # host bounds: no cache holds more than P + emitted (+ this round's speculative rows) valid rows
            self._set_hints(st.P + st.emitted + st.R, st.P + st.emitted + st.Fn)
            state = self._round_device(st, a)
        return _tree_round_host(st, state)

    def _tier_bound(self, emitted: int, total: int) -> int:
        """Emitted-token bound of the graph tier that holds `emitted` (GRAPH_TIER; the whole budget when tiers are off)."""
        tier = self.GRAPH_TIER
        if not tier or tier <= 0:
            return total
        return min(total, (emitted // tier + 1) * tier)

    def prepare_tree_graphs(self, st):
        """Capture the round graphs of every accepted-token count now instead of on first use (benchmarks: keeps the
        captures out of the timed region).  The warm-up rounds run on a snapshot of the decode state: they only
        scribble on cache rows beyond the valid lengths."""
        rp = st.replayer
        if not st.use_graphs or rp.disabled:
            return
        if st.temperature > 0:      # the stochastic rounds capture on first use only (keys (a, d0_rows), tree_round_stochastic)
            return
        st.graphs_forced = True
        names = ("cache_lens", "target_cache_lens_for_draft", "draft_cache_lens", "tree_mask", "all_spec", "history_logp_sum",
                 "acc_pad", "output_ids", "emitted_dev")
        tensors = [getattr(st, n) for n in names] + st.rules.state_tensors()     # (a warm-up round advances the rules' state too)
        with rp.guard():
            rp.roll_over(st.emitted)
            for a in range(1, st.gamma + 2):
                if rp.captured(a):
                    continue
                device_round = partial(self._round_device, st, a)
                if a not in rp.entries:
                    snap = [t.clone() for t in tensors]
                    rp.warm(a, device_round)
                    for t, saved in zip(tensors, snap):
                        t.copy_(saved)
                rp.capture(a, device_round)

    def _round_device(self, st, a: int):
        """The device work of one round (no host read inside): returns state [bsz, 2] = (acc_num, eos hit).
        The length tensors are passed without the reference's ``.clone()``: their in-place updates (inside
        ``ops.tree_grow`` / ``tree_verify_inputs`` / ``tree_commit``) are ordered behind the kernels that read them on
        the same stream."""
        cand, acc_n, Fn, gamma, bsz = st.cand, st.acc_n, st.Fn, st.gamma, st.bsz
        tree_mask, all_spec, history_logp_sum = st.tree_mask, st.all_spec, st.history_logp_sum
        ops = self.ops
        last_attn = self.model.layers[-1].self_attn
        # ---- D0: the a accepted tokens through the draft layer (:1003-1027).  At temperature > 0 the reference feeds the
        # whole zero-padded acc_ids row (its width, not acc_num, :1003): the extra rows only write cache rows that are
        # overwritten before they are read, but the ROW COUNT enters the bottom-right alignment of the causal cross-attention
        # (row i sees llm_kv_len - sq + i keys), so it is reproduced.
        n0 = a if st.temperature == 0 else st.d0_rows
        hidden_states, prenormed, position_embeddings = self._draft_head(st.acc_pad[:, :n0], pos_base=st.draft_cache_lens)
        hidden_states = self.glide(hidden_states=hidden_states, position_embeddings=position_embeddings,
                                   llm_kv=self._last_kv(), cache_lens=st.draft_cache_lens,
                                   llm_kv_len=st.target_cache_lens_for_draft, exec_type="decoding", prenormed=prenormed)
        # log_softmax + top-k of the draft's next-token distribution (:1019-1020), fused on the fp16 logits.  Under a shard
        # with `vocab_parallel` every rank multiplies by its slice of the lm_head only (dist.KVShard.head_select)
        vsh = last_attn.shard if (last_attn.shard is not None and last_attn.shard.vocab_parallel and st.temperature == 0) else None
        vocab_size = self.lm_head.out_features
        draft_head = self._head_of_draft_passes()             # (the vocabulary-sharded head_select path stays on the 16-bit lm_head)
        if vsh is not None:
            topk_logp, pred_ids = vsh.head_select(self.lm_head, hidden_states[:, a - 1, :], ops, k=cand[0])
        else:
            logits = draft_head(hidden_states[:, a - 1, :]).view(bsz, 1, -1)
            if st.temperature > 0:                     # spec_logits[:, 0] = current_logp (:1025, G8: log-probs, not logits)
                if st.spec_logits is None:
                    st.spec_logits = torch.zeros((bsz, Fn, vocab_size), dtype=torch.float32, device=logits.device)
                if not st.fused_logp:
                    st.spec_logits[:, 0] = logits[:, 0].float().log_softmax(dim=-1)
            if st.temperature > 0 and st.fused_logp:   # the graph path: the top-k launches store the row themselves
                topk_logp, pred_ids = ops.logprob_topk(logits, None, cand[0], logp_out=st.spec_logits[:, 0:1])
            else:
                topk_logp, pred_ids = ops.logprob_topk(logits, None, cand[0])
        # the root's children (:1021-1027): tree_mask rows + diagonal, all_spec, log-prob sums, and
        # `draft_cache_lens += a - 1` -- one launch, which also hands back the next pass's positions and packed mask
        position_ids, mask_bits = ops.tree_grow(tree_mask, all_spec, history_logp_sum, topk_logp, pred_ids, vocab_size, 0, 1,
                                                base=st.draft_cache_lens, base_add=a - 1)
        # ---- D1..: tree levels (:1029-1075)
        for ms in range(1, gamma):
            lo, mid = acc_n[ms - 1], acc_n[ms]
            hidden_states, prenormed, position_embeddings = self._draft_head(all_spec[:, lo:mid], position_ids=position_ids)   # p + depth (:1032)
            hidden_states = self.glide(hidden_states=hidden_states, position_embeddings=position_embeddings,
                                       llm_kv=self._last_kv(), cache_lens=st.draft_cache_lens,
                                       llm_kv_len=st.target_cache_lens_for_draft, exec_type="tree_decoding",
                                       tree_mask=tree_mask[:, lo:mid, :mid], tree_mask_bits=mask_bits, prenormed=prenormed)
            # log_softmax + cumulative log-prob + flat top-k over (node, token) (:1046-1064), one fused operator
            if vsh is not None:
                topk_logp_sum, topk_indices = vsh.head_select(self.lm_head, hidden_states, ops, k=cand[ms],
                                                              history=history_logp_sum[:, lo:mid])
            else:
                level_logits = draft_head(hidden_states)
                if st.temperature > 0 and st.fused_logp:
                    topk_logp_sum, topk_indices = ops.logprob_topk(level_logits, history_logp_sum[:, lo:mid], cand[ms],
                                                                   logp_out=st.spec_logits[:, lo:mid])
                else:
                    if st.temperature > 0:             # spec_logits[:, lo:mid] = current_logp (:1074)
                        st.spec_logits[:, lo:mid] = level_logits.float().log_softmax(dim=-1)
                    topk_logp_sum, topk_indices = ops.logprob_topk(level_logits, history_logp_sum[:, lo:mid], cand[ms])
            # father = index // vocab, token = index % vocab, mask row = father's row + diagonal (:1056-1075)
            position_ids, mask_bits = ops.tree_grow(tree_mask, all_spec, history_logp_sum, topk_logp_sum, topk_indices,
                                                    vocab_size, lo, mid, base=st.draft_cache_lens, want_next=ms + 1 < gamma)
        # ---- V: one R-row target pass (:1078-1091); `draft_cache_lens += 1` (:1076) rides in the input assembly
        hidden_states, position_ids = self._tree_verify_pass(st, a, bump=st.draft_cache_lens, bump_add=1)
        if st.temperature > 0:
            return self.lm_head(hidden_states)         # the stochastic branch continues in tree_round_stochastic
        # under a shard with `vocab_parallel` every rank takes the arg-max over its slice of the lm_head: no row of logits to rule
        pred = vsh.head_select(self.lm_head, hidden_states, ops, argmax=True).view(bsz, -1) if vsh is not None else None
        llm_logits = self.lm_head(hidden_states) if vsh is None else None
        # ---- A: accept / reject tree collapse + last-layer KV row move (:1104-1116); the accepted rows start at
        # cache_lens + a - 1 (:1104), the cache lengths themselves advance in the commit (`cache_lens += a`,
        # `target_cache_lens_for_draft += acc_num`)
        sh = last_attn.shard
        if sh is None:
            kv_lens, kc, vc = st.cache_lens, last_attn.K_Cache, last_attn.V_Cache
        elif sh.is_tail:      # the accepted rows live in the tail owner's local cache
            kv_lens, kc, vc = sh.local_len(st.cache_lens), last_attn.K_Cache, last_attn.V_Cache
        else:
            kv_lens, kc, vc = st.cache_lens, None, None
        return self._tree_accept(st, a, llm_logits, position_ids, (kv_lens, acc_n[-2], gamma + 1, kc, vc, a - 1),
                                 dict(draft_kv_lens=st.target_cache_lens_for_draft), pred)[0]

    def tree_round_stochastic(self, st) -> bool:
        """One round at temperature > 0 (``llama_glide.py:997-1102,1110-1121``).  The draft passes and the verification pass
        are those of ``tree_round``; acceptance is ``verify_stochastic``.  The bookkeeping follows the reference's T > 0
        branch AS IT IS, which differs from its T = 0 branch (documented): ``cache_lens`` advances by
        ``acc_num - 1`` only (no ``+= 1``), the accepted rows of the last layer's KV are NOT compacted, and the whole
        zero-padded ``acc_ids`` row is written to ``output_ids`` at ``cache_lens - input_len`` -- so later rounds overwrite
        part of what earlier rounds wrote.  Reproduced token for token (tests/golden/verify_stochastic.npz)."""
        a = st.a
        if a + st.Fn - 1 > st.R:
            # the reference fails here too: gamma + 2 accepted tokens do not fit its veri_spec buffer (:1081)
            raise RuntimeError(f"stochastic round: {a} accepted tokens + {st.Fn - 1} tree nodes exceed the {st.R}-row "
                               f"verification batch (the reference raises at llama_glide.py:1081 in the same state)")
        if st.use_graphs and not st.replayer.disabled and st.num >= self.GRAPH_AFTER * st.bsz:
            return self._graph_round_stochastic(st, a)
        # host bound of the valid rows, per round as in the eager T = 0 path: every round reads acc_num on the host anyway, and
        # the lengths (cache_lens advances by a - 1 per round, the draft's by acc_num) never exceed P + the sum of the accepted
        # counts -- NOT the whole token budget, which sized a 1k-prompt / 20k-budget run for 21k-row launches from round 1
        # 
        bound = min(st.emitted, st.output_ids.size(1))
        self._set_hints(st.P + bound + st.R, st.P + bound + st.Fn)
        llm_logits = self._round_device(st, a)                               # [bsz, Fn, V]
        st.cache_lens += a - 1                                               # :1094
        acc_ids, acc_num = self.verify_stochastic(st.all_spec, st.tree_mask, llm_logits, st.spec_logits, st.temperature)
        W = acc_ids.size(-1)
        cols = (st.cache_lens - st.input_len).long().unsqueeze(1) + torch.arange(W, device=acc_ids.device)[None, :]
        st.output_ids[torch.arange(st.bsz, device=acc_ids.device)[:, None], cols] = acc_ids          # :1102
        st.target_cache_lens_for_draft += acc_num.to(torch.int32)            # :1110
        n = int(acc_num[0])
        st.emitted += int(acc_num.max()) if st.bsz > 1 else n                # host mirror: an upper bound of every length's growth
        st.count += n - 1
        st.num += st.bsz
        st.tree_mask.fill_(0)
        st.tree_mask[:, :, 0] = 1
        st.all_spec.fill_(0)
        st.all_spec[:, 0] = acc_ids[:, n - 1]
        st.history_logp_sum.zero_()
        st.acc_pad.zero_()
        st.acc_pad[:, :W] = acc_ids
        st.acc_ids = st.acc_pad[:, :n]
        st.a = n
        st.d0_rows = W
        if int((st.cache_lens + acc_num.to(torch.int32) - st.input_len).max()) + st.gamma + 2 > st.output_ids.size(1):   # :1118
            return False
        if st.eos is not None and bool(st.output_ids.eq(st.eos).any()):      # :1120
            return False
        return True

    def _stochastic_device(self, st, a: int):
        """The device work of one round at temperature > 0 (no host read inside): the draft passes with the log-prob table
        stored by the top-k launches, the verification pass, ``cache_lens += a - 1`` (:1094), the acceptance walk on the
        pre-drawn randomness in ``st.mt_words`` / ``st.noise`` and the commit.  Returns state [1, 4] = (acc_num, eos hit,
        words_used, budget exhausted)."""
        ops = self.ops
        st.fused_logp = True
        try:
            llm_logits = self._round_device(st, a)                           # [1, Fn, V]
        finally:
            st.fused_logp = False                                            # (the eager rounds keep torch's log_softmax)
        st.cache_lens += a - 1
        # a beam tree grown from tree_shape has depth gamma: the reference's `tree_mask.sum(-1).max() + 1` (:1193) is gamma + 2
        acc_ids, acc_num, used = ops.tree_verify_stochastic(st.all_spec, st.tree_mask, llm_logits, st.spec_logits, st.temperature,
                                                            st.mt_words, st.noise, st.gamma + 2)
        return ops.tree_commit_stochastic(acc_ids, acc_num, used, st.output_ids, st.cache_lens, st.input_len, st.gamma, st.eos,
                                          st.tree_mask, st.all_spec, st.history_logp_sum, st.target_cache_lens_for_draft,
                                          st.acc_pad)

    def _graph_round_stochastic(self, st, a: int) -> bool:
        """``tree_round_stochastic`` from a HIP graph per (a, d0_rows): one replay and ONE host read per round.  The random
        streams are the eager path's, drawn once per round out here -- ``ops.MT_WORDS`` words of Python's ``random`` (rewound
        after the read to what the walk consumed, as ``ops.verify_stochastic`` does) and one Exponential(1) row -- and copied
        into the persistent buffers the captured walk reads.  Whatever becomes of the capture (warm-up, replay, or a failure
        that sends this round and all later ones down the eager road), these draws are the round's only ones."""
        import random
        import numpy as np
        ops, dev, W = self.ops, st.dev, st.gamma + 2
        V, dtype = self.lm_head.out_features, self.model.embed_tokens.weight.dtype
        if st.mt_words is None:                        # nothing is allocated inside a capture
            if st.spec_logits is None:
                st.spec_logits = torch.zeros((st.bsz, st.Fn, V), dtype=torch.float32, device=dev)
            st.mt_host = torch.empty((1, ops.MT_WORDS), dtype=torch.int32).pin_memory()
            st.mt_words = torch.empty((1, ops.MT_WORDS), dtype=torch.int32, device=dev)
            st.noise = torch.empty((1, V), dtype=dtype, device=dev)
        rng_state = random.getstate()
        words = random.getrandbits(32 * ops.MT_WORDS).to_bytes(4 * ops.MT_WORDS, "little")   # = MT_WORDS x getrandbits(32)
        st.mt_host.numpy()[0, :] = np.frombuffer(words, dtype=np.int32)
        noise_fn = getattr(ops, "stochastic_noise_fn", None)
        noise = noise_fn(V, dtype, dev) if noise_fn is not None else torch.empty((V,), dtype=dtype, device=dev).exponential_(1)
        st.mt_words.copy_(st.mt_host, non_blocking=True)       # (the round's host read below is behind this copy)
        st.noise.copy_(noise.view(1, V))
        device_round = partial(self._stochastic_device, st, a)
        state = st.replayer.run((a, st.d0_rows), device_round, st.emitted)
        if state is None:                              # the capture failed before the round was issued: eagerly, same draws
            bound = min(st.emitted, st.output_ids.size(1))
            self._set_hints(st.P + bound + st.R, st.P + bound + st.Fn)
            state = device_round()
        n, hit, used, over = state.tolist()[0]                               # the round's ONE host read
        random.setstate(rng_state)
        if used < 0:
            raise RuntimeError("verify_stochastic: the pre-drawn random words were exhausted")
        if used:
            random.getrandbits(32 * used)
        st.acc_ids = st.acc_pad[:, :n]
        st.a = n
        st.d0_rows = W
        st.emitted += n
        st.count += n - 1
        st.num += st.bsz
        if over:                                                             # :1118
            return False
        if hit:                                                              # :1120
            return False
        return True

    def verify_stochastic(self, input_ids, tree_mask, p_llm, p_ssm, temperature):               # :1177-1245
        """Drop-in for ``LlamaGlide.verify_stochastic``: (acc_ids [bsz, depth + 2] zero padded, acc_num [bsz])."""
        return self.ops.verify_stochastic(input_ids, tree_mask, p_llm, p_ssm, temperature)

    # ------------------------------------------------------------------------------------------
    def tree_verification(self, input_ids, output_ids, tree_mask, cache_lens, non_leaf_len):      # :1128-1175
        """Drop-in for ``LlamaGlide.tree_verification``: returns (acc_ids [bsz, acc_max],
        acc_num [bsz], double_input [bsz] int) and moves the last layer's KV rows."""
        depth = int(tree_mask.sum(dim=-1).max())
        last_attn = self.model.layers[-1].self_attn
        acc_pad, acc_num, double_input, _ = self.ops.tree_collapse(input_ids, output_ids, tree_mask, cache_lens, non_leaf_len,
                                                                   depth, last_attn.K_Cache, last_attn.V_Cache)
        return acc_pad[:, :int(acc_num.max())], acc_num, double_input


def _truncate_after_eos_vanilla(output_ids, num, eos, bsz):
    """The reference tests for EOS after every token and stops (``llama_glide.py:578``); this
    loop tests every 16 tokens to avoid a device sync per token, then restores the reference's
    visible result: tokens after the first EOS are zero, ``num`` counts forward passes up to it.  Returns
    (output_ids, num, steps the reference would have run or None)."""
    hit = output_ids.eq(eos)
    if not bool(hit.any()):
        return output_ids, num, None
    # the reference's loop always runs its first step: an EOS as the very first token stops it after step 1 (:571-579)
    first = max(int(hit.float().argmax(dim=-1).min()), 1)
    output_ids[:, first + 1:] = 0
    return output_ids, first * bsz, first
