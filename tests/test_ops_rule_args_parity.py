"""What the rule operators of ``longspec_amd/ops.py`` hand to the C ABI, and what they refuse, against a recording
(tests/golden/ops_rule_args.json) made by ``python tests/test_ops_rule_args_parity.py --record`` at the commit the file names,
BEFORE the wrappers' shared argument handling moved into private helpers.  No GPU: ``ops._dev`` is a no-op, ``ops._stream``
returns 0 and ``_C.load`` returns a recorder whose every symbol logs its arguments and returns 0 (``*_bytes``: 4096).

The wrappers: ``logprob_topk``, ``argmax_rows``, ``sample_rows``, ``penalize_rows``, ``token_state_add``, ``token_logprobs``,
``logprob_commit``, ``stop_scan``, ``stop_ban_rows``, ``ban_rows``, ``guide_rows``, ``guide_advance``, ``ngram_draft`` and
``ngram_tree_draft``.  A case is one wrapper called with named keyword arguments; its outcome is

* ``["raise", exception type, message]``, or
* ``["calls", [[symbol, args], ...], result]``: every library call in order.  A pointer argument is ``[name of the case tensor
  whose storage it points into, byte offset from that tensor's first element]``, ``"fresh"`` for memory the wrapper allocated
  (a copy, an output, a workspace) and None for a null pointer; a float is its ``float.hex()``; a descriptor passed by
  reference is the dict of its fields.  ``result`` holds shape, dtype, strides and pointer of every tensor returned and whether
  it IS the ``logits`` argument (the in-place contract of ``stop_ban_rows``, ``ban_rows`` and ``guide_rows``).

Cases (V = 32): every logits wrapper over [b, V] and [b, R, V], b in {1, 2}, R in {1, 3}, in six layouts -- contiguous, padded
row and batch strides, a row stride that is no multiple of 8, a storage offset of one element, a transposed view and a column
stride of 2; the extras of ``penalize_rows`` / ``ban_rows`` / ``guide_rows`` absent, empty, [b, R, C], [R, C], with a padded
mask row stride and at and one above each operator's limit; ``num`` absent, contiguous and a strided column; ids 1-D and 2-D;
and one refusal per ``raise`` statement the fourteen wrappers had at the recorded commit (``refuse/...``, each with exactly one
defect; the recording counts the statements), plus refusals that come from helpers shared before (``refuse+/...``)."""
import ast
import ctypes
import itertools
import json
import os
import sys
from types import SimpleNamespace as NS

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__" and ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from longspec_amd import _C, ops, Penalties, Sampling  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_rule_args.json")
V, W, TOPN = 32, 8, 2
F16, BF16, F32, I32, I64 = torch.float16, torch.bfloat16, torch.float32, torch.int32, torch.int64
WRAPPERS = ("logprob_topk", "argmax_rows", "sample_rows", "penalize_rows", "token_state_add", "token_logprobs", "logprob_commit",
            "stop_scan", "stop_ban_rows", "ban_rows", "guide_rows", "guide_advance", "ngram_draft", "ngram_tree_draft")
INPLACE = ("stop_ban_rows", "ban_rows", "guide_rows")        # they return the logits object itself
LAYOUTS = ("contiguous", "padded", "odd_stride", "offset1", "transposed", "col_stride2")
GUIDE_WORDS = 16


def z(*shape, dtype=I64):
    return torch.zeros(shape, dtype=dtype)


def logits(b, R, layout="contiguous", dtype=F16):
    """[b, R, V], or [b, V] with ``R`` None, in one of LAYOUTS."""
    rows = 1 if R is None else R
    if layout == "contiguous":
        x = z(b, rows, V, dtype=dtype)
    elif layout == "padded":
        x = z(b, rows + 1, V + 8, dtype=dtype)[:, :rows, :V]
    elif layout == "odd_stride":
        x = z(b, rows, V + 4, dtype=dtype)[..., :V]
    elif layout == "offset1":
        x = z(b * rows * V + 1, dtype=dtype)[1:].view(b, rows, V)
    elif layout == "transposed":
        x = z(b, V, rows, dtype=dtype).transpose(1, 2)
    else:
        x = z(b, rows, V, 2, dtype=dtype)[..., 0]
    return x[:, 0] if R is None else x


def extras(b, R, C, kind="b_r_c"):
    mask = {"b_r_c": lambda: z(b, R, C), "r_c": lambda: z(R, C), "padded_mask": lambda: z(b, R, C + 8)[..., :C]}[kind]()
    return dict(extra_ids=z(b, C), extra_mask=mask)


def lp_out(b, n=TOPN, w=W):
    return NS(token=z(b, w, dtype=F32), top=z(b, w, n, dtype=F32), top_ids=z(b, w, n))


def params(wrapper, b=2, R=3, layout="contiguous", dtype=F16, **over):
    """The keyword arguments of a plain good call of ``wrapper``, ``over`` laid on top."""
    x = logits(b, R, layout, dtype)
    rows = 1 if R is None else R
    lead = (b,) if R is None else (b, R)
    F = 1 + 2 * 3
    p = {
        "logprob_topk": lambda: dict(logits=x, history=None, k=4),
        "argmax_rows": lambda: dict(logits=x),
        "sample_rows": lambda: dict(logits=x, positions=z(*lead), sampling=Sampling(0.8, top_k=5, top_p=0.9, seed=7)),
        "penalize_rows": lambda: dict(logits=x, state=z(b, V, dtype=I32), penalties=Penalties(1.1, 0.2, 0.3)),
        "token_state_add": lambda: dict(state=z(b, V, dtype=I32), ids=z(b, 4)),
        "token_logprobs": lambda: dict(logits=x, ids=z(*lead), temperature=0.7, n=TOPN),
        "logprob_commit": lambda: dict(rows=(z(b, rows, dtype=F32), z(b, rows, TOPN, dtype=F32), z(b, rows, TOPN)), out=lp_out(b),
                                       base=z(b, dtype=I32)),
        "stop_scan": lambda: dict(output_ids=z(b, W), table=z(ops.STOP_TABLE_WORDS, dtype=I32), stop_state=z(b, 4, dtype=I32),
                                  written=z(b, dtype=I32)),
        "stop_ban_rows": lambda: dict(logits=x, table=z(ops.STOP_TABLE_WORDS, dtype=I32)),
        "ban_rows": lambda: dict(logits=x, table=z(ops.BAN_TABLE_WORDS, dtype=I32), output_ids=z(b, W)),
        "guide_rows": lambda: dict(logits=x, table=z(GUIDE_WORDS, dtype=I32), state=z(b, dtype=I32)),
        "guide_advance": lambda: dict(state=z(b, dtype=I32), table=z(GUIDE_WORDS, dtype=I32), ids=z(b, 4)),
        "ngram_draft": lambda: dict(prompt_ids=z(b, 8), input_len=z(b, dtype=I32), output_ids=z(b, W), cache_lens=z(b, dtype=I32),
                                    len_bound=16, gamma=3, max_ngram=3, min_ngram=1, spec_buffer=z(b, 4)),
        "ngram_tree_draft": lambda: dict(prompt_ids=z(b, 8), input_len=z(b, dtype=I32), output_ids=z(b, W), written=z(b, dtype=I32),
                                         len_bound=16, gamma=3, branches=2, max_ngram=3, min_ngram=1, all_spec=z(b, F),
                                         tree_mask=z(b, F, F)),
    }[wrapper]()
    p.update(over)
    return p


def build_cases():
    """[(case name, wrapper, keyword arguments)], in a fixed order."""
    cases = []

    def add(name, wrapper, **kw):
        sel = {k: kw.pop(k) for k in ("b", "R", "layout", "dtype") if k in kw}
        cases.append((f"{wrapper}/{name}", wrapper, params(wrapper, **sel, **kw)))

    def refuse(name, wrapper, **kw):
        add("refuse/" + name, wrapper, **kw)

    def refuse_more(name, wrapper, **kw):
        add("refuse+/" + name, wrapper, **kw)

    # ---- the logits grid
    grid = [(b, R) for b in (1, 2) for R in (None, 1, 3)]
    for wrapper in ("logprob_topk", "argmax_rows", "sample_rows", "penalize_rows", "token_logprobs", "stop_ban_rows", "ban_rows",
                    "guide_rows"):
        for (b, R), layout in itertools.product(grid, LAYOUTS):
            add(f"b{b}_R{R}_{layout}", wrapper, b=b, R=R, layout=layout)
        add("bf16", wrapper, dtype=BF16)
        # a batch stride that is no multiple of 8 under a row stride that is one, at b = 1: not every wrapper looks at it
        add("b1_odd_batch_stride", wrapper, logits=z(200, dtype=F16).as_strided((1, 3, V), (100, 40, 1)), b=1)
        if wrapper not in INPLACE:
            refuse_more("fp32_logits", wrapper, dtype=F32)

    # ---- extras: absent (the grid), empty, [b, R, C], [R, C], padded mask rows, at and above the limit
    for wrapper, limit in (("penalize_rows", 1024), ("ban_rows", ops.BAN_MAX_EXTRA), ("guide_rows", ops.GUIDE_MAX_EXTRA)):
        for b, R in ((1, 1), (2, 3)):
            add(f"extras_empty_b{b}_R{R}", wrapper, b=b, R=R, **extras(b, R, 0))
            add(f"extras_empty_ids_only_b{b}_R{R}", wrapper, b=b, R=R, extra_ids=z(b, 0))
            for kind in ("b_r_c", "r_c", "padded_mask"):
                add(f"extras_{kind}_b{b}_R{R}", wrapper, b=b, R=R, **extras(b, R, 5, kind))
        add("extras_b_r_c_2d_logits", wrapper, b=2, R=None, **extras(2, 1, 5))
        add("extras_padded_logits", wrapper, layout="padded", **extras(2, 3, 5, "r_c"))
        add("extras_at_limit", wrapper, **extras(2, 3, limit))
        if wrapper == "penalize_rows":
            add("extras_above_limit", wrapper, **extras(2, 3, limit + 1))
            add("extras_mask_only", wrapper, extra_mask=z(2, 3, 5))
        add("extras_ids_row_stride", wrapper, extra_ids=z(2, 9)[:, :5], extra_mask=z(2, 3, 5))

    # ---- the other keywords of the logits wrappers
    add("history", "logprob_topk", history=z(2, 3, dtype=F32))
    add("history_fp16_strided", "logprob_topk", history=z(2, 3, 2, dtype=F16)[..., 0])
    add("logp_out", "logprob_topk", logp_out=z(2, 3, V, dtype=F32))
    add("logp_out_padded", "logprob_topk", history=z(2, 3, dtype=F32), logp_out=z(2, 4, V + 8, dtype=F32)[:, :3, :V])
    add("streams", "sample_rows", streams=z(2, 3, dtype=I32))
    add("top2", "sample_rows", return_top2=True)
    add("top2_upper", "sample_rows", return_top2=True, return_upper=True)
    add("min_p", "sample_rows", sampling=Sampling(0.8, top_k=5, top_p=0.9, seed=7, min_p=0.1), streams=z(2, 3))
    add("typical_p_padded", "sample_rows", layout="padded", sampling=Sampling(1.3, seed=9, typical_p=0.5), return_top2=True)
    add("positions_int32_strided", "sample_rows", positions=z(2, 3, 2, dtype=I32)[..., 0])
    add("bias_built", "penalize_rows", penalties=Penalties(1.1, 0.2, 0.3, bias={3: 1.5}))
    add("bias_given", "penalize_rows", bias=z(V, dtype=F32))
    add("state_padded", "penalize_rows", state=z(2, V + 8, dtype=I32)[:, :V])
    add("n0", "token_logprobs", n=0)
    add("ids_1d", "token_logprobs", R=None, ids=z(2))
    add("ids_flat_for_rows", "token_logprobs", R=1, ids=z(2))
    add("ids_strided", "token_logprobs", ids=z(2, 3, 2)[..., 0])
    add("ids_row_stride", "token_logprobs", ids=z(2, 5)[:, :3])
    for depth in (None, "row", "tree"):
        add(f"depth_{depth}", "stop_ban_rows", depth=depth, tree_mask=z(2, 3, 7) if depth == "tree" else None,
            base=z(2, dtype=I32), base_sub=z(2, dtype=I32), base_add=3)
    add("tree_mask_padded", "stop_ban_rows", layout="padded", depth="tree", tree_mask=z(2, 4, 9)[:, :3, :7])
    add("tree_mask_ignored", "stop_ban_rows", depth="row", tree_mask=z(2, 3, 7))
    add("base", "ban_rows", base=z(2, dtype=I32), base_sub=z(2, dtype=I32), base_add=-1)
    add("no_text", "ban_rows", output_ids=None)
    add("text_w0", "ban_rows", output_ids=z(2, 0))
    add("text_padded", "ban_rows", output_ids=z(2, W + 3)[:, :W], **extras(2, 3, 5))
    add("text_b1_stride0", "ban_rows", b=1, output_ids=z(W).expand(1, W))
    add("table_larger", "guide_rows", table=z(100, dtype=I32))

    # ---- num: absent (the defaults), contiguous, a strided column; ids: 1-D and 2-D, and a column stride
    for wrapper in ("token_state_add", "guide_advance", "logprob_commit", "stop_scan"):
        for b in (1, 2):
            add(f"num_none_b{b}", wrapper, b=b)
            add(f"num_contiguous_b{b}", wrapper, b=b, num=z(b))
            add(f"num_strided_b{b}", wrapper, b=b, num=z(b, 2)[:, 0])
    for wrapper in ("token_state_add", "guide_advance"):
        add("ids_1d", wrapper, ids=z(2))
        add("ids_1d_many", wrapper, ids=z(8))
        add("ids_1d_b1", wrapper, b=1, ids=z(5))
        add("ids_row_stride", wrapper, ids=z(2, 9)[:, :4])
        add("ids_col_stride", wrapper, ids=z(2, 4, 2)[..., 0])
        add("ids_one_col_strided", wrapper, ids=z(2, 2)[:, :1])
    add("ids_at_limit", "guide_advance", ids=z(2, ops.GUIDE_MAX_EXTRA))
    add("ids_empty", "token_state_add", ids=z(2, 0))
    add("prompt", "token_state_add", prompt=True)
    add("state_padded", "token_state_add", state=z(2, V + 8, dtype=I32)[:, :V])
    add("index_map", "logprob_commit", index_map=z(2, 2), base_add=1, num=z(2, 2)[:, 1])
    add("n0", "logprob_commit", rows=(z(2, 3, dtype=F32), z(2, 3, 0, dtype=F32), z(2, 3, 0)), out=lp_out(2, 0))
    add("all", "stop_scan", written_sub=z(2, dtype=I32), written_add=1, num=z(2, 2)[:, 0], fill=7, state=z(2, 2), spec_mask=z(2, W),
        logprobs=lp_out(2))
    add("num_const", "stop_scan", num_const=3, logprobs=lp_out(2, 0))
    add("padded", "stop_scan", output_ids=z(2, W + 4)[:, :W], state=z(2, 5)[:, :3], spec_mask=z(2, W + 4)[:, :W])
    for wrapper in ("ngram_draft", "ngram_tree_draft"):
        for b in (1, 2):
            add(f"plain_b{b}", wrapper, b=b)
        add("padded_text", wrapper, prompt_ids=z(2, 12)[:, :8], output_ids=z(2, W + 4)[:, :W])
        add("b1_stride0", wrapper, b=1, prompt_ids=z(8).expand(1, 8))
    add("info_hist", "ngram_draft", info=z(2, 2, dtype=I32), hist=z(2, 4))
    add("info_hist", "ngram_tree_draft", info=z(2, 2, 2, dtype=I32), hist=z(2, 4), hist_nb=z(2, 3))

    # ---- one refusal per raise statement of the wrappers
    refuse("logp_out", "logprob_topk", logp_out=z(2, 3, V, dtype=F16))
    refuse("positions", "sample_rows", positions=z(2, 2))
    refuse("streams", "sample_rows", streams=z(2, 2, dtype=I32))
    refuse("logits_dim", "penalize_rows", logits=z(1, 2, 3, V, dtype=F16), state=z(1, V, dtype=I32))
    refuse("state", "penalize_rows", state=z(2, V))
    refuse("ids_need_mask", "penalize_rows", extra_ids=z(2, 5))
    refuse("extra_ids", "penalize_rows", extra_ids=z(2, 5, dtype=I32), extra_mask=z(2, 3, 5))
    refuse("extra_mask", "penalize_rows", extra_ids=z(2, 5), extra_mask=z(2, 2, 5))
    refuse("bias", "penalize_rows", bias=z(V, dtype=F16))
    refuse("state", "token_state_add", state=z(2, V))
    refuse("ids", "token_state_add", ids=z(2, 4, dtype=I32))
    refuse("num", "token_state_add", num=z(2, dtype=I32))
    refuse("logits_dim", "token_logprobs", logits=z(1, 2, 3, V, dtype=F16))
    refuse("ids", "token_logprobs", ids=z(2, 3, dtype=I32))
    refuse("row_lp", "logprob_commit", rows=(z(2, 3, dtype=F16), z(2, 3, TOPN, dtype=F32), z(2, 3, TOPN)))
    refuse("base", "logprob_commit", base=z(2))
    refuse("index_map", "logprob_commit", index_map=z(2, 2, dtype=I32))
    refuse("num", "logprob_commit", num=z(2, dtype=I32))
    refuse("output_ids", "stop_scan", output_ids=z(2, W, dtype=I32))
    refuse("stop_state", "stop_scan", stop_state=z(2, 3, dtype=I32))
    refuse("num", "stop_scan", num=z(2, dtype=I32))
    refuse("num_const", "stop_scan", num_const=-1)
    refuse("state", "stop_scan", state=z(2, 1))
    refuse("spec_mask", "stop_scan", spec_mask=z(2, W + 1))
    refuse("logprobs", "stop_scan", logprobs=NS(token=z(2, W, dtype=F16), top=z(2, W, TOPN, dtype=F32), top_ids=z(2, W, TOPN)))
    for wrapper in ("stop_ban_rows", "ban_rows", "guide_rows"):
        refuse("logits", wrapper, dtype=F32)
        refuse("overlapping", wrapper, logits=z(1, 1, V, dtype=F16).expand(2, 3, V))
    refuse("depth", "stop_ban_rows", depth="level")
    refuse("tree_mask", "stop_ban_rows", depth="tree")
    refuse("table", "ban_rows", table=z(ops.BAN_TABLE_WORDS - 1, dtype=I32))
    refuse("output_ids", "ban_rows", output_ids=z(2, W, dtype=I32))
    refuse("output_ids_overlapping", "ban_rows", output_ids=z(W).expand(2, W))
    refuse("state", "guide_rows", state=z(2))
    for wrapper, limit in (("ban_rows", ops.BAN_MAX_EXTRA), ("guide_rows", ops.GUIDE_MAX_EXTRA)):
        refuse("ids_need_mask", wrapper, extra_ids=z(2, 5))
        refuse("extras_above_limit", wrapper, **extras(2, 3, limit + 1))
        refuse("extra_ids", wrapper, extra_ids=z(2, 5, dtype=I32), extra_mask=z(2, 3, 5))
        refuse("extra_mask", wrapper, extra_ids=z(2, 5), extra_mask=z(2, 2, 5))
        refuse("mask_needs_ids", wrapper, extra_mask=z(2, 3, 5))
    refuse("state", "guide_advance", state=z(2))
    refuse("ids", "guide_advance", ids=z(2, 4, dtype=I32))
    refuse("ids_above_limit", "guide_advance", ids=z(2, ops.GUIDE_MAX_EXTRA + 1))
    refuse("num", "guide_advance", num=z(2, dtype=I32))
    for wrapper in ("ngram_draft", "ngram_tree_draft"):
        refuse("prompt_ids", wrapper, prompt_ids=z(2, 8, dtype=I32))
        refuse("prompt_rows", wrapper, prompt_ids=z(3, 8))
        refuse("gamma", wrapper, gamma=ops.NGRAM_MAX_GAMMA + 1)
        refuse("len_bound", wrapper, len_bound=0)
        refuse("info", wrapper, info=z(2, 2))
        refuse("hist", wrapper, hist=z(2, 3))
    refuse("spec_buffer", "ngram_draft", spec_buffer=z(2, 5))
    refuse("all_spec", "ngram_tree_draft", all_spec=z(2, 8))
    refuse("tree_mask", "ngram_tree_draft", tree_mask=z(2, 7, 8))

    # ---- further refusals: the other disjuncts and loop members of those statements, and the helpers shared before
    refuse_more("logp_out_shape", "logprob_topk", logp_out=z(2, 3, V + 8, dtype=F32))
    refuse_more("state_shape", "penalize_rows", state=z(1, V, dtype=I32))
    refuse_more("extra_ids_rows", "penalize_rows", extra_ids=z(3, 5), extra_mask=z(2, 3, 5))
    refuse_more("extra_mask_batch", "penalize_rows", extra_ids=z(2, 5), extra_mask=z(3, 3, 5))
    refuse_more("extra_mask_4d", "penalize_rows", extra_ids=z(2, 5), extra_mask=z(1, 2, 3, 5))
    refuse_more("extra_mask_col_stride", "penalize_rows", extra_ids=z(2, 5), extra_mask=z(2, 3, 5, 2)[..., 0])
    refuse_more("bias_other_penalties", "penalize_rows", penalties=Penalties(bias={V: 1.0}))
    refuse_more("ids_rows", "token_state_add", ids=z(3, 4))
    refuse_more("num_2d", "token_state_add", num=z(2, 1))
    refuse_more("ids_numel", "token_logprobs", ids=z(2, 2))
    for i, name in enumerate(("top_val", "top_idx")):
        rows = [z(2, 3, dtype=F32), z(2, 3, TOPN, dtype=F32), z(2, 3, TOPN)]
        rows[i + 1] = rows[i + 1].to(F16)
        refuse_more(name, "logprob_commit", rows=tuple(rows))
    for name in ("token", "top", "top_ids"):
        out = lp_out(2)
        setattr(out, name, getattr(out, name).to(F16))
        refuse_more("out_" + name, "logprob_commit", out=out)
        if name != "token":
            refuse_more("logprobs_" + name, "stop_scan", logprobs=out)
    refuse_more("base_strided", "logprob_commit", base=z(2, 2, dtype=I32)[:, 0])
    refuse_more("table", "stop_scan", table=z(ops.STOP_TABLE_WORDS + 1, dtype=I32))
    refuse_more("written", "stop_scan", written=z(2))
    refuse_more("written_sub", "stop_scan", written_sub=z(2, 2, dtype=I32)[:, 0])
    refuse_more("table", "stop_ban_rows", table=z(ops.STOP_TABLE_WORDS, dtype=I64))
    refuse_more("base", "stop_ban_rows", base=z(3, dtype=I32))
    refuse_more("tree_mask_rows", "stop_ban_rows", depth="tree", tree_mask=z(2, 2, 7))
    for wrapper in ("stop_ban_rows", "ban_rows", "guide_rows"):
        refuse_more("logits_col_stride", wrapper, layout="col_stride2")
        refuse_more("logits_4d", wrapper, logits=z(1, 2, 3, V, dtype=F16))
        refuse_more("overlapping_rows_only", wrapper, logits=z(2, 1, V, dtype=F16).expand(2, 3, V))
    refuse_more("base_sub", "ban_rows", base_sub=z(2))
    refuse_more("output_ids_rows", "ban_rows", output_ids=z(3, W))
    for wrapper in ("guide_rows", "guide_advance"):
        refuse_more("table_short", wrapper, table=z(ops.GUIDE_HEADER_WORDS - 1, dtype=I32))
        refuse_more("table_misaligned", wrapper, table=z(GUIDE_WORDS + 1, dtype=I32)[1:])
    refuse_more("ids_empty", "guide_advance", ids=z(2, 0))
    for wrapper in ("ngram_draft", "ngram_tree_draft"):
        refuse_more("output_ids", wrapper, output_ids=z(2, W, 2)[..., 0])
        refuse_more("overlapping", wrapper, output_ids=z(W).expand(2, W))
        refuse_more("min_ngram", wrapper, min_ngram=4)
        refuse_more("input_len", wrapper, input_len=z(2))
    refuse_more("cache_lens", "ngram_draft", cache_lens=z(2))
    refuse_more("branches", "ngram_tree_draft", branches=0, all_spec=z(2, 1), tree_mask=z(2, 1, 1))
    refuse_more("hist_nb", "ngram_tree_draft", hist_nb=z(2, 2))
    refuse_more("written", "ngram_tree_draft", written=z(2))
    return cases


class Recorder:
    """Stands in for the loaded library: every attribute is a function that logs (symbol, args)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, symbol):
        def fn(*args):
            self.calls.append((symbol, args))
            return 4096 if symbol.endswith("_bytes") else 0
        return fn


def named_tensors(kw):
    for key, v in kw.items():
        if isinstance(v, torch.Tensor):
            yield key, v
        elif isinstance(v, (tuple, list)):
            yield from ((f"{key}[{i}]", t) for i, t in enumerate(v))
        elif isinstance(v, NS):
            yield from ((f"{key}.{a}", t) for a, t in vars(v).items())


def pointer(p, tensors):
    if p is None:
        return None
    if isinstance(p, int) and p == 0:
        return 0
    for exact in (True, False):
        for name, t in tensors:
            lo = t.untyped_storage().data_ptr()
            if (p == t.data_ptr() and t.numel()) if exact else lo <= p < lo + t.untyped_storage().nbytes():
                return [name, p - t.data_ptr()]
    return "fresh"


def plain(v, ctype, tensors):
    if ctype is ctypes.c_void_p:
        return pointer(v, tensors)
    if ctype is ctypes.c_float:
        return float(v).hex()
    if isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer):
        d = v._obj
        return {f: plain(getattr(d, f), t, tensors) for f, t in d._fields_}
    return int(v)


def describe(res, kw, tensors):
    if res is None:
        return None
    if isinstance(res, torch.Tensor):
        return {"shape": list(res.shape), "dtype": str(res.dtype), "strides": list(res.stride()),
                "ptr": pointer(res.data_ptr(), tensors) if res.numel() else None, "is_logits": res is kw.get("logits")}
    return [describe(r, kw, tensors) for r in res]


def outcome(wrapper, kw):
    rec = Recorder()
    tensors = list(named_tensors(kw))
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "_dev", lambda *ts: None)
        mp.setattr(ops, "_stream", lambda: 0)
        mp.setattr(_C, "load", lambda: rec)
        try:
            res = getattr(ops, wrapper)(**kw)
        except Exception as e:                                        # noqa: BLE001
            return ["raise", type(e).__name__, str(e)]
    calls = [[sym, [plain(a, t, tensors) for a, t in zip(args, _C.SYMBOLS[sym][1], strict=True)]] for sym, args in rec.calls]
    return ["calls", calls, describe(res, kw, tensors)]


def count_raises():
    """``raise`` statements per wrapper in the ops.py of this checkout (``--record`` keeps them in the recording)."""
    with open(ops.__file__) as f:
        tree = ast.parse(f.read())
    return {n.name: sum(isinstance(m, ast.Raise) for m in ast.walk(n)) for n in tree.body
            if isinstance(n, ast.FunctionDef) and n.name in WRAPPERS}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


CASES = build_cases()


def test_case_table_is_the_recorded_one(golden):
    names = [name for name, _, _ in CASES]
    assert len(set(names)) == len(names)
    assert names == list(golden["cases"])
    assert {w for _, w, _ in CASES} == set(WRAPPERS)


@pytest.mark.parametrize("wrapper", WRAPPERS)
def test_outcomes_are_the_recorded_ones(golden, wrapper):
    mine = [(name, kw) for name, w, kw in CASES if w == wrapper]
    assert mine
    for name, kw in mine:
        got = json.loads(json.dumps(outcome(wrapper, kw)))
        assert got == golden["cases"][name], name
        if "/refuse" in name:
            assert got[0] == "raise", name
        elif wrapper in INPLACE and got[0] == "calls":          # (the grid's non-unit column strides are refused)
            assert got[2]["is_logits"], name


def test_every_raise_statement_is_reached(golden):
    """As many distinct refusal messages among the ``refuse/`` cases as the wrappers had ``raise`` statements, per wrapper."""
    for wrapper in WRAPPERS:
        msgs = [golden["cases"][name] for name, w, _ in CASES if w == wrapper and "/refuse/" in name]
        assert all(m[0] == "raise" for m in msgs)
        assert len({m[2] for m in msgs}) == len(msgs) == golden["raise_statements"][wrapper], wrapper
    assert sum(golden["raise_statements"].values()) == golden["raise_statements_total"]


def record():
    import subprocess
    commit = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    dirty = subprocess.check_output(["git", "status", "--porcelain", "--", "longspec_amd"], cwd=ROOT, text=True).strip()
    assert not dirty, "record at a clean checkout of longspec_amd/"
    raises = count_raises()
    out = {"what": "outcomes of tests/test_ops_rule_args_parity.py, recorded by its --record", "commit": commit,
           "raise_statements": raises, "raise_statements_total": sum(raises.values()),
           "cases": {name: outcome(w, kw) for name, w, kw in CASES}}
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    n_raise = sum(o[0] == "raise" for o in out["cases"].values())
    print(f"{GOLDEN}: {len(CASES)} cases ({n_raise} refusals) at {commit[:7]}; raise statements: {raises}")


if __name__ == "__main__":
    if "--record" in sys.argv:
        record()
    else:
        sys.exit("usage: python tests/test_ops_rule_args_parity.py --record")
