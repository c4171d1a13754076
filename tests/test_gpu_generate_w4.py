"""MXFP4 weights and the draft-pass lm_head end to end.

A model after ``quantize_weights_(scope, fmt="mxfp4")`` generates, token for token, what a fresh 16-bit model loaded from its
state_dict generates; a model with a low-precision ``draft_lm_head`` generates what a model whose ``draft_lm_head`` is a 16-bit
``DecodeLinear`` with the same (rounded) weight generates.  Both sides run the same arithmetic on the same numbers (the 4-bit
and 8-bit skinny GEMMs are bit-identical to the 16-bit one on the de-quantised weights), so there is no near-tie allowance.
HIP graphs on."""
import pytest
import torch

import cases
from test_gpu_generate import build

pytestmark = pytest.mark.gpu
RUNS = list(cases.generate_runs()) + list(cases.generate_runs("qwen2")) + list(cases.generate_runs("qwen2_bf16"))
_ids = lambda r: r["name"] + ("_bf16" if r["dtype"] == torch.bfloat16 else "")          # noqa: E731


def _generate(m, run, vanilla=True):
    m.GRAPH_AFTER = 0                                     # replay rounds from HIP graphs as early as possible
    ids = run["prompt"].cuda()
    pl = torch.tensor([run["prompt_len"]], device="cuda")
    kw = dict(max_gen_len=run["max_gen_len"], eos_id=run["eos_id"])
    out = {}
    if vanilla:
        v_out, v_num, _ = m.vanilla_generate(ids, pl, **kw)
        out["vanilla"] = (v_out.cpu(), int(v_num))
    s_out, s_count, s_num, _, _ = m.spec_generate(ids, pl, gamma=4, **kw)
    t_out, t_count, t_num, _, _ = m.tree_spec_generate(ids, pl, tree_shape=run["tree_shape"], **kw)
    out["chain"] = (s_out.cpu(), int(s_count), int(s_num))
    out["tree"] = (t_out.cpu(), int(t_count), int(t_num))
    return out


def _same(got, want):
    for kind in want:
        assert torch.equal(got[kind][0], want[kind][0]), f"{kind}: output_ids differ"
        assert got[kind][1:] == want[kind][1:], f"{kind}: count / num differ: {got[kind][1:]} vs {want[kind][1:]}"


@pytest.mark.parametrize("scope", ["all", "draft"])
@pytest.mark.parametrize("run", RUNS, ids=_ids)
def test_mxfp4_model_equals_16bit_model_of_its_state_dict(run, scope):
    from longspec_amd import ops
    from longspec_amd.llama import DecodeLinear
    a = build(run).quantize_weights_(scope, fmt="mxfp4")
    in_scope = [m for m in a.modules() if isinstance(m, DecodeLinear) and m.weight_quant == "mxfp4"]
    assert in_scope and all(m.quant_scope == "draft" for m in in_scope) == (scope == "draft")
    assert not any(m.weight_quant == "fp8" for m in a.modules() if isinstance(m, DecodeLinear))
    b = build(run)
    b.load_state_dict(a.state_dict(), strict=True)
    assert all(m.weight_quant is None for m in b.modules() if isinstance(m, DecodeLinear))
    n0 = ops.W4_CALLS
    got = _generate(a, run)
    assert ops.W4_CALLS > n0, "the quantised model never went through ls_linear_w4_fwd"
    assert all(isinstance(p, ops.PackedWeight4) for m in in_scope for p in m._packed.values())
    assert any(m._packed for m in in_scope)
    n1 = ops.W4_CALLS
    want = _generate(b, run)
    assert ops.W4_CALLS == n1, "the 16-bit twin must not use the 4-bit entry point"
    _same(got, want)


def _plain_twin_head(a):
    """A 16-bit DecodeLinear that carries the weight of ``a.draft_lm_head``."""
    from longspec_amd.llama import DecodeLinear
    src = a.draft_lm_head
    with torch.device("meta"):
        head = DecodeLinear(src.in_features, src.out_features, bias=False, ops=a.ops)
    head.weight = torch.nn.Parameter(src.weight.detach().clone(), requires_grad=False)
    assert head.weight_quant is None
    return head


def _calls(ops, fmt):
    return ops.W4_CALLS if fmt == "mxfp4" else ops.W8_CALLS


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
@pytest.mark.parametrize("run", RUNS, ids=_ids)
def test_draft_head_equals_16bit_head_with_its_weight(run, fmt):
    from longspec_amd import ops
    keys = list(build(run).state_dict().keys())
    a = build(run).quantize_draft_head_(fmt)
    assert list(a.state_dict().keys()) == keys and a.lm_head.weight_quant is None
    assert isinstance(a.draft_lm_head.packed(), ops.PackedWeight4 if fmt == "mxfp4" else ops.PackedWeight8)
    b = build(run)
    b.draft_lm_head = _plain_twin_head(a)
    plain = build(run)
    assert torch.equal(a.lm_head.weight, plain.lm_head.weight)
    n0 = _calls(ops, fmt)
    got = _generate(a, run)
    assert _calls(ops, fmt) > n0, "the draft passes never streamed the low-precision head"
    n1 = ops.W4_CALLS + ops.W8_CALLS
    want = _generate(b, run, vanilla=False)
    assert ops.W4_CALLS + ops.W8_CALLS == n1
    _same(got, want)
    # the target path is not affected: vanilla decoding is the untouched model's
    m = plain
    m.GRAPH_AFTER = 0
    v_out, v_num, _ = m.vanilla_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"),
                                         max_gen_len=run["max_gen_len"], eos_id=run["eos_id"])
    assert torch.equal(got["vanilla"][0], v_out.cpu()) and got["vanilla"][1] == int(v_num)


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_low_precision_launches_per_tree_round_are_the_draft_passes(fmt):
    """Launch by launch (no graphs): every tree round streams the low-precision head once per draft pass -- step 0 and the
    gamma - 1 levels -- and the verify pass, the prefill's first token and vanilla decoding add none."""
    from longspec_amd import ops
    run = RUNS[0]
    a = build(run).quantize_draft_head_(fmt)
    a.GRAPH_ROUNDS = False
    ids, pl = run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda")
    kw = dict(max_gen_len=run["max_gen_len"], eos_id=run["eos_id"])
    rounds, per_round = [], []
    orig = a._round_device

    def spy(st, n):
        before = _calls(ops, fmt)
        r = orig(st, n)
        per_round.append(_calls(ops, fmt) - before)
        rounds.append(st.gamma)
        return r

    a._round_device = spy
    n0 = _calls(ops, fmt)
    a.tree_spec_generate(ids, pl, tree_shape=run["tree_shape"], **kw)
    assert rounds and per_round == rounds, (per_round, rounds)
    assert _calls(ops, fmt) - n0 == sum(rounds), "a launch outside the draft passes used the low-precision head"
    n1 = _calls(ops, fmt)
    a.vanilla_generate(ids, pl, **kw)
    assert _calls(ops, fmt) == n1
    # the chain drafter: gamma launches per round, none in the verify pass
    s_rounds = []
    orig_chain = a.chain_round

    def spy_chain(st):
        before = _calls(ops, fmt)
        r = orig_chain(st)
        s_rounds.append(_calls(ops, fmt) - before)
        return r

    a.chain_round = spy_chain
    a.spec_generate(ids, pl, gamma=4, **kw)
    assert s_rounds and all(n == 4 for n in s_rounds), s_rounds


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_stochastic_tree_run_with_graphs_reads_the_draft_head(fmt):
    """One T = 0.8 tree run replayed from HIP graphs: the same seed on ``a`` (low-precision draft head) and ``b`` (16-bit head
    with the same weight) gives the same tokens, so the stochastic path reads the draft head's log-probs consistently."""
    import random
    from longspec_amd import ops
    run = RUNS[0]
    a = build(run).quantize_draft_head_(fmt)
    b = build(run)
    b.draft_lm_head = _plain_twin_head(a)
    outs = []
    n0 = _calls(ops, fmt)
    for m in (a, b):
        m.GRAPH_AFTER = 0
        random.seed(7001)
        torch.manual_seed(8001)
        out, count, num, _, _ = m.tree_spec_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"),
                                                     tree_shape=run["tree_shape"], max_gen_len=run["max_gen_len"],
                                                     eos_id=run["eos_id"], temperature=0.8)
        outs.append((out.cpu(), int(count), int(num)))
        if m is a:
            assert _calls(ops, fmt) > n0
            n1 = ops.W4_CALLS + ops.W8_CALLS
    assert ops.W4_CALLS + ops.W8_CALLS == n1
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1:] == outs[1][1:], (outs[0][1:], outs[1][1:])


@pytest.mark.parametrize("mode,fmt", [("fp8", "fp8"), ("fp4", "mxfp4")])
def test_env_default_builds_the_draft_head_at_first_use(monkeypatch, mode, fmt):
    """LONGSPEC_DRAFT_HEAD: the head is built inside the first generation (under inference_mode, before the first round), the
    rounds replay from graphs, and the tokens are those of the model whose head was built by hand."""
    from longspec_amd import ops
    from longspec_amd.llama_glide import DRAFT_HEAD_ENV
    run = RUNS[0]
    want = _generate(build(run).quantize_draft_head_(fmt), run, vanilla=False)
    monkeypatch.setenv(DRAFT_HEAD_ENV, mode)
    a = build(run)
    assert a.draft_lm_head is None
    n0 = _calls(ops, fmt)
    got = _generate(a, run, vanilla=False)
    assert a.draft_lm_head is not None and a.draft_lm_head.weight_quant == fmt and _calls(ops, fmt) > n0
    assert a.lm_head.weight_quant is None
    _same(got, want)
