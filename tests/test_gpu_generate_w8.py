"""FP8 (e4m3) weights end to end: a model after ``quantize_weights_(scope)`` generates, token for token, what a fresh 16-bit
model loaded from its state_dict generates -- both sides run the same arithmetic on the same numbers (the 8-bit skinny GEMM is
bit-identical to the 16-bit one on the de-quantised weights), so there is no near-tie allowance.  HIP graphs on."""
import pytest
import torch

import cases
from test_gpu_generate import build

pytestmark = pytest.mark.gpu
RUNS = list(cases.generate_runs()) + list(cases.generate_runs("qwen2")) + list(cases.generate_runs("qwen2_bf16"))


def _generate(m, run):
    m.GRAPH_AFTER = 0                                     # replay rounds from HIP graphs as early as possible
    ids = run["prompt"].cuda()
    pl = torch.tensor([run["prompt_len"]], device="cuda")
    kw = dict(max_gen_len=run["max_gen_len"], eos_id=run["eos_id"])
    v_out, v_num, _ = m.vanilla_generate(ids, pl, **kw)
    s_out, s_count, s_num, _, _ = m.spec_generate(ids, pl, gamma=4, **kw)
    t_out, t_count, t_num, _, _ = m.tree_spec_generate(ids, pl, tree_shape=run["tree_shape"], **kw)
    return dict(vanilla=(v_out.cpu(), int(v_num)), chain=(s_out.cpu(), int(s_count), int(s_num)),
                tree=(t_out.cpu(), int(t_count), int(t_num)))


@pytest.mark.parametrize("scope", ["all", "draft"])
@pytest.mark.parametrize("run", RUNS, ids=lambda r: r["name"] + ("_bf16" if r["dtype"] == torch.bfloat16 else ""))
def test_quantized_model_equals_16bit_model_of_its_state_dict(run, scope):
    from longspec_amd import ops
    from longspec_amd.llama import DecodeLinear
    a = build(run).quantize_weights_(scope)
    in_scope = [m for m in a.modules() if isinstance(m, DecodeLinear) and m.weight_quant == "fp8"]
    assert in_scope and all(m.quant_scope == "draft" for m in in_scope) == (scope == "draft")
    b = build(run)
    b.load_state_dict(a.state_dict(), strict=True)
    assert all(m.weight_quant is None for m in b.modules() if isinstance(m, DecodeLinear))
    n0 = ops.W8_CALLS
    got = _generate(a, run)
    used = ops.W8_CALLS - n0
    assert used > 0, "the quantised model never went through ls_linear_w8_fwd"
    assert all(isinstance(p, ops.PackedWeight8) for m in in_scope for p in m._packed.values())
    assert any(m._packed for m in in_scope)
    n1 = ops.W8_CALLS
    want = _generate(b, run)
    assert ops.W8_CALLS == n1, "the 16-bit twin must not use the 8-bit entry point"
    for kind in ("vanilla", "chain", "tree"):
        assert torch.equal(got[kind][0], want[kind][0]), f"{kind}: output_ids differ"
        assert got[kind][1:] == want[kind][1:], f"{kind}: count / num differ: {got[kind][1:]} vs {want[kind][1:]}"
