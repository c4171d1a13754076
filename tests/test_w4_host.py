"""MXFP4 (e2m1 elements, e8m0 block scales) weights, host side: the block quantiser of longspec_amd/quant.py against a literal
restatement of its definition, ``quantize_weight_("mxfp4")`` / ``quantize_weights_(fmt="mxfp4")`` and the draft-pass lm_head on
a toy LlamaGlide driven by the oracle's operators (no GPU)."""
import pytest
import torch

import cases
import oracle_ops

GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _mk(shape, seed, scale, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _blocks(t):
    return t.view(t.shape[0], -1, 32)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("K", [256, 4096])
@pytest.mark.parametrize("std", [0.03, None, 4.0], ids=["std0.03", "stdK^-0.5", "std4"])
def test_quantize_blocks_mxfp4_definition(dtype, K, std):
    """Every de-quantised value is a grid value times 2^E; 3 * 2^E < amax <= 6 * 2^E wherever E is not clamped; each element is
    the nearest grid value; the de-quantised values are the same numbers in fp32, fp16 and bf16 and every non-zero fp16 one
    is normal; re-quantising the de-quantised weight returns the same VALUES always, and the same (q, e) except for blocks
    whose largest element rounded to 3 (there E moves down by one and the elements double)."""
    from longspec_amd import quant
    w = _mk((200, K), 5 + K, std if std is not None else K ** -0.5, dtype)
    w[7] = 0
    q, e = quant.quantize_blocks_mxfp4(w)
    assert q.dtype == torch.uint8 and q.shape == (200, K // 2) and e.dtype == torch.uint8 and e.shape == (200, K // 32)
    E = e.to(torch.int32) - 127
    assert int(E.min()) >= -13 and int(E.max()) <= 13
    amax = _blocks(w.float()).abs().amax(2)
    s = torch.exp2(E.float())
    free = (amax > 0) & (E > -13) & (E < 13)
    assert bool(free.any())
    assert bool(((3 * s < amax) & (amax <= 6 * s))[free].all())
    assert bool((E[amax == 0] == 0).all()) and bool((amax[7] == 0).all())
    d = quant.dequantize_blocks_mxfp4(q, e)
    ratio = _blocks(d).abs() / s[:, :, None]
    assert bool((ratio[..., None] == GRID).any(-1).all()), "a de-quantised value is off the e2m1 grid"
    # nearest grid value (no block here saturates: amax <= 6 * 2^E)
    t = (_blocks(w.float()) / s[:, :, None])[free]
    err = (t.abs()[..., None] - GRID).abs()
    assert bool(((_blocks(d) / s[:, :, None])[free].abs() - t.abs()).abs().le(err.amin(-1)).all())
    assert torch.equal(torch.signbit(d), torch.signbit(w.float())), "the sign of w is kept, zero magnitudes included"
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(quant.dequantize_blocks_mxfp4(q, e, dt).float(), d), f"a de-quantised value is not a {dt} value"
    h = d.to(torch.float16)
    assert bool((h[h != 0].abs() >= 2.0 ** -14).all()), "a non-zero de-quantised value is an fp16 subnormal"
    q2, e2 = quant.quantize_blocks_mxfp4(d.to(dtype))
    assert torch.equal(quant.dequantize_blocks_mxfp4(q2, e2), d)
    top = torch.maximum(q & 7, (q >> 4) & 7).view(200, -1, 16).amax(2)           # the block's largest magnitude code
    edge = (top == 5) & (E > -13)                                               # code 5 = 3.0
    same = (e2 == e) & (q2 == q).view(200, -1, 16).all(2)
    assert bool(same[~edge & (amax > 0) & (top > 0)].all())
    assert bool((e2[edge] == e[edge] - 1).all())


def test_tie_table_saturation_and_signs():
    from longspec_amd import quant
    v = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 0.0, -0.0, -0.25, 6.0, 7.0, -100.0, 5.01, -0.26, 0.5, 1.5, 3.0])
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 0.0, -0.0, -0.0, 6.0, 6.0, -6.0, 6.0, -0.5, 0.5, 1.5, 3.0]
    code = quant.e2m1_rne(v)
    got = torch.where(code >= 8, -GRID[(code & 7).long()], GRID[(code & 7).long()])
    assert torch.equal(got, torch.tensor(want)) and torch.equal(torch.signbit(got), torch.signbit(torch.tensor(want)))
    # the same table through the quantiser: a block whose amax is 6 has E = 0
    w = torch.zeros(1, 32)
    w[0, :18] = v
    w[0, 11], w[0, 12] = 6.0, -6.0
    q, e = quant.quantize_blocks_mxfp4(w)
    assert int(e[0, 0]) == 127
    d = quant.dequantize_blocks_mxfp4(q, e)
    want[11], want[12] = 6.0, -6.0
    assert torch.equal(d[0, :18], torch.tensor(want)) and torch.equal(torch.signbit(d[0, :18]), torch.signbit(torch.tensor(want)))


def test_zero_block_clamp_ends_and_nibble_order():
    from longspec_amd import quant
    w = torch.zeros(4, 64)
    w[1, :32] = torch.linspace(-1, 1, 32) * 2.0 ** -20            # far below the lower clamp: E = -13
    w[1, 32:] = torch.linspace(-1, 1, 32) * 6 * 2.0 ** -13        # amax = 6 * 2^-13: E = -13 exactly, unclamped value
    w[2, :32] = torch.linspace(-1, 1, 32) * 1e6                   # above the upper clamp: E = 13, saturates
    w[2, 32:] = torch.linspace(-1, 1, 32) * 6 * 2.0 ** 13
    w[3, 0], w[3, 1], w[3, 33] = 1.0, -6.0, 3.0
    q, e = quant.quantize_blocks_mxfp4(w)
    assert e.tolist() == [[127, 127], [114, 114], [140, 140], [127, 126]]
    assert bool((q[0] == 0).all())
    d = quant.dequantize_blocks_mxfp4(q, e)
    assert bool((d[1, :32] == 0).all()) and torch.equal(torch.signbit(d[1, :32]), torch.signbit(w[1, :32]))
    assert float(d[1, 63]) == 6 * 2.0 ** -13 and float(d[1, 32]) == -6 * 2.0 ** -13
    assert float(d[2, 0]) == -6 * 2.0 ** 13 and float(d[2, 31]) == 6 * 2.0 ** 13 and float(d[2, 63]) == 6 * 2.0 ** 13
    assert bool((d[2].abs() <= 6 * 2.0 ** 13).all())
    # lower k in the low nibble: (1.0 -> code 2, -6.0 -> code 15) share byte 0; 3.0 at k = 33 with E = -1 is code 7, high nibble
    assert int(q[3, 0]) == (2 | (15 << 4)) and int(q[3, 16]) == (7 << 4)
    assert torch.equal(d[3], w[3])
    with pytest.raises(ValueError):
        quant.quantize_blocks_mxfp4(torch.zeros(4, 48))
    with pytest.raises(ValueError):
        quant.dequantize_blocks_mxfp4(q, e[:, :1])


def _toy(run):
    from longspec_amd.llama_glide import LlamaGlide
    m = LlamaGlide(run["cfg"], ops=oracle_ops, dtype=torch.float16)
    m.load_state_dict({**run["target_sd"], **{"glide." + k: v for k, v in run["draft_sd"].items()}}, strict=True)
    return m


def _on_grid(w):
    from longspec_amd import quant
    q, e = quant.quantize_blocks_mxfp4(w)
    return torch.equal(quant.dequantize_blocks_mxfp4(q, e, w.dtype), w)


def test_decode_linear_quantize_weight_mxfp4_on_cpu():
    from longspec_amd.llama import DecodeLinear
    m = DecodeLinear(64, 32, bias=False, ops=oracle_ops)
    with torch.no_grad():
        m.weight.normal_(0, 0.03)
    before = m.weight.clone()
    assert not _on_grid(before)
    assert m.quantize_weight_("mxfp4") is m
    assert m.weight_quant == "mxfp4" and m._q4 is None and m._q8 is None            # on the CPU only .weight is rewritten
    assert _on_grid(m.weight) and not torch.equal(m.weight, before)
    x = torch.randn(3, 64)
    assert torch.equal(m(x), torch.nn.functional.linear(x, m.weight))
    f = DecodeLinear(64, 32, bias=False, ops=oracle_ops).quantize_weight_()
    assert f.weight_quant == "fp8"                                                   # the default is unchanged
    with pytest.raises(ValueError):
        m.quantize_weight_("int4")


@pytest.mark.parametrize("scope", ["all", "draft"])
def test_quantize_weights_mxfp4_scopes_on_cpu(scope):
    run = next(iter(cases.generate_runs()))
    m = _toy(run)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert m.quantize_weights_(scope, fmt="mxfp4") is m
    touched = 0
    for k, v in m.state_dict().items():
        proj = k.endswith("_proj.weight") or k == "lm_head.weight"
        if proj and (scope == "all" or k.startswith("glide.")):
            assert _on_grid(v) and not torch.equal(v, before[k]), k
            touched += 1
        else:
            assert torch.equal(v.view(torch.int16), before[k].view(torch.int16)), k
    assert touched > 0
    with pytest.raises(ValueError):
        m.quantize_weights_("all", fmt="int4")


def test_env_values(monkeypatch):
    from longspec_amd.llama import DecodeLinear, WEIGHT_QUANT_ENV
    from longspec_amd.llama_glide import DRAFT_HEAD_ENV
    run = next(iter(cases.generate_runs()))
    monkeypatch.setenv(WEIGHT_QUANT_ENV, "fp4-draft")
    t, d = DecodeLinear(64, 32, bias=False, ops=oracle_ops), DecodeLinear(64, 32, bias=False, ops=oracle_ops)
    d.quant_scope = "draft"
    with torch.no_grad():
        t.weight.normal_(0, 0.03)
        d.weight.normal_(0, 0.03)
    x = torch.randn(3, 64)
    t(x), d(x)
    assert d.weight_quant == "mxfp4" and _on_grid(d.weight) and t.weight_quant is None and not _on_grid(t.weight)
    monkeypatch.setenv(WEIGHT_QUANT_ENV, "fp4")
    t2 = DecodeLinear(64, 32, bias=False, ops=oracle_ops)
    t2(x)
    assert t2.weight_quant == "mxfp4"
    monkeypatch.setenv(WEIGHT_QUANT_ENV, "fp2")
    with pytest.raises(ValueError):
        DecodeLinear(64, 32, ops=oracle_ops)
    monkeypatch.delenv(WEIGHT_QUANT_ENV)
    monkeypatch.setenv(DRAFT_HEAD_ENV, "int4")
    with pytest.raises(ValueError):
        _toy(run)
    monkeypatch.setenv(DRAFT_HEAD_ENV, "fp4")
    m = _toy(run)
    assert m.draft_lm_head is None                                  # built at the first draft pass
    head = m._head_of_draft_passes()
    assert head is m.draft_lm_head and head.weight_quant == "mxfp4" and _on_grid(head.weight)
    assert m._head_of_draft_passes() is head                               # ... once per lm_head weight version


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_draft_head_is_not_part_of_the_state_dict(fmt):
    from longspec_amd.llama import DecodeLinear
    run = next(iter(cases.generate_runs()))
    m = _toy(run)
    keys = list(m.state_dict().keys())
    n_params, n_modules = len(list(m.parameters())), len(list(m.modules()))
    lm = m.lm_head.weight.clone()
    assert m.quantize_draft_head_(fmt) is m
    assert list(m.state_dict().keys()) == keys
    assert len(list(m.parameters())) == n_params and len(list(m.modules())) == n_modules
    assert torch.equal(m.lm_head.weight, lm) and m.lm_head.weight_quant is None
    head = m.draft_lm_head
    assert isinstance(head, DecodeLinear) and head.weight_quant == fmt and head.weight.shape == lm.shape
    assert not torch.equal(head.weight, lm)
    # a 16-bit head assigned by hand stays out of the registered modules too; None restores the shared head
    plain = DecodeLinear(lm.shape[1], lm.shape[0], bias=False, ops=oracle_ops)
    m.draft_lm_head = plain
    assert list(m.state_dict().keys()) == keys and m._head_of_draft_passes() is plain
    m.draft_lm_head = None
    assert m._head_of_draft_passes() is m.lm_head
    with pytest.raises(ValueError):
        m.quantize_draft_head_("int4")


def test_draft_head_changes_the_draft_never_the_output_on_cpu():
    """Greedy tree and chain decoding stay lossless with a low-precision draft head: the tokens are vanilla decoding's."""
    run = next(iter(cases.generate_runs()))
    a, b = _toy(run).quantize_draft_head_("mxfp4"), _toy(run)
    ids, pl = run["prompt"], torch.tensor([run["prompt_len"]])
    kw = dict(max_gen_len=run["max_gen_len"], eos_id=run["eos_id"])
    va, vb = a.vanilla_generate(ids, pl, **kw), b.vanilla_generate(ids, pl, **kw)
    assert torch.equal(va[0], vb[0]) and va[1] == vb[1]
    ta = a.tree_spec_generate(ids, pl, tree_shape=run["tree_shape"], **kw)
    n = int(ta[1]) + int(ta[2])
    assert torch.equal(ta[0][0, :n], va[0][0, :n])
    sa = a.spec_generate(ids, pl, gamma=4, **kw)
    n = min(int(sa[1]) + int(sa[2]), run["max_gen_len"])
    assert torch.equal(sa[0][0, :n], va[0][0, :n])


def test_env_draft_head_is_built_inside_a_generation(monkeypatch):
    """The generate loops run under inference_mode; the head built there is an ordinary module whose weight version is tracked."""
    from longspec_amd.llama_glide import DRAFT_HEAD_ENV
    run = next(iter(cases.generate_runs()))
    ids, pl = run["prompt"], torch.tensor([run["prompt_len"]])
    kw = dict(max_gen_len=run["max_gen_len"], eos_id=run["eos_id"])
    want = _toy(run).quantize_draft_head_("mxfp4").tree_spec_generate(ids, pl, tree_shape=run["tree_shape"], **kw)
    monkeypatch.setenv(DRAFT_HEAD_ENV, "fp4")
    m = _toy(run)
    got = m.tree_spec_generate(ids, pl, tree_shape=run["tree_shape"], **kw)
    assert m.draft_lm_head is not None and m.draft_lm_head.weight_quant == "mxfp4" and m.lm_head.weight_quant is None
    assert torch.equal(got[0], want[0]) and (int(got[1]), int(got[2])) == (int(want[1]), int(want[2]))
    s = m.spec_generate(ids, pl, gamma=4, **kw)
    w = _toy(run).quantize_draft_head_("mxfp4")
    monkeypatch.delenv(DRAFT_HEAD_ENV)
    s2 = w.spec_generate(ids, pl, gamma=4, **kw)
    assert torch.equal(s[0], s2[0])


def test_draft_head_follows_the_model_through_to():
    """The unregistered head moves with ``model.to(...)``; at its next use the weight is on the new dtype's grid again."""
    run = next(iter(cases.generate_runs()))
    m = _toy(run).quantize_draft_head_("mxfp4")
    keys = list(m.state_dict().keys())
    want = m.draft_lm_head.weight.detach().clone()
    m.to(torch.bfloat16)
    head = m.draft_lm_head
    assert head.weight.dtype == torch.bfloat16 and m.lm_head.weight.dtype == torch.bfloat16
    assert list(m.state_dict().keys()) == keys
    assert torch.equal(head.weight.float(), want.float())           # e2m1 * 2^E is exact in both dtypes
    head(torch.randn(2, head.in_features, dtype=torch.bfloat16))
    assert head.weight_quant == "mxfp4" and _on_grid(head.weight) and torch.equal(head.weight.float(), want.float())
