"""FP8 (e4m3) weights, host side: the row-wise quantiser of longspec_amd/quant.py against a literal restatement, and
``quantize_weights_`` on a toy LlamaGlide driven by the oracle's operators (no GPU)."""
import pytest
import torch

import cases
import oracle_ops


def _mk(shape, seed, scale, dtype):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("K", [256, 4096])
@pytest.mark.parametrize("std", [0.03, None], ids=["std0.03", "stdK^-0.5"])
def test_quantize_rows_e4m3_definition(dtype, K, std):
    """Scales are exact powers of two with 224 s < amax <= 448 s, the bytes are torch's e4m3fn cast of w / s, zero rows get
    s = 1, the NaN encoding never appears, and q * s is exactly representable in fp16 and bf16.

    Quantising the de-quantised weight returns the same VALUES for every row, and the same (q, s) for every row except
    those whose largest byte is 224 = 448 / 2 (amax / s in (224, 232] rounds down to it): there the definition
    s = 2^ceil(log2(amax / 448)) itself moves one exponent from the scale into the bytes, (q, s) -> (2 q, s / 2) -- the
    bound 224 s < amax and (q, s)-idempotence cannot both hold on such a row.  About 5 % of random rows are of that kind;
    both outcomes are pinned below."""
    from longspec_amd import quant
    w = _mk((300, K), 5 + K, std if std is not None else K ** -0.5, dtype)
    w[7] = 0
    q, s = quant.quantize_rows_e4m3(w)
    assert q.dtype == torch.uint8 and q.shape == w.shape and s.dtype == torch.float32 and s.shape == (300,)
    amax = w.float().abs().amax(1)
    nz = amax > 0
    mant, _ = torch.frexp(s)
    assert bool((mant == 0.5).all()), "scales must be exact powers of two"
    assert bool(((224 * s < amax) & (amax <= 448 * s))[nz].all())
    assert bool((s[~nz] == 1).all()) and not bool(nz[7])
    want_q = (w.float() / s[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)      # no clamp needed: |w / s| <= 448
    assert torch.equal(q, want_q)
    assert not bool(((q & 0x7F) == 0x7F).any())
    d = quant.dequantize_rows_e4m3(q, s)
    assert torch.equal(d, want_q.view(torch.float8_e4m3fn).float() * s[:, None])
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(d.to(dt).float(), d), f"q * s is not a {dt} value"
    q2, s2 = quant.quantize_rows_e4m3(d.to(dtype))
    assert torch.equal(quant.dequantize_rows_e4m3(q2, s2), d)
    edge = (q & 0x7F).amax(1) == 0x76                            # 0x76 = 224: the row's largest magnitude
    same = (s2 == s) & (q2 == q).all(1)
    assert bool(same[~edge].all())
    assert bool((s2[edge] == s[edge] / 2).all())
    assert torch.equal(q2[edge].view(torch.float8_e4m3fn).float(), 2 * q[edge].view(torch.float8_e4m3fn).float())
    # a third pass is a fixed point in (q, s) too wherever the second did not hit the edge again
    q3, s3 = quant.quantize_rows_e4m3(quant.dequantize_rows_e4m3(q2, s2).to(dtype))
    assert torch.equal(q3, q2) and torch.equal(s3, s2)


def test_quantizer_saturates_and_general_scale():
    from longspec_amd import quant
    w = torch.tensor([[1.0, -0.5, 0.25, 0.0], [3.0, 3.0, -3.0, 1e-3]])
    q, s = quant.quantize_rows_e4m3(w, pow2=False)
    assert torch.equal(s, w.abs().amax(1) / 448.0)
    assert torch.equal(q, (w / s[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))
    assert int(q[0, 0]) == 0x7E and int(q[1, 2]) == 0xFE
    # what torch's cast alone would turn into NaN saturates here
    big = torch.tensor([[500.0, -1e9, 448.0, 464.0]])
    assert torch.equal((big.clamp(-448, 448)).to(torch.float8_e4m3fn).view(torch.uint8), torch.tensor([[0x7E, 0xFE, 0x7E, 0x7E]], dtype=torch.uint8))
    with pytest.raises(ValueError):
        quant.quantize_rows_e4m3(torch.zeros(8))


def _toy(run):
    from longspec_amd.llama_glide import LlamaGlide
    m = LlamaGlide(run["cfg"], ops=oracle_ops, dtype=torch.float16)
    m.load_state_dict({**run["target_sd"], **{"glide." + k: v for k, v in run["draft_sd"].items()}}, strict=True)
    return m


def _on_grid(w):
    from longspec_amd import quant
    q, s = quant.quantize_rows_e4m3(w)
    return torch.equal(quant.dequantize_rows_e4m3(q, s, w.dtype), w)


def _is_projection(name):
    return name.endswith("_proj.weight") or name == "lm_head.weight"


@pytest.mark.parametrize("scope", ["all", "draft", "target"])
def test_quantize_weights_scopes_on_cpu(scope):
    run = next(iter(cases.generate_runs()))
    m = _toy(run)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert m.quantize_weights_(scope) is m
    touched = 0
    for k, v in m.state_dict().items():
        draft = k.startswith("glide.")
        in_scope = _is_projection(k) and (scope == "all" or (scope == "draft") == draft)
        if in_scope:
            assert _on_grid(v), k
            assert not torch.equal(v, before[k]), k
            touched += 1
        else:
            assert torch.equal(v.view(torch.int16), before[k].view(torch.int16)), k          # bit for bit
    assert touched > 0
    if scope == "draft":
        assert all(k.startswith("glide.") for k, v in m.state_dict().items() if not torch.equal(v, before[k]))
    with pytest.raises(ValueError):
        m.quantize_weights_("everything")


def test_quantized_model_equals_its_state_dict_on_cpu():
    """Generation of the quantised model == generation of a fresh 16-bit model loaded from its state_dict."""
    run = next(iter(cases.generate_runs()))
    a = _toy(run).quantize_weights_("all")
    b = _toy(run)
    b.load_state_dict(a.state_dict(), strict=True)
    ids, pl = run["prompt"], torch.tensor([run["prompt_len"]])
    kw = dict(max_gen_len=run["max_gen_len"], eos_id=run["eos_id"])
    va, vb = a.vanilla_generate(ids, pl, **kw), b.vanilla_generate(ids, pl, **kw)
    assert torch.equal(va[0], vb[0]) and va[1] == vb[1]
    ta = a.tree_spec_generate(ids, pl, tree_shape=run["tree_shape"], **kw)
    tb = b.tree_spec_generate(ids, pl, tree_shape=run["tree_shape"], **kw)
    assert torch.equal(ta[0], tb[0]) and (int(ta[1]), int(ta[2])) == (int(tb[1]), int(tb[2]))


def test_env_default_quantizes_at_first_use(monkeypatch):
    from longspec_amd.llama import DecodeLinear, WEIGHT_QUANT_ENV
    monkeypatch.setenv(WEIGHT_QUANT_ENV, "fp8-draft")
    t, d = DecodeLinear(64, 32, bias=False, ops=oracle_ops), DecodeLinear(64, 32, bias=False, ops=oracle_ops)
    d.quant_scope = "draft"
    with torch.no_grad():                                   # filled in place after construction, as the benchmark does
        t.weight.normal_(0, 0.03)
        d.weight.normal_(0, 0.03)
    x = torch.randn(3, 64)
    t(x), d(x)
    assert d.weight_quant == "fp8" and _on_grid(d.weight) and t.weight_quant is None and not _on_grid(t.weight)
    monkeypatch.setenv(WEIGHT_QUANT_ENV, "int4")
    with pytest.raises(ValueError):
        DecodeLinear(64, 32, ops=oracle_ops)
