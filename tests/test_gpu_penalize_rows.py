"""``ops.penalize_rows`` (csrc/penalty.hip) against tests/penalty_oracle.py, bit for bit: every step of the formula is one IEEE
fp32 operation in a fixed order, so the 16-bit outputs are compared as int16 patterns.  The case table is
tests/penalty_cases.py; the two tests without the ``gpu`` mark check the table itself on the CPU."""
import math

import pytest
import torch

import penalty_cases as pc
import penalty_oracle as po
from longspec_amd import Penalties

gpu = pytest.mark.gpu
_EXPECTED = {}


def expected(case):
    """The oracle's output of a case, computed once and shared."""
    if case["name"] not in _EXPECTED:
        _EXPECTED[case["name"]] = po.penalize_rows(case["logits"], case["state"], case["pen"], case["extra_ids"], case["extra_mask"])
    return _EXPECTED[case["name"]]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _cuda(t):
    return None if t is None else t.cuda()


def _extras(case):
    """The extras on the device with the layout the case has on the CPU (a view stays a view)."""
    ids, mask = case["extra_ids"], case["extra_mask"]
    if ids is None:
        return None, None
    if mask.dim() == 3 and mask.stride(1) == mask.shape[2] + 1:    # all_spec[:, 1:] / tree_mask[:, :, 1:]
        full_ids = torch.zeros((ids.shape[0], ids.shape[1] + 1), dtype=torch.int64)
        full_ids[:, 1:] = ids
        full_mask = torch.ones((mask.shape[0], mask.shape[1], mask.shape[2] + 1), dtype=torch.int64)
        full_mask[:, :, 1:] = mask
        return full_ids.cuda()[:, 1:], full_mask.cuda()[:, :, 1:]
    return ids.cuda(), mask.cuda()


def run(case, padded=False):
    from longspec_amd import ops
    x = case["logits"]
    if padded:                                                 # row stride V + 24, the padding poisoned
        buf = torch.full((*x.shape[:2], x.shape[2] + 24), 3.0e4, dtype=x.dtype)
        buf[:, :, :x.shape[2]] = x
        x_dev = buf.cuda()[:, :, :x.shape[2]]
    else:
        x_dev = x.cuda()
    before = x_dev.clone()
    ids, mask = _extras(case)
    out = ops.penalize_rows(x_dev, case["state"].cuda(), case["pen"], ids, mask)
    assert out.is_contiguous() and out.data_ptr() != x_dev.data_ptr() and torch.equal(bits(x_dev), bits(before))
    return out


CASES = pc.cases()


def test_the_case_table_holds_what_it_promises():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    tree = next(c for c in CASES if c["name"].startswith("tree-"))
    V = tree["logits"].shape[-1]
    ids, mask = tree["extra_ids"][0], tree["extra_mask"][0]
    assert tree["logits"].shape[1] == 69 and tree["extra_ids"].storage_offset() == 1 and tree["extra_mask"].stride(1) == 69
    for col in (0, 7, 8, 8191, 8192, V - 1, V + 3, -1):
        assert bool((ids == col).any()), col
    for oov in (V + 3, -1):                                    # under a set mask and under a zero mask
        c = int((ids == oov).nonzero()[0])
        assert bool((mask[:, c] != 0).any()) and bool((mask[:, c] == 0).any())
    leaf = mask[-1]
    on_path = ids[leaf != 0].tolist()
    assert sorted(on_path) == [7, 8, 8191, 8191, 8192]
    state = tree["state"][0]
    assert state[7] > 0 and state[8] < 0 and (state[8] & 0x7FFFFFFF) == 0 and state[8191] == 0
    chain = next(c for c in CASES if c["name"].startswith("chain-"))
    assert chain["extra_mask"].dim() == 2 and chain["logits"].shape[0] == 3


@pytest.mark.parametrize("mutant", po.MUTANTS)
def test_every_wrong_variant_changes_some_case(mutant):
    """No GPU: a wrong oracle is told from the right one by the table, so a kernel with that fault would be too."""
    hit = []
    for case in CASES:
        if case["logits"].shape[-1] > 8200 or case["logits"].shape[1] > 5 and not case["name"].startswith("tree-"):
            continue                                            # (the small cases already tell every variant apart)
        wrong = po.penalize_rows(case["logits"], case["state"], case["pen"], case["extra_ids"], case["extra_mask"], mutant=mutant)
        if not torch.equal(bits(wrong), bits(expected(case))):
            hit.append(case["name"])
    assert hit, f"no case tells the variant {mutant!r} from the formula"
    if mutant in ("no_extras", "dup_once", "other_row_mask"):
        assert any(n.startswith("tree-") for n in hit), hit


@gpu
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernel_matches_the_oracle_bit_for_bit(case):
    want = bits(expected(case))
    for padded in (False, True):
        got = bits(run(case, padded))
        bad = (got != want).nonzero()
        assert bad.numel() == 0, (case["name"], padded, bad[:4].tolist(), got[got != want][:4].tolist(), want[got != want][:4].tolist())


@gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_default_parameters_change_nothing(dtype):
    case = next(c for c in CASES if c["name"] == f"none-{dtype}")
    assert torch.equal(bits(run(case)), bits(case["logits"]))
    special = next(c for c in CASES if c["name"] == f"special-none-{dtype}")
    assert torch.equal(bits(run(special)), bits(special["logits"]))


@gpu
@pytest.mark.parametrize("name", ["b3-V1032-R5", "b3-V8200-R69", "chain"])
def test_each_batch_row_equals_its_own_launch(name):
    case = next(c for c in CASES if c["name"] == f"{name}-{torch.float16}")
    whole = bits(run(case))
    for z in range(case["logits"].shape[0]):
        mask = case["extra_mask"]
        one = dict(case, logits=case["logits"][z:z + 1], state=case["state"][z:z + 1], extra_ids=case["extra_ids"][z:z + 1],
                   extra_mask=mask if mask.dim() == 2 else mask[z:z + 1])
        assert torch.equal(bits(run(one)), whole[z:z + 1]), z


@gpu
def test_a_row_alone_among_others_and_reversed():
    """A row's output depends on that row, its extras and the scalars only."""
    case = next(c for c in CASES if c["name"] == f"tree-{torch.float16}")
    whole = bits(run(case))
    R = case["logits"].shape[1]
    rev = torch.arange(R - 1, -1, -1)
    flipped = dict(case, logits=case["logits"][:, rev].contiguous(), extra_mask=case["extra_mask"][:, rev].contiguous())
    assert torch.equal(bits(run(flipped))[:, rev], whole)
    for r in (0, 5, R - 1):
        alone = dict(case, logits=case["logits"][:, r:r + 1].contiguous(), extra_mask=case["extra_mask"][:, r:r + 1].contiguous())
        assert torch.equal(bits(run(alone)), whole[:, r:r + 1]), r


def _raw(x, o, st, pen, i=None, m=None, bs=None, **over):
    """``ls_penalize_rows`` itself; `over` replaces single arguments."""
    from longspec_amd import _C, ops
    b, R, V = x.shape
    a = dict(logits=x.data_ptr(), out=o.data_ptr(), b=b, rows=R, vocab=V, dtype=ops._dtype(x), isb=x.stride(0), isr=x.stride(1),
             osb=o.stride(0), osr=o.stride(1), state=st.data_ptr(), ssb=st.stride(0),
             ids=i.data_ptr() if i is not None else None, idsb=i.stride(0) if i is not None else 0,
             mask=m.data_ptr() if m is not None else None, msb=m.stride(0) if m is not None else 0,
             msr=m.stride(1) if m is not None else 0, C=i.shape[1] if i is not None else 0, rep=pen.repetition,
             pres=pen.presence, freq=pen.frequency, bias=bs.data_ptr() if bs is not None else None)
    a.update(over)
    return _C.load().ls_penalize_rows(*a.values(), ops._stream())


@gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("name", ["tree", "bias-all", "special-all"])
def test_in_place_and_strided_output(name, dtype):
    """``out == logits`` and an ``out`` of its own with padded rows (the padding is left alone) give the same bits."""
    case = next(c for c in CASES if c["name"] == f"{name}-{dtype}")
    want = bits(expected(case))
    x = case["logits"]
    b, R, V = x.shape
    ids, mask = _extras(case)
    state = case["state"].cuda()
    bias = case["pen"].bias_table(V, "cuda")
    buf = torch.full((b, R, V + 24), 32768.0, dtype=x.dtype)
    buf[:, :, :V] = x
    buf = buf.cuda()
    view = buf[:, :, :V]
    assert _raw(view, view, state, case["pen"], ids, mask, bias) == 0
    assert torch.equal(bits(view), want) and bool((buf[:, :, V:] == 32768.0).all())
    out = torch.full((b, R, V + 8), -7.0, dtype=x.dtype, device="cuda")
    assert _raw(x.cuda(), out[:, :, :V], state, case["pen"], ids, mask, bias) == 0
    assert torch.equal(bits(out[:, :, :V]), want) and bool((out[:, :, V:] == -7.0).all())


@gpu
def test_host_checks_refuse_before_any_launch():
    from longspec_amd import _C
    V, R = 1032, 3
    x = torch.zeros((1, R, V), dtype=torch.float16, device="cuda")
    wide = torch.zeros((1, R, V + 16), dtype=torch.float16, device="cuda")
    out = torch.full_like(x, 5.0)
    state = torch.zeros((1, V + 8), dtype=torch.int32, device="cuda")
    bias = torch.zeros((V + 8,), dtype=torch.float32, device="cuda")
    ids = torch.zeros((1, 8), dtype=torch.int64, device="cuda")
    mask = torch.ones((1, R, 8), dtype=torch.int64, device="cuda")
    pen = Penalties(1.3, 0.5, 0.25)
    assert _raw(x, out, state, pen, ids, mask, bias) == 0
    out.fill_(5.0)
    bad = [dict(vocab=V - 4), dict(isr=V + 4), dict(osr=V + 4), dict(isb=R * V + 4), dict(osb=R * V + 4), dict(ssb=V + 4),
           dict(isr=V - 8), dict(logits=wide.data_ptr() + 2, isr=V + 16), dict(out=out.data_ptr() + 8), dict(state=state.data_ptr() + 4),
           dict(bias=bias.data_ptr() + 4), dict(rep=0.0), dict(rep=-1.0), dict(rep=math.nan), dict(C=-1), dict(C=1025),
           dict(ids=None), dict(mask=None), dict(dtype=7), dict(rows=0), dict(b=0)]
    for over in bad:
        assert _raw(x, out, state, pen, ids, mask, bias, **over) == _C.LS_ERR_INVALID_ARG, over
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()), "a refused call launched"
    assert _raw(x, out, state, pen, None, None, None, C=0) == 0                     # C = 0: no extras, NULL pointers
    with pytest.raises(RuntimeError, match="GPU only"):
        from longspec_amd import ops
        ops.penalize_rows(x.cpu(), state.cpu()[:, :V], pen)
