"""ls_logprob_topk_store (ops.logprob_topk(..., logp_out=)): the top-k launches also write the rows' fp32 log-probs, the
draft's ``spec_logits[:, lo:mid] = current_logp`` of the temperature > 0 rounds (llama_glide.py:1025,1074).

The stored log-probs are checked against a float64 ``log_softmax`` of the same logits on the CPU.  The bound is not a constant:
torch's own ``logits.float().log_softmax(-1)`` on the GPU -- the expression the store replaces -- is another fp32 evaluation of
the same formula that differs in summation order only, so the store may be at most TWICE as far from the float64 truth as
torch is on the same inputs (both figures are printed)."""
import pytest
import torch

from conftest import record_margin

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
LO = 1                     # the rows go to spec_logits[:, LO:LO + rows]; row 0 and the two rows behind them must stay untouched


def _logits(rows, V, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, rows, V, generator=g) * 3.0).to(dtype)


def _check(logits, k):
    """Both history variants on one set of logits; returns (largest error of the store, of torch's fp32 log_softmax)."""
    from longspec_amd import ops
    _, rows, V = logits.shape
    truth = logits[0].double().log_softmax(-1)                                 # CPU, float64
    x = logits.cuda()
    torch_err = (x.float().log_softmax(-1)[0].cpu().double() - truth).abs().max().item()
    hist = torch.linspace(-3.0, -0.25, rows, dtype=torch.float32)[None].cuda()
    worst = 0.0
    for history in (None, hist):
        want_v, want_i = ops.logprob_topk(x, history, k)
        spec = torch.full((1, LO + rows + 2, V), SENTINEL, dtype=torch.float32, device="cuda")
        got_v, got_i = ops.logprob_topk(x, history, k, logp_out=spec[:, LO:LO + rows])
        assert torch.equal(got_v, want_v) and torch.equal(got_i, want_i), "the store changed the top-k"
        spec = spec.cpu()
        assert bool((spec[:, :LO] == SENTINEL).all()) and bool((spec[:, LO + rows:] == SENTINEL).all()), "rows outside [lo, mid) touched"
        lp = spec[0, LO:LO + rows]
        assert bool(torch.isfinite(lp).all())
        worst = max(worst, (lp.double() - truth).abs().max().item())
        # a top-k value IS the stored log-prob of its column (+ history), bit for bit: one pair of row statistics
        r, c = (got_i[0].cpu() // V), (got_i[0].cpu() % V)
        picked = lp[r, c] if history is None else lp[r, c] + history[0].cpu()[r]
        assert torch.equal(picked, got_v[0].cpu())
    return worst, torch_err


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("V", [8, 8200, 32000, 152064])
@pytest.mark.parametrize("rows", [1, 4, 16])
def test_logp_store(rows, V, dtype):
    k = 4 if rows * V < 64 else 16
    err, torch_err = _check(_logits(rows, V, dtype, 1000 * rows + V % 977), k)
    print(f"logp store rows={rows} V={V} {dtype}: max |err| vs float64 {err:.3e}; torch fp32 log_softmax {torch_err:.3e}; "
          f"bound {2 * torch_err:.3e}")
    record_margin(f"logp_store rows={rows} V={V}", err, err, 2 * torch_err)
    assert err <= 2 * torch_err


def test_logp_store_survives_logits_near_the_fp16_limits():
    """One row with a single logit at +60 000 and all others at -60 000: every exp but one underflows to zero; the stored
    log-probs are finite (0 and -120 000), no NaN."""
    rows, V = 4, 8200
    logits = _logits(rows, V, torch.float16, 77)
    logits[0, 2, :] = -60000.0
    logits[0, 2, 4321] = 60000.0
    err, torch_err = _check(logits, 16)
    print(f"logp store, extreme row: max |err| vs float64 {err:.3e}; torch fp32 log_softmax {torch_err:.3e}; bound {2 * torch_err:.3e}")
    assert err <= 2 * torch_err


def test_logp_out_is_validated():
    from longspec_amd import ops
    x = _logits(2, 64, torch.float16, 5).cuda()
    with pytest.raises(TypeError):
        ops.logprob_topk(x, None, 4, logp_out=torch.zeros((1, 2, 64), dtype=torch.float16, device="cuda"))
    with pytest.raises(TypeError):
        ops.logprob_topk(x, None, 4, logp_out=torch.zeros((1, 3, 64), dtype=torch.float32, device="cuda"))
