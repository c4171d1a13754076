"""``ops.rope_apply_`` with a batch: a batched prefill hands it q / k of [b, R, heads, 128] and ONE table row per position
(``position_ids`` [1, R]), which ``apply_rotary_pos_emb`` broadcasts over the batch.  Every batch row must get the rotation
the same row gets alone -- the kernel reads a table row per (batch, position) and must not run past a [1, R, 128] table."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_one_table_row_per_position_is_broadcast_over_the_batch(dtype):
    from longspec_amd import ops
    b, R, Hq, Hk = 3, 260, 2, 1
    g = torch.Generator().manual_seed(3)
    q = torch.randn((b, R, Hq, 128), generator=g).to(dtype).cuda()
    k = torch.randn((b, R, Hk, 128), generator=g).to(dtype).cuda()
    inv_freq = (1.0 / (10000 ** (torch.arange(0, 128, 2).float() / 128))).cuda()
    cos, sin = ops.rope_cos_sin(torch.arange(R, device="cuda")[None], inv_freq, 1.0, dtype)
    assert cos.shape == (1, R, 128)
    want_q, want_k = q.clone(), k.clone()
    for z in range(b):
        ops.rope_apply_(want_q[z:z + 1], want_k[z:z + 1], cos, sin)
    got_q, got_k = q.clone(), k.clone()
    ops.rope_apply_(got_q, got_k, cos, sin)
    assert torch.equal(got_q, want_q) and torch.equal(got_k, want_k)
    assert not torch.equal(got_q, q)
    # a table with a row per (batch, position) is taken as it is
    full_q, full_k = q.clone(), k.clone()
    ops.rope_apply_(full_q, full_k, cos.expand(b, R, 128).contiguous(), sin.expand(b, R, 128).contiguous())
    assert torch.equal(full_q, want_q) and torch.equal(full_k, want_k)


def test_a_table_of_another_size_is_refused():
    from longspec_amd import ops
    q = torch.zeros((2, 8, 1, 128), dtype=torch.float16, device="cuda")
    k = torch.zeros((2, 8, 1, 128), dtype=torch.float16, device="cuda")
    for rows in (4, 12, 24):
        t = torch.zeros((1, rows, 128), dtype=torch.float16, device="cuda")
        with pytest.raises(ValueError, match="cos / sin"):
            ops.rope_apply_(q, k, t, t)
