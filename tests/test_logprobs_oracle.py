"""tests/logprob_oracle.py against ``torch.log_softmax`` in float64 and its own definition: ties, -inf, the padding of short
lists, and the commit with -1 map entries and destinations out of range."""
import math

import numpy as np
import torch

import logprob_oracle as lo
from longspec_amd.logprobs import new_buffers


def test_values_are_the_float64_log_softmax_of_the_tempered_row():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn((2, 3, 64), generator=g) * 4).to(torch.float16)
    ids = torch.randint(0, 64, (2, 3), generator=g)
    for T in (1.0, 0.6, 2.0):
        row_lp, top_val, top_idx = lo.token_logprobs64(x, ids, T, 5)
        ref = torch.log_softmax(x.double() / float(np.float32(T)), dim=-1)
        assert np.allclose(row_lp, ref.gather(-1, ids[..., None])[..., 0].numpy(), rtol=0, atol=1e-12)
        assert np.allclose(top_val, ref.gather(-1, torch.from_numpy(top_idx)).numpy(), rtol=0, atol=1e-12)
        want = torch.sort(x.float(), dim=-1, descending=True, stable=True).indices[..., :5]
        assert torch.equal(torch.from_numpy(top_idx), want)
        assert abs(np.exp(lo.row_logprobs64(x[0, 0], T)).sum() - 1) < 1e-12


def test_ties_go_to_the_smaller_column_and_the_zeros_are_equal():
    x = torch.tensor([[1.0, -0.0, 2.0, 0.0, 2.0, -0.0, 1.0, 0.0]], dtype=torch.float16)
    row_lp, top_val, top_idx = lo.token_logprobs64(x, torch.tensor([4]), 1.0, 8)
    assert top_idx[0, 0].tolist() == [2, 4, 0, 6, 1, 3, 5, 7]
    assert top_val[0, 0, 0] == top_val[0, 0, 1] == row_lp[0, 0] and len(set(top_val[0, 0, 4:].tolist())) == 1


def test_minus_inf_logits_and_ids_outside_the_vocabulary():
    x = torch.full((1, 2, 8), -math.inf, dtype=torch.float16)
    x[0, 0, 5] = 3.0
    x[0, 1, 2:4] = 1.0
    row_lp, top_val, top_idx = lo.token_logprobs64(x, torch.tensor([[5, 0]]), 0.6, 3)
    assert row_lp[0, 0] == 0.0 and row_lp[0, 1] == -math.inf
    assert top_idx[0, 0].tolist() == [5, 0, 1] and top_val[0, 0].tolist() == [0.0, -math.inf, -math.inf]
    assert top_idx[0, 1].tolist() == [2, 3, 0] and np.allclose(top_val[0, 1, :2], math.log(0.5))
    row_lp, _, top_idx = lo.token_logprobs64(x, torch.tensor([[8, -1]]), 1.0, 1)
    assert np.isnan(row_lp).all() and top_idx[0, :, 0].tolist() == [5, 2]


def test_a_list_longer_than_the_row_is_padded():
    x = torch.arange(8, dtype=torch.float16).view(1, 8)
    row_lp, top_val, top_idx = lo.token_logprobs(x, torch.tensor([7]), 1.0, 12)
    assert top_idx[0, 0].tolist() == [7, 6, 5, 4, 3, 2, 1, 0, -1, -1, -1, -1]
    assert (top_val[0, 0, 8:] == -math.inf).all() and top_val.dtype == torch.float32 and row_lp[0, 0] == top_val[0, 0, 0]
    row_lp, top_val, top_idx = lo.token_logprobs(x, torch.tensor([7]), 1.0, 0)
    assert top_val.shape == (1, 1, 0) == top_idx.shape and row_lp.shape == (1, 1)


def test_commit_skips_padding_and_columns_out_of_range():
    b, R, n, W = 2, 4, 2, 6
    rows = (torch.arange(b * R, dtype=torch.float32).view(b, R), torch.arange(b * R * n, dtype=torch.float32).view(b, R, n),
            torch.arange(b * R * n).view(b, R, n) + 100)
    out = new_buffers(b, W, n, "cpu")
    imap = torch.tensor([[2, 2, -1], [3, 0, 1]])
    lo.logprob_commit(rows, out, torch.tensor([1, 4], dtype=torch.int32), num=torch.tensor([3, 3]), index_map=imap)
    assert out.token[0, 1:3].tolist() == [2.0, 2.0] and torch.isnan(out.token[0, [0, 3, 4, 5]]).all()      # -1: skipped
    assert out.token[1, 4:].tolist() == [7.0, 4.0] and torch.isnan(out.token[1, :4]).all()                 # column 6: skipped
    assert out.top_ids[1, 5].tolist() == [108, 109] and out.top[0, 2].tolist() == [4.0, 5.0] and (out.top_ids[0, 3:] == -1).all()
    out = new_buffers(b, W, n, "cpu")
    lo.logprob_commit(rows, out, torch.tensor([0, 0], dtype=torch.int32), base_add=1, num=torch.tensor([[2, 9], [4, 9]])[:, 0])
    assert out.token[0, 1:3].tolist() == [0.0, 1.0] and torch.isnan(out.token[0, 3:]).all() and torch.isnan(out.token[:, 0]).all()
    assert out.token[1, 1:5].tolist() == [4.0, 5.0, 6.0, 7.0]
    out = new_buffers(b, W, n, "cpu")
    lo.logprob_commit(rows, out, torch.tensor([-1, 5], dtype=torch.int32))
    assert out.token[0, :3].tolist() == [1.0, 2.0, 3.0] and out.token[1, 5] == 4.0 and torch.isnan(out.token[1, :5]).all()
