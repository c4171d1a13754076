"""``ops.token_state_add`` (csrc/penalty.hip) against the numpy oracle of tests/penalty_oracle.py, exactly: counts in bits 0-30,
the prompt flag in bit 31, ids outside the vocabulary ignored."""
import numpy as np
import pytest
import torch

import penalty_oracle as po

pytestmark = pytest.mark.gpu
V = 1032


def _apply(state, ids, num=None, prompt=False):
    """(device result, oracle result) of one call on a copy of `state` (numpy int32 [b, V])."""
    from longspec_amd import ops
    dev = torch.from_numpy(state.copy()).cuda()
    ops.token_state_add(dev, ids.cuda(), None if num is None else num.cuda(), prompt=prompt)
    want = po.token_state_add_np(state, ids.numpy(), None if num is None else num.numpy(), prompt)
    return dev.cpu().numpy(), want


def _start(b=1, seed=0):
    rng = np.random.RandomState(seed)
    word = rng.randint(0, 4, size=(b, V)).astype(np.uint32)
    word |= (rng.rand(b, V) < 0.3).astype(np.uint32) << np.uint32(31)
    return word.view(np.int32)


def test_duplicates_inside_one_call():
    ids = torch.tensor([[5, 5, 5, 9, 1031, 0, 0]], dtype=torch.int64)
    state = np.zeros((1, V), dtype=np.int32)
    got, want = _apply(state, ids)
    assert np.array_equal(got, want)
    assert (got[0, 5], got[0, 9], got[0, 1031], got[0, 0], int(got.sum())) == (3, 1, 1, 2, 7)


def test_num_cuts_the_row():
    ids = torch.tensor([[3, 4, 5, 6], [3, 4, 5, 6], [3, 4, 5, 6]], dtype=torch.int64)
    for num in ([0, 2, 4], [1, 1, 1], [4, 9, 3]):
        got, want = _apply(_start(3, 1), ids, torch.tensor(num, dtype=torch.int64))
        assert np.array_equal(got, want), num
    pair = torch.tensor([[2, 0], [3, 1], [1, 5]], dtype=torch.int64)           # a strided num: column 0 of a commit's state
    got, want = _apply(_start(3, 1), ids, pair[:, 0])
    assert np.array_equal(got, want)


def test_ids_outside_the_vocabulary_are_ignored():
    ids = torch.tensor([[-1, V, V + 7, 1 << 40, -(1 << 40), 17]], dtype=torch.int64)
    for prompt in (False, True):
        start = _start(1, 2)
        got, want = _apply(start, ids, prompt=prompt)
        assert np.array_equal(got, want)
        changed = (got != start).nonzero()[1].tolist()
        assert changed in ([17], [])                                           # (the flag of 17 may have been set already)


def test_prompt_mode_sets_bit_31_only_and_is_idempotent():
    from longspec_amd import ops
    start = _start(1, 3)
    ids = torch.tensor([[7, 7, 8, 500, 1031]], dtype=torch.int64)
    got, want = _apply(start, ids, prompt=True)
    assert np.array_equal(got, want)
    assert np.array_equal(got.view(np.uint32) & 0x7FFFFFFF, start.view(np.uint32) & 0x7FFFFFFF), "a count changed"
    assert all(got[0, c] < 0 for c in (7, 8, 500, 1031))
    dev = torch.from_numpy(got.copy()).cuda()
    ops.token_state_add(dev, ids.cuda(), prompt=True)
    assert np.array_equal(dev.cpu().numpy(), got)


def test_count_mode_never_touches_bit_31():
    start = _start(1, 4)
    ids = torch.from_numpy(np.random.RandomState(5).randint(0, V, size=(1, 300)))
    got, want = _apply(start, ids)
    assert np.array_equal(got, want)
    assert np.array_equal(got.view(np.uint32) >> 31, start.view(np.uint32) >> 31)


@pytest.mark.parametrize("n", [1, 5000])
def test_one_id_and_five_thousand_with_repeats(n):
    ids = torch.from_numpy(np.random.RandomState(n).randint(0, 40, size=(1, n)))
    got, want = _apply(np.zeros((1, V), dtype=np.int32), ids)
    assert np.array_equal(got, want) and int(got.sum()) == n


def test_three_batch_rows_are_independent():
    rng = np.random.RandomState(6)
    ids = torch.from_numpy(rng.randint(-3, V + 3, size=(3, 64)))
    num = torch.tensor([64, 0, 17], dtype=torch.int64)
    start = _start(3, 7)
    got, want = _apply(start, ids, num)
    assert np.array_equal(got, want) and np.array_equal(got[1], start[1])
    wide = torch.from_numpy(rng.randint(0, V, size=(3, 80)))                   # a column slice: row stride 80, 64 ids
    got, want = _apply(start, wide[:, 8:72], num)
    assert np.array_equal(got, want)
