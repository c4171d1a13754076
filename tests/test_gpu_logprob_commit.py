"""``ops.logprob_commit`` (csrc/logprob.hip) against the exact oracle of tests/logprob_oracle.py, bit for bit: the accepted
count below and at the row bound and read with a stride, a map with -1 padding and a repeated source, destinations running
past the buffer, and no map."""
import pytest
import torch

import logprob_oracle as lo
from longspec_amd.logprobs import new_buffers

pytestmark = pytest.mark.gpu


def rows_of(b, R, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((b, R), generator=g), torch.randn((b, R, n), generator=g), torch.randint(0, 1000, (b, R, n), generator=g))


def both(rows, W, base, base_add=0, num=None, index_map=None):
    """(device buffers on the CPU, oracle buffers) of one commit into freshly filled buffers."""
    from longspec_amd import ops
    b, n = rows[0].shape[0], rows[1].shape[2]
    dev, want = new_buffers(b, W, n, "cuda"), new_buffers(b, W, n, "cpu")
    cu = lambda t: t if t is None or t.is_cuda else t.cuda()          # a device view keeps its strides
    ops.logprob_commit(tuple(t.cuda() for t in rows), dev, base.cuda(), base_add, cu(num), cu(index_map))
    torch.cuda.synchronize()
    lo.logprob_commit(rows, want, base, base_add, None if num is None else num.cpu(), index_map)
    return dev, want


def same(dev, want):
    for name in ("token", "top", "top_ids"):
        g, w = getattr(dev, name).cpu(), getattr(want, name)
        if g.dtype == torch.float32:
            g, w = g.view(torch.int32), w.view(torch.int32)
        assert torch.equal(g, w), name


@pytest.mark.parametrize("n", [0, 5, 20])
def test_map_with_padding_and_a_repeated_source(n):
    rows = rows_of(2, 69, n)
    imap = torch.tensor([[68, 3, 3, -1, -1, -1], [0, 17, 40, 41, 68, 2]])
    for num in ([3, 6], [2, 5], [0, 1], [6, 6]):                       # below and equal to max_rows; row 0 may reach its -1s
        dev, want = both(rows, 64, torch.tensor([1, 30], dtype=torch.int32), num=torch.tensor(num), index_map=imap)
        same(dev, want)
    assert torch.isnan(dev.token[0, 4:]).all() and not torch.isnan(dev.token[0, 1:4]).any()


def test_num_read_with_stride_two_and_no_map():
    rows = rows_of(2, 5, 3, seed=1)
    state = torch.tensor([[2, 4], [5, 1]]).cuda()                       # a chain commit's state, on the device
    num = state[:, 0]                                                   # ... and its column 0: a view with stride 2
    assert num.is_cuda and num.stride(0) == 2 and num.data_ptr() == state.data_ptr()
    dev, want = both(rows, 16, torch.tensor([0, 7], dtype=torch.int32), base_add=1, num=num)
    same(dev, want)
    assert not torch.isnan(dev.token[0, 1:3]).any() and torch.isnan(dev.token[0, 3:]).all() and torch.isnan(dev.token[:, 0]).all()
    # batch row 1 took num[1 * 2] = 5 rows: a kernel that read num[1] = 4 (the state's other column) would leave column 12
    assert not torch.isnan(dev.token[1, 8:13]).any() and torch.isnan(dev.token[1, 13:]).all()
    dev, want = both(rows, 16, torch.tensor([3, 0], dtype=torch.int32))          # num = None: every row
    same(dev, want)
    assert not torch.isnan(dev.token[0, 3:8]).any()


def test_destinations_past_the_buffer_are_left_alone():
    rows = rows_of(2, 6, 4, seed=2)
    imap = torch.arange(6).repeat(2, 1)
    dev, want = both(rows, 8, torch.tensor([5, -2], dtype=torch.int32), num=torch.tensor([6, 6]), index_map=imap)
    same(dev, want)
    assert not torch.isnan(dev.token[0, 5:]).any() and torch.isnan(dev.token[0, :5]).all()
    assert not torch.isnan(dev.token[1, :4]).any() and torch.isnan(dev.token[1, 4:]).all()
    dev, want = both(rows, 8, torch.tensor([8, 100], dtype=torch.int32), base_add=1)
    same(dev, want)
    assert torch.isnan(dev.token).all()
