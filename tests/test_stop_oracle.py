"""The stop oracle (tests/stop_oracle.py) on hand-written cases, ``Stop``'s validation, its device table and the environment
string."""
import pytest
import torch

import stop_oracle as so
from longspec_amd import Stop
from longspec_amd import stop as stop_mod
from longspec_amd.logprobs import new_buffers


def test_a_token_id_at_column_0():
    assert so.scan([7, 1, 2], Stop(token_ids=[7])) == (1, 0, 0)
    assert so.cut([7, 1, 2, 9, 9], 3, Stop(token_ids=[7]), 5) == ([7, 5, 5, 9, 9], (1, 0, 0))


def test_a_sequence_never_reaches_in_front_of_column_0():
    # the prompt may end in 4: the text [5, ...] does not complete (4, 5) at column 0, a later 4 5 does
    stop = Stop(sequences=[(4, 5)])
    assert so.scan([5, 1, 2], stop) == (-1, -1, -1)
    assert so.scan([5, 4, 5], stop) == (3, 0, 1)
    assert so.scan([5], Stop(sequences=[(5, 5, 5)])) == (-1, -1, -1)          # longer than the text


def test_the_earliest_of_two_matches_wins():
    stop = Stop(token_ids=[9, 3])
    assert so.scan([1, 3, 9, 3], stop) == (2, 1, 1)                            # 3 at column 1 beats 9 at column 2
    assert so.scan([1, 2, 8, 8, 6], Stop(token_ids=[6], sequences=[(8, 8)])) == (4, 1, 2)


def test_which_is_the_first_stop_in_listing_order():
    text = [1, 2, 3]
    assert so.scan(text, Stop(token_ids=[3], sequences=[(2, 3), (3,)])) == (3, 0, 2)
    assert so.scan(text, Stop(sequences=[(2, 3), (3,), (1, 2, 3)])) == (3, 0, 1)
    assert so.scan(text, Stop(sequences=[(1, 2, 3), (3,)])) == (3, 0, 0)
    assert so.scan(text, Stop(token_ids=[8, 3], sequences=[(3,)])) == (3, 1, 2)


def test_min_tokens_boundaries():
    text = [1, 7, 7, 7]
    assert so.scan(text, Stop(token_ids=[7], min_tokens=1)) == (2, 0, 1)       # c = min
    assert so.scan(text, Stop(token_ids=[7], min_tokens=2)) == (3, 0, 2)       # c = min - 1 is ignored
    assert so.scan(text, Stop(token_ids=[7], min_tokens=4)) == (-1, -1, -1)
    # a sequence that ends in front of min_tokens is ignored and can match again; one that ends at min_tokens may begin in front
    assert so.scan([4, 5, 1, 4, 5], Stop(sequences=[(4, 5)], min_tokens=2)) == (5, 0, 3)
    assert so.scan([1, 4, 5], Stop(sequences=[(4, 5)], min_tokens=2)) == (3, 0, 1)


def _scan_rounds(rounds, stop, fill=0, top_n=2, width=12):
    """The operator over a text that arrives in ``rounds`` (lists of tokens): (output_ids, stop_state, flags per round, lp)."""
    out = torch.full((1, width), fill, dtype=torch.int64)
    lp = new_buffers(1, width, top_n, "cpu")
    state = stop_mod.new_state(1, "cpu")
    table = stop.table(100, "cpu")
    written = torch.zeros((1,), dtype=torch.int32)
    flags = []
    for r in rounds:
        n = len(r)
        out[0, int(written):int(written) + n] = torch.tensor(r)
        lp.token[0, int(written):int(written) + n] = 0.5
        lp.top[0, int(written):int(written) + n] = 0.25
        lp.top_ids[0, int(written):int(written) + n] = 3
        written += n
        rs = torch.tensor([[n, 1]])
        so.stop_scan(out, table, state, written, num=torch.tensor([n]), fill=fill, state=rs, logprobs=lp)
        flags.append(int(rs[0, 1]))
    return out, state, flags, lp


def test_a_sequence_completes_across_two_rounds():
    out, state, flags, lp = _scan_rounds([[1, 2, 4], [5, 6, 7], [8]], Stop(sequences=[(4, 5)]), fill=11)
    assert state[0].tolist() == [4, 0, 2, 0] and flags == [1, 3, 3]
    assert out[0].tolist() == [1, 2, 4, 5] + [11] * 8
    assert not torch.isnan(lp.token[0, :4]).any() and torch.isnan(lp.token[0, 4:]).all()
    assert (lp.top[0, 4:] == float("-inf")).all() and (lp.top_ids[0, 4:] == -1).all() and (lp.top_ids[0, :4] == 3).all()


def test_the_operator_only_scans_the_rounds_columns_and_a_stopped_row_only_erases():
    # column 1 holds a stop id, but the operator is told the round wrote the last column only: the caller's contract
    out = torch.tensor([[1, 7, 2, 0, 0]])
    state = stop_mod.new_state(1, "cpu")
    so.stop_scan(out, Stop(token_ids=[7]).table(100, "cpu"), state, torch.tensor([3], dtype=torch.int32), num_const=1)
    assert state[0].tolist() == [-1, -1, -1, 0] and out[0].tolist() == [1, 7, 2, 0, 0]
    so.stop_scan(out, Stop(token_ids=[7]).table(100, "cpu"), state, torch.tensor([3], dtype=torch.int32), num_const=2)
    assert state[0].tolist() == [2, 0, 1, 0] and out[0].tolist() == [1, 7, 0, 0, 0]
    out[0, 2:4] = torch.tensor([7, 7])
    so.stop_scan(out, Stop(token_ids=[7]).table(100, "cpu"), state, torch.tensor([4], dtype=torch.int32), num_const=2)
    assert state[0].tolist() == [2, 0, 1, 0] and out[0].tolist() == [1, 7, 0, 0, 0]


def test_the_ban():
    stop = Stop(token_ids=[2, 5], sequences=[(1,)], min_tokens=3)
    table = stop.table(8, "cpu")
    x = torch.arange(4 * 8, dtype=torch.float16).view(1, 4, 8).clone()
    want = x.clone()
    want[0, :2, 2] = want[0, :2, 5] = float("-inf")                            # rows 0, 1 predict columns 1, 2 < 3
    got = so.stop_ban_rows(x, table, base=torch.tensor([1], dtype=torch.int32), depth="row")
    assert got is x and torch.equal(x, want)
    y = torch.zeros((2, 8), dtype=torch.bfloat16)
    so.stop_ban_rows(y, table, base=torch.tensor([9, 4], dtype=torch.int32), base_sub=torch.tensor([7, 0], dtype=torch.int32))
    assert y[0].tolist() == [0, 0, float("-inf"), 0, 0, float("-inf"), 0, 0] and not y[1].any()
    mask = torch.zeros((1, 3, 3), dtype=torch.int64)
    mask[0, :, 0] = 1
    mask[0, 1, 1] = mask[0, 2, 1] = mask[0, 2, 2] = 1                          # depths 0, 1, 2
    z = torch.zeros((1, 3, 8), dtype=torch.float16)
    so.stop_ban_rows(z, table, base=torch.tensor([1], dtype=torch.int32), depth="tree", tree_mask=mask)
    assert torch.isinf(z[0, :2, 2]).all() and torch.isinf(z[0, :2, 5]).all() and not z[0, 2].any()


def test_stop_validation():
    s = Stop(token_ids=[1, 2], sequences=[[3, 4], (5,)], min_tokens=3)
    assert s.token_ids == (1, 2) and s.sequences == ((3, 4), (5,)) and s.min_tokens == 3
    assert s == Stop((1, 2), ((3, 4), (5,)), 3) != Stop((1, 2), ((3, 4), (5,))) and hash(s) == hash(Stop((1, 2), ((3, 4), (5,)), 3))
    assert [s.stop_len(i) for i in range(4)] == [1, 1, 2, 1]
    Stop(token_ids=range(64))
    Stop(sequences=[list(range(16))] * 16)
    for kw in (dict(), dict(token_ids=[1, 1]), dict(token_ids=range(65)), dict(sequences=[[]]), dict(sequences=[list(range(17))]),
               dict(sequences=[[1]] * 17), dict(token_ids=[-1]), dict(token_ids=[2 ** 31]), dict(sequences=[[1, -2]]),
               dict(token_ids=[1], min_tokens=-1)):
        with pytest.raises(ValueError):
            Stop(**kw)
    for kw in (dict(token_ids=[1.5]), dict(token_ids=[True]), dict(token_ids="12"), dict(token_ids=5), dict(sequences=[3]),
               dict(sequences=["ab"]), dict(sequences=[[1, "2"]]), dict(token_ids=[1], min_tokens=1.0), dict(token_ids=[1], min_tokens=True)):
        with pytest.raises(TypeError):
            Stop(**kw)
    with pytest.raises(ValueError, match="700"):
        Stop(token_ids=[700]).table(512, "cpu")
    with pytest.raises(ValueError, match="512"):
        Stop(token_ids=[1], sequences=[[3, 512]]).table(512, "cpu")


def test_the_table_round_trips():
    for s in (Stop(token_ids=[1, 2], sequences=[[3, 4], (5,)], min_tokens=3), Stop(token_ids=range(64)),
              Stop(sequences=[list(range(q, q + 16)) for q in range(16)], min_tokens=2 ** 31 - 1)):
        t = s.table(1000, "cpu")
        assert t.dtype == torch.int32 and tuple(t.shape) == (stop_mod.TABLE_WORDS,) and stop_mod.TABLE_WORDS == 341
        assert so.stop_of_table(t) == s


def test_the_environment_string(monkeypatch):
    monkeypatch.delenv(stop_mod.STOP_ENV, raising=False)
    assert stop_mod.env_stop() is None and stop_mod.resolve(None, None, True) is None
    monkeypatch.setenv(stop_mod.STOP_ENV, "ids=128001+128009,seq=13+13|198+198+198,min=8")
    want = Stop([128001, 128009], [[13, 13], [198, 198, 198]], 8)
    assert stop_mod.env_stop() == want == stop_mod.resolve(None, None, True) == stop_mod.resolve(None, 0.0, True)
    assert stop_mod.resolve(None, 0.5, True) is None and stop_mod.resolve(None, None, False) is None
    assert stop_mod.resolve(Stop([1]), None, True) == Stop([1])                # the argument wins
    assert Stop.parse(" min=2 , ids=7") == Stop([7], min_tokens=2) and Stop.parse("seq=1") == Stop(sequences=[[1]])
    for bad in ("7", "ids", "ids=", "ids=a", "ids=1+", "ids=1,ids=2", "seq=1||2", "min=3", "min=1+2,ids=1", "ids=1,min=x", "ids=1,k=2",
                "ids=1+1", "ids=1;seq=2", "ids=1,min=-1"):
        monkeypatch.setenv(stop_mod.STOP_ENV, bad)
        with pytest.raises(ValueError):
            stop_mod.env_stop()
    with pytest.raises(TypeError):
        stop_mod.resolve([1], None, True)
    with pytest.raises(ValueError, match="temperature"):
        stop_mod.resolve(Stop([1]), 0.5, True)
