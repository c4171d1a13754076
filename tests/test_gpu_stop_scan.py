"""``ops.stop_scan`` (``ls_stop_scan``) against the oracle (tests/stop_oracle.py), exact: texts that arrive in rounds of 1..7
columns, batch 1..3 with rows that stop in different rounds and are scanned again afterwards, 0 / 1 / 64 ids, no sequence / one
of length 1 / 16 of length 16, matches at column 0 and at the last column, a sequence longer than the written text, two
candidates in one round, ``min_tokens`` boundaries, the log-prob buffers with ``top_n`` 0 and 20, and guard elements in front
of, behind and between the rows of every buffer."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stop_oracle as so
from longspec_amd import Stop
from longspec_amd import stop as stop_mod

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, STRIDE, GUARD = 40, 48, 8            # output_ids: 40 columns in rows of 48 elements


@pytest.fixture(scope="module")
def ops():
    from longspec_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


class Buffers:
    """Every buffer of a scan, as views into flat guarded allocations (`.flat`: what is compared, guards included)."""

    def __init__(self, b, fill, top_n, device, spec_mask=True, round_state=True):
        self.flat = {}

        def make(name, dtype, sizes, strides, sentinel):
            span = 1 + sum((s - 1) * st for s, st in zip(sizes, strides))
            flat = torch.full((GUARD + span + GUARD,), sentinel, dtype=dtype)
            self.flat[name] = flat = flat.to(device)
            return flat.as_strided(sizes, strides, GUARD)

        self.out = make("out", torch.int64, (b, W), (STRIDE, 1), -77)
        self.out[:] = fill
        self.spec_mask = make("spec_mask", torch.int64, (b, W), (STRIDE, 1), -55) if spec_mask else None
        if spec_mask:
            self.spec_mask[:] = 0
        self.stop_state = make("stop_state", torch.int32, (b, 4), (4, 1), 1234)
        self.stop_state.copy_(stop_mod.new_state(b, "cpu"))
        self.state = make("state", torch.int64, (b, 2), (2, 1), 99) if round_state else None
        self.lp = None
        if top_n is not None:
            self.lp = SimpleNamespace(token=make("lp_token", torch.float32, (b, W), (W, 1), 5.0),
                                      top=make("lp_top", torch.float32, (b, W, top_n), (W * top_n, top_n, 1), 6.0),
                                      top_ids=make("lp_top_ids", torch.int64, (b, W, top_n), (W * top_n, top_n, 1), 44))
            self.lp.token[:], self.lp.top[:], self.lp.top_ids[:] = float("nan"), float("-inf"), -1


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def run_rounds(ops, text, rounds, stop, fill=0, top_n=None, form="tree", spec_mask=True, vocab=1000):
    """``text`` [b, <= W] arrives in ``rounds`` (a list of [b] column counts); the kernel and the oracle scan after every round
    and every buffer is compared, guards included, after every scan.  Returns the final stop_state [b, 4] (a list)."""
    b = len(text)
    cpu, dev = Buffers(b, fill, top_n, "cpu", spec_mask), Buffers(b, fill, top_n, DEV, spec_mask)
    table = stop.table(vocab, "cpu")
    table_d = table.to(DEV)
    written = [0] * b
    for r, counts in enumerate(rounds):
        for z in range(b):
            w0, w1 = written[z], written[z] + counts[z]
            for bufs, dv in ((cpu, "cpu"), (dev, DEV)):
                bufs.out[z, w0:w1] = torch.tensor(text[z][w0:w1], dtype=torch.int64, device=dv)
                if bufs.spec_mask is not None:
                    bufs.spec_mask[z, w0:w1] = 1
                if bufs.lp is not None:
                    bufs.lp.token[z, w0:w1], bufs.lp.top[z, w0:w1], bufs.lp.top_ids[z, w0:w1] = 0.5 + w0, -1.0 - w0, w0
            written[z] = w1
        num = torch.tensor(counts, dtype=torch.int64)
        for bufs, scan, dv in ((cpu, so.stop_scan, "cpu"), (dev, ops.stop_scan, DEV)):
            bufs.state[:, 0], bufs.state[:, 1] = num.to(dv), r % 2                     # (acc_num, the EOS flag of the commit)
            kw = dict(fill=fill, state=bufs.state, spec_mask=bufs.spec_mask, logprobs=bufs.lp)
            tab = table if dv == "cpu" else table_d
            if form == "tree":                       # written = emitted_dev, num = acc_num
                scan(bufs.out, tab, bufs.stop_state, torch.tensor(written, dtype=torch.int32, device=dv), num=num.to(dv), **kw)
            elif form == "chain":                    # written = cache_lens - input_len + 1, num = state[:, 0] (stride 2)
                lens = torch.tensor([w + 999 for w in written], dtype=torch.int32, device=dv)
                scan(bufs.out, tab, bufs.stop_state, lens, written_sub=torch.full((b,), 1000, dtype=torch.int32, device=dv),
                     written_add=1, num=bufs.state[:, 0], **kw)
            else:                                    # the vanilla step: one column, no state tensor
                assert all(c == 1 for c in counts)
                kw["state"] = None
                scan(bufs.out, tab, bufs.stop_state, torch.tensor(written, dtype=torch.int32, device=dv), num_const=1, **kw)
        for name in cpu.flat:
            assert torch.equal(bits(cpu.flat[name]), bits(dev.flat[name].cpu())), f"round {r}: {name}"
    return cpu.stop_state.tolist()


def random_rounds(rng, b, total, lo=1, hi=7):
    """Rounds of lo..hi columns per row until every row holds ``total`` columns (the first round: column 0 alone)."""
    left, rounds = [total - 1] * b, [[1] * b]
    while any(left):
        counts = [min(int(rng.randint(lo, hi + 1)), n) for n in left]
        left = [n - c for n, c in zip(left, counts)]
        rounds.append(counts)
    return rounds


def make_stop(rng, text, n_ids, seqs, min_tokens=0):
    """A stop with ``n_ids`` ids and sequences of kind ``seqs`` ("none", "one1", "16x16"), several of which occur in ``text``."""
    flat = [t for row in text for t in row]
    ids = []
    if n_ids:
        ids = [flat[int(rng.randint(len(flat)))]]
        pool = [v for v in rng.permutation(400).tolist() if v not in ids]
        ids = pool[:n_ids - 1] + ids                                 # the id of the text comes last in listing order
    sequences = []
    if seqs == "one1":
        sequences = [[flat[int(rng.randint(len(flat)))]]]
    elif seqs == "16x16":
        for q in range(16):
            z, c = q % len(text), 15 + int(rng.randint(len(text[0]) - 15))
            s = list(text[z][c - 15:c + 1])
            if q % 3 == 0:
                s[int(rng.randint(16))] += 1                         # a near miss
            sequences.append(s)
    return Stop(ids, sequences, min_tokens)


@pytest.mark.parametrize("form", ["tree", "chain"])
@pytest.mark.parametrize("top_n", [None, 0, 20])
@pytest.mark.parametrize("n_ids,seqs", [(1, "none"), (64, "none"), (0, "one1"), (0, "16x16"), (64, "16x16"), (1, "one1")])
@pytest.mark.parametrize("b", [1, 2, 3])
def test_random_texts_in_rounds(ops, b, n_ids, seqs, top_n, form):
    rng = np.random.RandomState(1000 * b + 10 * n_ids + len(seqs) + (top_n or 0))
    text = rng.randint(0, 12, size=(b, W)).tolist()
    stop = make_stop(rng, text, n_ids, seqs, min_tokens=int(rng.randint(0, 4)))
    state = run_rounds(ops, text, random_rounds(rng, b, W), stop, fill=int(rng.randint(0, 500)), top_n=top_n, form=form)
    assert all(s[0] == so.scan(text[z], stop)[0] for z, s in enumerate(state))
    assert any(s[0] > 0 for s in state), "the case was built to stop"


def test_rows_of_a_batch_stop_in_different_rounds_and_are_scanned_again(ops):
    text = [[1] * 5 + [7] + [2] * 34, [1] * 20 + [7] + [2] * 19, [1] * W]
    rounds = [[1, 1, 1]] + [[3, 3, 3]] * 13
    state = run_rounds(ops, text, rounds, Stop(token_ids=[7]), fill=3, top_n=2)
    assert [s[:3] for s in state] == [[6, 0, 5], [21, 0, 20], [-1, -1, -1]]


def test_matches_at_column_0_and_at_the_last_column(ops):
    text = [[7] + [1] * 39, [1] * 39 + [7]]
    for form, rounds in (("tree", [[1, 1]] + [[3, 3]] * 13), ("vanilla", [[1, 1]] * W)):
        state = run_rounds(ops, text, rounds, Stop(token_ids=[7], sequences=[[1, 7]]), fill=9, top_n=0, form=form)
        assert [s[:3] for s in state] == [[1, 0, 0], [40, 0, 39]]
    state = run_rounds(ops, [[1] * 38 + [4, 5]], [[1]] + [[3]] * 13, Stop(sequences=[[4, 5]]), spec_mask=False)
    assert state[0][:3] == [40, 0, 38]


def test_a_sequence_longer_than_the_written_text_and_one_across_the_prompt_boundary(ops):
    long = list(range(100, 116))
    text = [long[1:] + [3] * 25, [5, 9] + [3] * 38]                 # row 0 holds the tail of `long` from column 0 on
    state = run_rounds(ops, text, [[1, 1], [7, 7], [7, 7], [7, 7]], Stop(sequences=[long, [4, 5], long[1:]]), top_n=1)
    assert [s[:3] for s in state] == [[15, 2, 0], [-1, -1, -1]]


def test_two_candidates_in_one_round_and_the_order_of_which(ops):
    text = [[1, 2, 3, 8, 9, 3, 8] + [0] * 33]
    assert run_rounds(ops, text, [[1], [6]], Stop(token_ids=[9, 8]))[0][:3] == [4, 1, 3]                  # 8 at column 3 is earlier
    assert run_rounds(ops, text, [[1], [6]], Stop(token_ids=[9], sequences=[[3, 8]]))[0][:3] == [4, 1, 2]
    assert run_rounds(ops, text, [[1], [6]], Stop(sequences=[[2, 3, 8], [8], [3, 8]]))[0][:3] == [4, 0, 1]
    assert run_rounds(ops, text, [[1], [6]], Stop(token_ids=[5, 8], sequences=[[8]]))[0][:3] == [4, 1, 3]


@pytest.mark.parametrize("min_tokens,want", [(3, [4, 0, 3]), (4, [7, 0, 6]), (6, [7, 0, 6]), (7, [-1, -1, -1])])
def test_min_tokens_boundaries(ops, min_tokens, want):
    text = [[1, 2, 3, 8, 9, 3, 8] + [0] * 33]
    assert run_rounds(ops, text, [[1], [6], [5]], Stop(token_ids=[8], min_tokens=min_tokens))[0][:3] == want
    # a sequence that ends in front of min_tokens is ignored, one that ends at it may begin in front of it
    seq = Stop(sequences=[[3, 8]], min_tokens=min_tokens)
    assert run_rounds(ops, text, [[1], [6], [5]], seq)[0][:3] == ([4, 0, 2] if min_tokens <= 3 else [7, 0, 5] if min_tokens <= 6 else want)


def test_argument_checks(ops):
    out = torch.zeros((1, 8), dtype=torch.int64, device=DEV)
    table = Stop([1]).table(10, DEV)
    state = stop_mod.new_state(1, DEV)
    written = torch.ones((1,), dtype=torch.int32, device=DEV)
    ops.stop_scan(out, table, state, written)
    for bad in (dict(output_ids=out.int()), dict(table=table[:-1]), dict(table=table.long()), dict(stop_state=state[:, :3]),
                dict(written=written.long()), dict(num=written), dict(state=torch.zeros((1, 1), dtype=torch.int64, device=DEV)),
                dict(spec_mask=torch.zeros((1, 7), dtype=torch.int64, device=DEV)), dict(output_ids=out.cpu())):
        kw = dict(output_ids=out, table=table, stop_state=state, written=written)
        kw.update(bad)
        with pytest.raises((TypeError, RuntimeError)):
            ops.stop_scan(**kw)
