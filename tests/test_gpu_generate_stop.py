"""``stop=`` end to end on the HIP kernels: the toy runs of tests/test_host_generate_stop.py on the device.  Every expectation
is the oracle's cut of the DEVICE's own plain text of the same loop -- exact, and immune to 16-bit near-ties against the CPU:
the cut inside a round, across rounds and on column 0, the loops replayed from HIP graphs against the launch-by-launch loops,
``prepare_tree_graphs``' warm-up rounds, and ``min_tokens`` against the device's banned vanilla run."""
import pytest
import torch

import sampled_runs as sr
import stop_oracle as so
import test_host_generate_logprobs as hl
import test_host_generate_stop as hs
from longspec_amd import Stop
from test_host_generate_penalized import top2_margin
from test_host_generate_sampled import build as _build, get_run

pytestmark = pytest.mark.gpu
KEYS = ["greedy-mixed", "greedy-bf16", "greedy-long", "sampled-forced"]
KINDS = {"id-inside-a-round", "bigram-inside-a-round", "bigram-across-rounds", "column-0"}
_models, _plain = {}, {}


def model_of(key):
    if key not in _models:
        family, name, sampling, pen_kw = hl.CONFIGS[key]
        run = get_run(family, name)
        m = _build(run, device="cuda")
        m.GRAPH_AFTER = 0
        _models[key] = (run, sampling, m)
    return _models[key]


def device_loop(m, loop, run, sampling, stop, graphs, spy=False, **kw):
    from longspec_amd import ops
    m.GRAPH_ROUNDS = graphs
    try:
        return hs.run_loop(m, loop, run, sampling, stop, device="cuda", spy_on=ops if spy else None, **kw)
    finally:
        m.GRAPH_ROUNDS = True


def plain_runs(key):
    """{loop: the device's plain run}, launch by launch under the spy: the rounds' accepted counts are read off the operators."""
    if key not in _plain:
        run, sampling, m = model_of(key)
        _plain[key] = {loop: device_loop(m, loop, run, sampling, None, graphs=False, spy=True) for loop in hs.loops_of(run)}
    return _plain[key]


def derived(key):
    """{Stop: what it is}, one stop of every kind, from the speculative loops of the device's plain runs (the tree loop first)."""
    found = {}
    plain = plain_runs(key)
    for loop in sorted(plain, key=lambda l: l != "tree"):
        p = plain[loop]
        if loop == "vanilla" or max(p.rounds) < 2:
            continue
        for kind, (stop, c) in hs.derive_stops(p, loop).items():
            found.setdefault(kind, (stop, f"{kind} of {loop} at column {c}"))
    assert set(found) == KINDS, sorted(found)
    return dict(found.values())


def same_bits(a, b, what):
    assert a.out == b.out and a.stop == b.stop, what
    for name in ("token", "top", "top_ids"):
        assert torch.equal(hl.bits(getattr(a.lp, name)), hl.bits(getattr(b.lp, name))), (what, name)


@pytest.mark.parametrize("key", KEYS)
def test_every_loop_returns_the_oracles_cut_of_the_devices_plain_text(key):
    run, sampling, m = model_of(key)
    plain = plain_runs(key)
    assert all(p.n > hs.LAST_COL and p.stop is None for p in plain.values())
    for stop, what in derived(key).items():
        for loop in plain:
            got = device_loop(m, loop, run, sampling, stop, graphs=True)
            hs.check_cut(got, plain[loop], stop, hs.fill_of(m, run, loop), loop, what)


@pytest.mark.parametrize("key", ["greedy-mixed", "greedy-long"])
def test_graph_replay_gives_the_bits_of_the_launch_by_launch_loops(key):
    """The tree loop through ``prepare_tree_graphs``, so that every round is a replay: its warm-up rounds leave ``stop_state``
    (and the text) as they were."""
    run, sampling, m = model_of(key)
    plain = plain_runs(key)
    states = {}

    def wrap(what, prepare):
        orig = getattr(m, what)

        def begin(*a, **k):
            st = orig(*a, **k)
            if prepare and m.GRAPH_ROUNDS:
                before = [t.clone() for t in (st.stop_state, st.output_ids, st.logprobs.token, st.logprobs.top_ids)]
                m.prepare_tree_graphs(st)
                assert st.replayer.captures > 0 and not st.replayer.disabled, "no round was captured up front"
                for t, b in zip((st.stop_state, st.output_ids, st.logprobs.token, st.logprobs.top_ids), before):
                    assert torch.equal(hl.bits(t), hl.bits(b)), "a warm-up round left a trace"
                assert not st.stopped and st.emitted == 1
            states[what] = st
            return st
        setattr(m, what, begin)

    wrap("begin_tree_decode", True)
    wrap("begin_vanilla_decode", False)
    try:
        for stop, what in derived(key).items():
            for loop, begin in (("vanilla", "begin_vanilla_decode"), ("tree", "begin_tree_decode")):
                replayed = device_loop(m, loop, run, sampling, stop, graphs=True)
                rp = states[begin].replayer
                assert rp.captures > 0 and not rp.disabled, f"{loop}: nothing was replayed ({what})"
                eager = device_loop(m, loop, run, sampling, stop, graphs=False)
                same_bits(replayed, eager, (what, loop))
                hs.check_cut(replayed, plain[loop], stop, hs.fill_of(m, run, loop), loop, what)
    finally:
        del m.begin_tree_decode, m.begin_vanilla_decode


class BanSpy(hs.BanSpy):
    """... on the device's operator module."""

    def __init__(self):
        from longspec_amd import ops
        super().__init__(ops)


@pytest.mark.parametrize("key,col,min_tokens", hs.BANNED)
def test_min_tokens_equals_the_devices_banned_vanilla_run(key, col, min_tokens):
    run, sampling, m = model_of(key)
    text = plain_runs(key)["vanilla"].out
    stop = Stop(token_ids=[text[col]], min_tokens=min_tokens)
    spy = BanSpy()
    saved = m.ops
    m.ops, m.GRAPH_ROUNDS = spy, False
    try:
        out = m.vanilla_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"), max_gen_len=hs.GEN,
                                 eos_id=run["eos_id"], sampling=sampling, stop=stop)[0][0].tolist()
        triple = tuple(int(t[0]) for t in (m.last_stop.length, m.last_stop.which, m.last_stop.match_start))
    finally:
        m.ops, m.GRAPH_ROUNDS = saved, True
    n = triple[0] if triple[0] > 0 else hs.GEN
    rows = torch.cat([r[1] for r in spy.rows])[:n].cpu()
    assert rows.float().argmax(dim=-1).tolist() == out[:n], "a token is not the arg-max of its banned row"
    assert torch.isinf(rows[:min_tokens, text[col]].float()).all() and not torch.isinf(rows[min_tokens:].float()).any()
    assert text[col] not in out[:min_tokens] and out[:col] == text[:col]
    margin = top2_margin(rows)
    print(f"{key}: smallest top-2 margin of the device's banned run {margin:.4f}, bound {sr.TOL[run['dtype']]}")
    assert margin >= sr.TOL[run["dtype"]], "choose another (run, stop) pair: a row of the device's banned run is a near-tie"
    assert triple == so.scan(out[:n], stop) and out[n:] == [0] * (hs.GEN - n)
    for loop in hs.loops_of(run):
        for graphs in (True, False):
            got = device_loop(m, loop, run, sampling, stop, graphs=graphs)
            k = min(n, got.n) if triple[0] < 0 else n
            assert got.stop == triple and got.out[:k] == out[:k], (loop, graphs, got.out, out)
