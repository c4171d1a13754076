"""``logprobs=`` end to end on the HIP kernels: the toy runs of tests/test_host_generate_logprobs.py on the device -- the keyword
changes no token, the log-probs are within the bound of the CPU oracle's run of the same loop, the loops replayed from HIP
graphs give the bits of the launch-by-launch loops, ``prepare_tree_graphs`` leaves the fill behind the emitted columns, and
the first alternative of a greedy row is the emitted token."""
import pytest
import torch

import sampled_runs as sr
import test_host_generate_logprobs as hl
from longspec_amd import Logprobs, Penalties
from test_host_generate_sampled import build as _build, get_run

pytestmark = pytest.mark.gpu
# greedy fp16 / bf16, greedy and sampled with penalties on the long prompt (+ MagicDec)
KEYS = ["greedy-mixed", "greedy-bf16", "greedy-long", "sampled-penalised-long"]


def build(run):
    m = _build(run, device="cuda")
    m.GRAPH_AFTER = 0
    return m


def device_runs(key, logprobs):
    family, name, sampling, pen_kw = hl.CONFIGS[key]
    run = get_run(family, name)
    pen = Penalties(**pen_kw) if pen_kw else None
    m = build(run)
    loops = ["vanilla", "chain", "tree"] + (["magicdec"] if run["prompt_len"] >= 1024 else [])
    return run, sampling, {loop: hl.run_loop(m, loop, run, sampling, pen, logprobs, spy_on=None, device="cuda") for loop in loops}


def emitted_columns(lp):
    return int((~torch.isnan(lp.token[0])).sum())


@pytest.mark.parametrize("key", KEYS)
def test_no_token_changes_and_the_logprobs_are_the_cpu_oracles(key):
    run, sampling, with_lp = device_runs(key, Logprobs(hl.TOP_N))
    _, _, without = device_runs(key, None)
    T = sampling.temperature if sampling is not None else 1.0
    bound = 2 * sr.TOL[run["dtype"]] / T
    _, _, cpu = hl.runs_of(key)
    for loop, (out, count, num, lp, _) in with_lp.items():
        assert torch.equal(out, without[loop][0]) and (count, num) == without[loop][1:3], loop
        assert without[loop][3] is None
        n = emitted_columns(lp)
        assert n >= 8 and torch.isnan(lp.token[0, n:]).all() and (lp.top_ids[0, n:] == -1).all(), loop
        assert (lp.top[0, n:] == float("-inf")).all(), loop
        c_out, _, _, c_lp, _ = cpu[loop][0]
        n = min(n, emitted_columns(c_lp))
        same = (out[0, :n].cpu() == c_out[0, :n]).long().cumprod(0).sum().item()
        assert same >= 8, f"{loop}: only {same} tokens in common with the CPU oracle's run"
        err = (lp.token[0, :same].cpu().double() - c_lp.token[0, :same].double()).abs().max().item()
        print(f"{key} {loop}: {same} common tokens, largest log-prob difference to the CPU oracle {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (loop, err, bound)
        if sampling is None:                                      # the arg-max's own tie rule: exact
            cols = emitted_columns(lp)
            assert torch.equal(lp.top_ids[0, :cols, 0], out[0, :cols]), loop
            assert torch.equal(lp.top[0, :cols, 0], lp.token[0, :cols]), loop


@pytest.mark.parametrize("key", ["greedy-mixed", "sampled-penalised-long"])
def test_graph_replay_gives_the_bits_of_the_launch_by_launch_loops(key):
    family, name, sampling, pen_kw = hl.CONFIGS[key]
    run = get_run(family, name)
    pen = Penalties(**pen_kw) if pen_kw else None
    m = build(run)
    res = {}
    for graphs in (True, False):
        m.GRAPH_ROUNDS = graphs
        for loop in ("vanilla", "tree"):
            states = []
            what = "begin_vanilla_decode" if loop == "vanilla" else "begin_tree_decode"
            orig = getattr(m, what)
            setattr(m, what, lambda *a, _o=orig, **k: states.append(_o(*a, **k)) or states[-1])
            try:
                out, _, _, lp, _ = hl.run_loop(m, loop, run, sampling, pen, Logprobs(5), spy_on=None, device="cuda")
            finally:
                delattr(m, what)
            if graphs:
                assert states[0].replayer.captures > 0 and not states[0].replayer.disabled, f"{loop}: nothing was replayed"
            res[(graphs, loop)] = (out, lp)
    for loop in ("vanilla", "tree"):
        (g_out, g_lp), (e_out, e_lp) = res[(True, loop)], res[(False, loop)]
        assert torch.equal(g_out, e_out), loop
        for name in ("token", "top", "top_ids"):
            assert torch.equal(hl.bits(getattr(g_lp, name)), hl.bits(getattr(e_lp, name))), f"{loop}: {name}"


def test_prepare_tree_graphs_leaves_the_fill_behind_the_emitted_columns():
    run = get_run("llama", "mixed")
    m = build(run)
    seen = []
    orig = m.begin_tree_decode

    def begin(*a, **k):
        st = orig(*a, **k)
        before = [t.clone() for t in (st.logprobs.token, st.logprobs.top, st.logprobs.top_ids)]
        m.prepare_tree_graphs(st)
        assert st.replayer.captures > 0 and not st.replayer.disabled, "no round was captured up front"
        lp = st.logprobs
        assert st.emitted == 1 and not torch.isnan(lp.token[:, 0]).any()
        assert torch.isnan(lp.token[:, 1:]).all() and (lp.top_ids[:, 1:] == -1).all() and (lp.top[:, 1:] == float("-inf")).all()
        for t, b in zip((lp.token, lp.top, lp.top_ids), before):
            assert torch.equal(hl.bits(t), hl.bits(b))
        seen.append(st)
        return st

    m.begin_tree_decode = begin
    try:
        out, _, _, lp, _ = hl.run_loop(m, "tree", run, None, None, Logprobs(2), spy_on=None, device="cuda")
    finally:
        del m.begin_tree_decode
    n = seen[0].emitted
    assert n >= 8 and emitted_columns(lp) == n and torch.isnan(lp.token[0, n:]).all() and (lp.top_ids[0, n:] == -1).all()
    assert torch.equal(lp.top_ids[0, :n, 0], out[0, :n])
