"""Token penalties and logit bias (``penalties=``) end to end on the HIP kernels: the pairs of
tests/test_host_generate_penalized.py on the device -- launch by launch, replayed from HIP graphs and with the graphs captured up
front -- against the CPU oracle's penalised vanilla text, the state word table after graph runs (a warm-up round counted twice
shows here), the distinct-token property under graphs, and two generations with different penalties on one model object."""
import pytest
import torch

import penalty_oracle as po
import sampled_runs as sr
import test_host_generate_penalized as hp
from longspec_amd import Penalties, Sampling
from test_host_generate_sampled import build as _build, get_run

pytestmark = pytest.mark.gpu
_CPU = {}


def build(run):
    return _build(run, device="cuda")


def cpu_text(kind, name, kw):
    """(run, penalties, tokens, the CPU oracle's penalised vanilla text, its penalised rows), computed once per pair."""
    key = (kind, name, repr(kw))
    if key not in _CPU:
        run, m, pen, gen, text = hp.checked_vanilla(kind, name, kw)
        _, raw = hp.vanilla_with_raw(m, po.ops, run, pen, gen)
        _CPU[key] = (run, pen, gen, text, hp.penalised_rows(run, text, raw, pen))
    return _CPU[key]


def parting(out, n, text, rows, tol, what):
    """None when ``out[:n]`` is the CPU text; else the first other token, after asserting that it is an explained near-tie:
    the device took the runner-up of the CPU's penalised row and the two were closer than `tol` (the rule of
    tests/sampled_runs.py, on logits instead of keys)."""
    a, b = out[:n].cpu(), text[:n]
    neq = (a != b).nonzero()
    if neq.numel() == 0:
        return None
    i = int(neq[0])
    best = rows[i].float().topk(2)
    margin = float(best.values[0] - best.values[1])
    assert int(a[i]) == int(best.indices[1]) and margin < tol, \
        f"{what}: parts from the CPU text at token {i} (took {int(a[i])}, CPU {int(b[i])}, runner-up {int(best.indices[1])}, margin {margin})"
    return i


def device_texts(m, run, pen, gen):
    ids, pl = run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda")
    v, _, _ = m.vanilla_generate(ids, pl, max_gen_len=gen, eos_id=run["eos_id"], penalties=pen)
    return {"vanilla": (v.cpu(), gen), **hp.loops(m, run, gen, device="cuda", penalties=pen)}


@pytest.mark.parametrize("kind,name,kw", hp.all_pairs())
def test_the_device_emits_the_cpu_text_three_ways(kind, name, kw):
    run, pen, gen, text, rows = cpu_text(kind, name, kw)
    tol = sr.TOL[run["dtype"]]
    m = build(run)
    m.GRAPH_AFTER = 0
    for mode in ("eager", "graphs", "prepared"):
        m.GRAPH_ROUNDS = mode != "eager"
        if mode == "prepared":
            st = hp.drive_tree(m, run, pen, gen, prepare=True)
            assert st.replayer.captures > 0 and not st.replayer.disabled, "no round was captured up front"
            texts = {"tree": (st.output_ids.cpu(), min(st.emitted, gen))}
            hp.assert_state_is_the_bincount(run, st, "tree")
        else:
            texts = device_texts(m, run, pen, gen)
        for loop, (out, n) in texts.items():
            assert n >= gen - 7, (mode, loop, n)
            assert parting(out[0], n, text, rows, tol, f"{mode} {loop}") is None, (mode, loop)


@pytest.mark.parametrize("family,name", [("llama", "mixed"), ("qwen2_bf16", "qwen_bf16_g5")])
def test_the_state_is_the_bincount_after_graph_runs(family, name):
    run = get_run(family, name)
    m = build(run)
    m.GRAPH_AFTER = 0
    pen = Penalties(**hp.STRONG)
    gen = 40
    st = hp.drive_tree(m, run, pen, gen)
    assert st.replayer.captures > 0 and not st.replayer.disabled, "no round was replayed"
    hp.assert_state_is_the_bincount(run, st, "tree")
    st = hp.drive_tree(m, run, pen, gen, prepare=True)
    assert st.replayer.captures > 0 and not st.replayer.disabled
    hp.assert_state_is_the_bincount(run, st, "tree")
    vs = hp.drive_vanilla(m, run, pen, gen)
    assert vs.replayer.captures > 0 and not vs.replayer.disabled, "no step was replayed"
    hp.assert_state_is_the_bincount(run, vs, "vanilla")
    hp.assert_state_is_the_bincount(run, hp.drive_chain(m, run, pen, gen), "chain")
    m.GRAPH_ROUNDS = False
    eager = hp.drive_tree(m, run, pen, gen)
    assert torch.equal(eager.token_state, st.token_state) and torch.equal(eager.output_ids, st.output_ids)


@pytest.mark.parametrize("family,name", [("llama", "forced"), ("qwen2_bf16", "qwen_bf16_g5")])
def test_no_token_repeats_under_graphs(family, name):
    run = get_run(family, name)
    m = build(run)
    m.GRAPH_AFTER = 0
    gen = 40
    for loop, (out, n) in device_texts(m, run, Penalties(presence=1e4), gen).items():
        row = out[0, :n].tolist()
        assert len(set(row)) == len(row), (loop, row)


def test_a_second_generation_takes_its_own_penalties():
    """The scalars are launch arguments of graphs that belong to one generation."""
    run = get_run("llama", "forced")
    m = build(run)
    gen = 32
    a, b = Penalties(**hp.STRONG), Penalties(repetition=1.05, presence=1e4)

    def tree(pen):
        st = hp.drive_tree(m, run, pen, gen)
        return st.output_ids[0, :st.emitted].cpu(), st

    m.GRAPH_ROUNDS = False
    want_a, want_b = tree(a)[0], tree(b)[0]
    n = min(want_a.numel(), want_b.numel())
    assert not torch.equal(want_a[:n], want_b[:n])
    m.GRAPH_ROUNDS, m.GRAPH_AFTER = True, 0
    for pen, want in ((a, want_a), (b, want_b), (b, want_b), (a, want_a)):
        got, st = tree(pen)
        assert st.replayer.captures > 0 and not st.replayer.disabled
        assert torch.equal(got, want), "a generation replayed another generation's penalties"


def test_sampled_with_penalties_from_graphs():
    """``ls_penalize_rows`` -> ``ls_sample_rows`` -> ``ls_token_state_add`` inside captured rounds and steps: the sampled pairs of
    the CPU file under the rule of tests/sampled_runs.py (a loop may leave the spied vanilla text only where it took the
    runner-up and the keys were closer than tol / T); at most one pair may part; the state is the bincount afterwards."""
    from longspec_amd import ops
    g = hp.SAMPLED
    T, gen = g["temperature"], g["max_gen_len"]
    pen = Penalties(**g["penalties"])
    parted = []
    for name, seed in (("gqa_mixed", 133), ("mixed@1030", 287), ("forced", 772)):
        assert (name, seed) in g["pairs"]
        run = get_run(g["family"], name)
        P, tol = run["prompt_len"], sr.TOL[run["dtype"]]
        sampling = Sampling(T, g["top_k"], g["top_p"], seed)
        m = build(run)
        m.GRAPH_AFTER = 0
        spy = sr.Top2Spy(ops)
        m.ops, m.GRAPH_ROUNDS = spy, False
        try:
            v_out, _, _ = m.vanilla_generate(run["prompt"].cuda(), torch.tensor([P], device="cuda"), max_gen_len=gen,
                                             eos_id=run["eos_id"], sampling=sampling, penalties=pen)
        finally:
            m.ops, m.GRAPH_ROUNDS = ops, True
        v_out = v_out.cpu()
        rec = {pos: v for (s, pos), v in spy.rec.items() if s == 0}
        n_v = sr.stop_len(v_out, m._stop_id(run["eos_id"], "vanilla"), gen)
        texts = device_texts_sampled(m, run, pen, sampling, gen)
        for loop, (out, n, st) in texts.items():
            if st is not None:
                assert st.replayer.captures > 0 and not st.replayer.disabled, f"{loop}: nothing was replayed"
                hp.assert_state_is_the_bincount(run, st, loop)
            at = sr.parting(out, min(n, n_v), v_out, rec, P, T, tol, f"{name} seed {seed} {loop}")
            if at is not None:
                parted.append((name, seed, loop, at))
    print("parted:", parted)
    assert len({(n, s) for n, s, _, _ in parted}) <= 1, parted


def device_texts_sampled(m, run, pen, sampling, gen):
    """{loop: (output_ids, tokens that count, decode state or None)} with graphs on."""
    states = {}
    for what in ("begin_vanilla_decode", "begin_tree_decode"):
        orig = getattr(m, what)
        setattr(m, what, lambda *a, _o=orig, _w=what, **k: states.setdefault(_w, _o(*a, **k)))
    try:
        ids, pl = run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda")
        v, _, _ = m.vanilla_generate(ids, pl, max_gen_len=gen, eos_id=run["eos_id"], penalties=pen, sampling=sampling)
        outs = hp.loops(m, run, gen, device="cuda", penalties=pen, sampling=sampling)
    finally:
        del m.begin_vanilla_decode, m.begin_tree_decode
    res = {k: (o, n, None) for k, (o, n) in outs.items()}
    res["vanilla"] = (v.cpu(), gen, states["begin_vanilla_decode"])
    res["tree"] = (*outs["tree"], states["begin_tree_decode"])
    return res
