"""``guide=`` end to end on the HIP kernels: the toy runs of tests/test_host_generate_guide.py on the device, under the parity
guide and the choice guide.  The device's guided vanilla run, launch by launch under a spy that keeps every row ``ops.guide_rows``
handed back and the state it was handed, is the host oracle's text up to a column the project's 16-bit near-tie bound explains;
every loop -- vanilla, chain, tree, lookup with one branch and with two, launch by launch and replayed from HIP graphs -- is that
device text up to such a column, and exactly that text where no row of the device's run is a near-tie; replayed rounds equal
eager rounds token for token, with one host read per replayed round."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import guide_oracle as go
import sampled_runs as sr
import test_gpu_generate_lookup as gk
import test_gpu_generate_lookup_tree as gt
import test_host_generate_guide as hg

pytestmark = pytest.mark.gpu
GEN, G = gk.GEN, 4
RUNS = hg.RUNS
_ref = {}


class GuideSpy:
    """The device's operator module with every row ``guide_rows`` returned and the state it was handed kept (host reads: for
    launch-by-launch runs only)."""

    def __init__(self):
        from longspec_amd import ops
        self._base, self.rows, self.states = ops, [], []

    def __getattr__(self, name):
        return getattr(self._base, name)

    def guide_rows(self, logits, table, state, **kw):
        self.states.append(state.cpu().tolist())
        out = self._base.guide_rows(logits, table, state, **kw)
        self.rows.append(out.reshape(-1, out.shape[-1])[:1].float().cpu())
        return out


def cut(text, eos):
    return text[:text.index(eos) + 1] if eos in text else text


def device_vanilla(family, name, guide, eos):
    """(text, the guided row of every column) of the device's launch-by-launch vanilla run under ``guide``."""
    if (family, name, guide) not in _ref:
        run, m = gk.model_of(family, name)
        V = run["cfg"].vocab_size
        spy = GuideSpy()
        m.ops, m.GRAPH_ROUNDS = spy, False
        try:
            out = m.vanilla_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"), max_gen_len=GEN,
                                     eos_id=run["eos_id"], guide=guide)[0][0].tolist()
        finally:
            m.ops, m.GRAPH_ROUNDS = spy._base, True
        rows = torch.cat(spy.rows)
        text = cut(out, eos)
        assert rows.argmax(dim=-1).tolist()[:len(text)] == text, "a token is not the arg-max of its guided row"
        p = go.parse(guide.table(V, "cpu"))
        for c in range(min(len(text), rows.shape[0])):                    # the rows carry -inf exactly where the oracle forbids
            s = go.walk(p, guide.start, text[:c])
            assert s >= 0 and spy.states[c] == [s], ("a step did not see the state of the text so far", c)
            assert torch.isinf(rows[c]).nonzero().view(-1).tolist() == np.flatnonzero(~go.allowed(p, s, V)).tolist(), c
        _ref[family, name, guide] = (text, rows)
    return _ref[family, name, guide]


def explained(text, ref, rows, tol, what):
    """``text`` is ``ref`` up to its first difference, and there both tokens lie within ``tol`` of the best entry of the
    device's vanilla row.  Returns the number of columns that agree."""
    n = min(len(text), len(ref))
    diff = [c for c in range(n) if text[c] != ref[c]]
    if not diff:
        return n
    c = diff[0]
    top, took, other = float(rows[c].max()), float(rows[c, ref[c]]), float(rows[c, text[c]])
    print(f"{what}: parts at column {c}: {text[c]} at {other}, the device's vanilla run {ref[c]} at {took}; bound {tol}")
    assert took == top and top - other < tol, what
    return c


def glide_loop(family, name, loop, guide, graphs):
    run, m = gk.model_of(family, name)
    ids, pl = run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda")
    kw = dict(max_gen_len=GEN, eos_id=run["eos_id"], guide=guide)
    states = []
    begin = {"vanilla": "begin_vanilla_decode", "chain": "begin_chain_decode", "magicdec": "begin_chain_decode",
             "tree": "begin_tree_decode", "lookup1": "begin_lookup_decode", "lookup2": "begin_lookup_decode"}[loop]
    orig = getattr(m, begin)
    setattr(m, begin, lambda *a, **k: states.append(orig(*a, **k)) or states[-1])
    m.GRAPH_ROUNDS = graphs
    try:
        if loop == "vanilla":
            got = SimpleNamespace(out=m.vanilla_generate(ids, pl, **kw)[0][0].tolist(), n=GEN)
        elif loop in ("chain", "magicdec"):
            gen = m.spec_generate if loop == "chain" else m.magicdec_generate
            out, count, num, _, _ = gen(ids, pl, gamma=G if loop == "chain" else 3, **kw)
            got = SimpleNamespace(out=out[0].tolist(), n=1 + int(count) + int(num))
        elif loop == "tree":
            out, count, num, _, _ = m.tree_spec_generate(ids, pl, tree_shape=hg.tree_shape_of(run, name), **kw)
            got = SimpleNamespace(out=out[0].tolist(), n=int(count) + int(num))        # (the tree loop's num starts at 1)
        else:
            out, count, num, _, _ = m.lookup_generate(ids, pl, gamma=G, max_ngram=3, min_ngram=1, branches=int(loop[-1]), **kw)
            got = SimpleNamespace(out=out[0].tolist(), n=1 + int(count) + int(num))
    finally:
        delattr(m, begin)
        m.GRAPH_ROUNDS = True
    st = states[0]
    assert st.guide is not None and st.guide.cfg == guide and st.guide.state.dtype == torch.int32
    assert not st.replayer.disabled if hasattr(st, "replayer") else True
    got.st = st
    return got


def run_loop(family, name, loop, guide, graphs):
    """The long runs of the lookup loops go through the helpers of their own tests (which assert replayed / eager as asked, and
    size the launch-by-launch tree rounds like the replayed ones)."""
    if loop == "lookup1":
        return gk.lookup(family, name, graphs=graphs, guide=guide)
    if loop == "lookup2":
        return gt.tree_lookup(family, name, graphs=graphs, b=2, tier_sized=not graphs, guide=guide)
    got = glide_loop(family, name, loop, guide, graphs)
    if loop in ("vanilla", "tree"):                                       # (the chain rounds are not captured)
        assert (got.st.replayer.captures > 0 and not got.st.replayer.disabled) == bool(graphs), "replayed / eager as asked"
    return got


@pytest.mark.parametrize("family,name", RUNS)
def test_every_loop_eager_and_replayed_gives_the_parity_text(family, name):
    run, m = gk.model_of(family, name)
    tol = sr.TOL[run["dtype"]]
    eos, V = hg.eos_of(run, m), run["cfg"].vocab_size
    plain, _ = gk.vanilla(family, name)
    start = next(s for s in (plain[0] % 2, 1 - plain[0] % 2) if not hg.in_parity(plain, s, eos))       # the device's own plain text leaves it
    guide = hg.parity_guide(V, eos, start)
    ref, rows = device_vanilla(family, name, guide, eos)
    assert hg.in_parity(ref, start, eos) and ref != plain[:len(ref)] and len(ref) >= GEN - 24
    host = hg.text_of(hg.run_loop(family, name, "vanilla", guide), eos)
    same = explained(host, ref, rows, tol, (name, "the host oracle's text"))
    assert same >= 24
    best = rows.topk(2, dim=-1).values
    exact = float((best[:, 0] - best[:, 1]).min()) >= tol                 # no row of the device's run is a near-tie
    print(f"{name}: the host oracle's text agrees on {same} columns; smallest top-2 margin of the device's guided rows "
          f"{float((best[:, 0] - best[:, 1]).min()):.4f}, bound {tol}")
    p = go.parse(guide.table(V, "cpu"))
    for loop in ("vanilla", "chain", "tree", "lookup1", "lookup2"):
        got = {graphs: run_loop(family, name, loop, guide, graphs) for graphs in (False, True)}
        for graphs, g in got.items():
            text = cut(g.out[:min(g.n, GEN)], eos)
            assert len(text) >= len(ref) - 24, (loop, graphs, len(text))
            upto = explained(text, ref, rows, tol, (name, loop, "replayed" if graphs else "eager"))
            assert upto >= 24 and hg.in_parity(text, start, eos), (loop, graphs)
            assert all(go.walk(p, guide.start, text[:c]) >= 0 for c in range(len(text) + 1)), (loop, graphs)
            assert upto == min(len(text), len(ref)) or not exact, (loop, graphs)
        n = min(got[True].n, got[False].n, GEN)                          # replayed against launch by launch: the same text
        assert got[True].n == got[False].n and got[True].out[:n] == got[False].out[:n], loop


@pytest.mark.parametrize("family,name", [("llama", "mixed"), ("qwen2_bf16", "qwen_bf16_g5")])
def test_every_loop_eager_and_replayed_gives_the_chosen_text(family, name):
    run, m = gk.model_of(family, name)
    tol = sr.TOL[run["dtype"]]
    guide, seqs, eos = hg.choice_for(family, name)
    ref, rows = device_vanilla(family, name, guide, eos)
    assert ref in [s + [eos] for s in seqs]
    for loop in ("vanilla", "chain", "tree", "lookup1", "lookup2"):
        texts = []
        for graphs in (False, True):
            g = glide_loop(family, name, loop, guide, graphs)
            text = cut(g.out[:min(g.n, GEN)], eos)
            assert text in [s + [eos] for s in seqs], (loop, graphs, text)
            explained(text, ref, rows, tol, (name, loop, graphs))            # the vanilla run's choice, or the other side of a near-tie
            texts.append(g.out[:min(g.n, GEN)])
        assert texts[0] == texts[1], loop


def test_magicdec_on_a_long_prompt():
    """The fourth loop needs a prompt beyond its streaming window: the `mixed` run behind a 1030-token prompt."""
    family, name = "llama", "mixed@1030"
    run, m = gk.model_of(family, name)
    tol = sr.TOL[run["dtype"]]
    eos, V = hg.eos_of(run, m), run["cfg"].vocab_size
    plain, _ = gk.vanilla(family, name)
    start = next(s for s in (0, 1) if not hg.in_parity(plain, s, eos))
    guide = hg.parity_guide(V, eos, start)
    ref, rows = device_vanilla(family, name, guide, eos)
    for loop in ("magicdec", "chain"):
        g = glide_loop(family, name, loop, guide, graphs=True)
        text = cut(g.out[:min(g.n, GEN)], eos)
        assert len(text) >= len(ref) - 8 and explained(text, ref, rows, tol, (name, loop)) >= 24 and hg.in_parity(text, start, eos), loop


def test_one_host_read_per_replayed_round():
    """torch.cuda.synchronize and the .tolist / .item / .cpu / int() / bool() reads of device tensors, counted inside every
    round of the tree loop and of both lookup loops whose graph was already captured when it began, under the parity guide."""
    family, name = "llama", "mixed"
    run, m = gk.model_of(family, name)
    eos, V = hg.eos_of(run, m), run["cfg"].vocab_size
    plain, _ = gk.vanilla(family, name)
    start = next(s for s in (0, 1) if not hg.in_parity(plain, s, eos))
    guide = hg.parity_guide(V, eos, start)
    reads, patched = {"n": 0}, []

    def counting(owner, attr):
        real = getattr(owner, attr)

        def spy(*a, **k):
            if owner is torch.cuda or (a and isinstance(a[0], torch.Tensor) and a[0].is_cuda):
                reads["n"] += 1
            return real(*a, **k)

        patched.append((owner, attr, real, attr in vars(owner)))
        setattr(owner, attr, spy)

    from longspec_amd.llama_glide import LlamaGlide
    real_tree, real_lookup = LlamaGlide.tree_round, LlamaGlide.lookup_round
    per_round = {"tree": [], "lookup1": [], "lookup2": []}

    def tree_round(self, st):
        replayed = st.use_graphs and st.replayer.captured(st.a)
        reads["n"] = 0
        go_on = real_tree(self, st)
        if replayed:
            per_round["tree"].append(reads["n"])
        return go_on

    def lookup_round(self, st):
        tree = getattr(st, "branches", 1) > 1
        replayed = st.use_graphs and st.replayer.captured(st.a if tree else None)
        reads["n"] = 0
        go_on = real_lookup(self, st)
        if replayed:
            per_round["lookup2" if tree else "lookup1"].append(reads["n"])
        return go_on

    LlamaGlide.tree_round, LlamaGlide.lookup_round = tree_round, lookup_round
    try:
        counting(torch.cuda, "synchronize")
        for attr in ("tolist", "item", "cpu", "numpy", "__int__", "__bool__", "__float__", "__index__"):
            counting(torch.Tensor, attr)
        texts = {loop: glide_loop(family, name, loop, guide, graphs=True) for loop in per_round}
    finally:
        LlamaGlide.tree_round, LlamaGlide.lookup_round = real_tree, real_lookup
        for owner, attr, real, own in patched:
            if own:
                setattr(owner, attr, real)
            else:
                delattr(owner, attr)
    for loop, counts in per_round.items():
        print(f"{loop}: {len(counts)} replayed rounds, host reads {sorted(set(counts))}")
        assert len(counts) >= 3, f"{loop}: only {len(counts)} rounds were replayed"
        assert set(counts) == {1}, (loop, counts)
        g = texts[loop]
        assert hg.in_parity(cut(g.out[:min(g.n, GEN)], eos), start, eos), loop
