"""``ban=`` end to end on the HIP kernels: the toy runs of tests/test_host_generate_ban.py on the device.  The device's banned
vanilla run, launch by launch under a spy that keeps every row ``ops.ban_rows`` handed back, is the host oracle's text up to a
column the project's 16-bit near-tie bound explains; every loop -- vanilla, chain, tree, lookup with one branch and with two,
launch by launch and replayed from HIP graphs -- is that device text up to such a column, and exactly that text where no row of
the device's run is a near-tie."""
from types import SimpleNamespace

import pytest
import torch

import ban_oracle as bo
import sampled_runs as sr
import test_gpu_generate_lookup as gk
import test_gpu_generate_lookup_tree as gt
import test_host_generate_ban as hb
from longspec_amd import Ban

pytestmark = pytest.mark.gpu
GEN, G = gk.GEN, 4
RUNS = hb.RUNS
_ref = {}


class BanSpy:
    """The device's operator module with every row ``ban_rows`` returned and the committed text it saw kept (host reads: for
    launch-by-launch runs only)."""

    def __init__(self):
        from longspec_amd import ops
        self._base, self.rows, self.seen = ops, [], []

    def __getattr__(self, name):
        return getattr(self._base, name)

    def ban_rows(self, logits, table, output_ids, base=None, base_sub=None, base_add=0, **kw):
        out = self._base.ban_rows(logits, table, output_ids, base=base, base_sub=base_sub, base_add=base_add, **kw)
        cpu = lambda t: None if t is None else t.cpu()
        self.seen.append(bo.row_texts(1, 1, cpu(output_ids), cpu(base), cpu(base_sub), base_add)[0][0])
        self.rows.append(out.reshape(-1, out.shape[-1])[:1].float().cpu())
        return out


def device_vanilla(family, name, ban):
    """(text, the banned row of every column) of the device's launch-by-launch vanilla run under ``ban``."""
    if (family, name, ban) not in _ref:
        run, m = gk.model_of(family, name)
        spy = BanSpy()
        m.ops, m.GRAPH_ROUNDS = spy, False
        try:
            out = m.vanilla_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"), max_gen_len=GEN,
                                     eos_id=run["eos_id"], ban=ban)[0][0].tolist()
        finally:
            m.ops, m.GRAPH_ROUNDS = spy._base, True
        rows = torch.cat(spy.rows)
        assert rows.shape[0] == GEN and rows.argmax(dim=-1).tolist() == out, "a token is not the arg-max of its banned row"
        assert spy.seen == [out[:c] for c in range(GEN)], "a step did not see the text so far"
        V = rows.shape[1]
        for c in range(GEN):                                              # the rows carry -inf exactly where the oracle forbids
            bad = sorted(t for t in bo.forbidden(out[:c], ban) if 0 <= t < V)
            assert torch.isinf(rows[c]).nonzero().view(-1).tolist() == bad, c
        _ref[family, name, ban] = (out, rows)
    return _ref[family, name, ban]


def explained(text, n, ref, rows, tol, what):
    """``text[:n]`` is ``ref`` up to its first difference, and there both tokens lie within ``tol`` of the best entry of the
    device's vanilla row.  Returns the number of columns that agree."""
    n = min(n, len(ref))
    diff = [c for c in range(n) if text[c] != ref[c]]
    if not diff:
        return n
    c = diff[0]
    top, took, other = float(rows[c].max()), float(rows[c, ref[c]]), float(rows[c, text[c]])
    print(f"{what}: parts at column {c}: {text[c]} at {other}, the device's vanilla run {ref[c]} at {took}; bound {tol}")
    assert took == top and top - other < tol, what
    return c


def glide_loop(family, name, loop, ban, graphs):
    run, m = gk.model_of(family, name)
    ids, pl = run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda")
    kw = dict(max_gen_len=GEN, eos_id=run["eos_id"], ban=ban)
    states = []
    begin = {"vanilla": "begin_vanilla_decode", "chain": "begin_chain_decode", "magicdec": "begin_chain_decode",
             "tree": "begin_tree_decode"}[loop]
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
        else:
            out, count, num, _, _ = m.tree_spec_generate(ids, pl, tree_shape=hb.tree_shape_of(run, name), **kw)
            got = SimpleNamespace(out=out[0].tolist(), n=int(count) + int(num))        # (the tree loop's num starts at 1)
    finally:
        delattr(m, begin)
        m.GRAPH_ROUNDS = True
    st = states[0]
    assert st.ban is not None and st.ban.cfg == ban
    if loop in ("vanilla", "tree"):                                       # (the chain rounds are not captured)
        assert (st.replayer.captures > 0 and not st.replayer.disabled) == bool(graphs), "replayed / eager as asked"
    return got


def run_loop(family, name, loop, ban, graphs):
    if loop == "lookup1":
        return gk.lookup(family, name, graphs=graphs, ban=ban)
    if loop == "lookup2":
        return gt.tree_lookup(family, name, graphs=graphs, b=2, tier_sized=not graphs, ban=ban)
    return glide_loop(family, name, loop, ban, graphs)


@pytest.mark.parametrize("family,name", RUNS)
def test_every_loop_eager_and_replayed_gives_the_banned_text(family, name):
    ban = Ban(no_repeat_ngram=3)
    run, m = gk.model_of(family, name)
    tol = sr.TOL[run["dtype"]]
    plain, _ = gk.vanilla(family, name)
    ref, rows = device_vanilla(family, name, ban)
    assert bo.repeats(plain, 3) is not None and bo.repeats(ref, 3) is None and ref != plain
    host = hb.run_loop(family, name, "vanilla", ban).out
    same = explained(host, GEN, ref, rows, tol, (name, "the host oracle's text"))
    assert same >= 24
    best = rows.topk(2, dim=-1).values
    exact = float((best[:, 0] - best[:, 1]).min()) >= tol                 # no row of the device's run is a near-tie
    print(f"{name}: the host oracle's text agrees on {same} columns; smallest top-2 margin of the device's banned rows "
          f"{float((best[:, 0] - best[:, 1]).min()):.4f}, bound {tol}")
    for loop in ("vanilla", "chain", "tree", "lookup1", "lookup2"):
        got = {graphs: run_loop(family, name, loop, ban, graphs) for graphs in (False, True)}
        for graphs, g in got.items():
            n = min(g.n, GEN)
            assert n >= GEN - 24, (loop, graphs, n)
            upto = explained(g.out, n, ref, rows, tol, (name, loop, "replayed" if graphs else "eager"))
            assert upto >= 24 and bo.repeats(g.out[:n], 3) is None, (loop, graphs)
            assert upto == n or not exact, (loop, graphs)
        n = min(got[True].n, got[False].n, GEN)                          # replayed against launch by launch: the same text
        assert got[True].n == got[False].n and got[True].out[:n] == got[False].out[:n], loop


def test_magicdec_on_a_long_prompt():
    """The fourth loop needs a prompt beyond its streaming window: the `mixed` run behind a 1030-token prompt."""
    family, name = "llama", "mixed@1030"
    run, m = gk.model_of(family, name)
    tol = sr.TOL[run["dtype"]]
    ban = Ban(no_repeat_ngram=2)
    plain, _ = gk.vanilla(family, name)
    ref, rows = device_vanilla(family, name, ban)
    assert bo.repeats(plain, 2) is not None and bo.repeats(ref, 2) is None
    for loop in ("magicdec", "chain"):
        g = glide_loop(family, name, loop, ban, graphs=True)
        n = min(g.n, GEN)
        assert n >= GEN - 8 and explained(g.out, n, ref, rows, tol, (name, loop)) >= 24 and bo.repeats(g.out[:n], 2) is None, loop


def test_sequences_and_bigrams_on_the_mixed_run():
    family, name = "llama", "mixed"
    run, m = gk.model_of(family, name)
    tol = sr.TOL[run["dtype"]]
    plain, _ = gk.vanilla(family, name)
    ban = Ban(no_repeat_ngram=2, sequences=[plain[5:8], [plain[1]]])
    ref, rows = device_vanilla(family, name, ban)
    assert ref[0] == plain[0] and ref[1] != plain[1]
    assert bo.repeats(ref, 2) is None and plain[1] not in ref and all(ref[c:c + 3] != plain[5:8] for c in range(GEN - 2))
    for loop in ("chain", "tree", "lookup2"):
        for graphs in (False, True):
            g = run_loop(family, name, loop, ban, graphs)
            n = min(g.n, GEN)
            assert explained(g.out, n, ref, rows, tol, (loop, graphs)) >= 24 and bo.repeats(g.out[:n], 2) is None
            assert plain[1] not in g.out[:n]
