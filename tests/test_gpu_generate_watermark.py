"""``watermark=`` end to end on the HIP kernels: the toy runs of tests/test_host_generate_watermark.py on the device.  The device's
watermarked vanilla run, launch by launch under a spy that keeps every row ``ops.watermark_rows`` handed back, is the host
oracle's text up to a column the project's 16-bit near-tie bound explains; every loop -- vanilla, chain, tree, lookup with one
branch and with two, launch by launch and replayed from HIP graphs -- is that device text up to such a column, and exactly that
text where no row of the device's run is a near-tie.  ``Watermark.detect`` on the device counts what the host counts."""
from types import SimpleNamespace

import pytest
import torch

import ban_oracle as bo
import sampled_runs as sr
import test_gpu_generate_ban as gb
import test_gpu_generate_lookup as gk
import test_gpu_generate_lookup_tree as gt
import test_host_generate_watermark as hw
import watermark_oracle as wo
from longspec_amd import Watermark

pytestmark = pytest.mark.gpu
GEN, G = gk.GEN, 4
RUNS = hw.RUNS
explained = gb.explained
_ref = {}
# The marks of the host tests, under a key of this file's own.  Under HARD x + 1000 lies on a grid of 0.5 (fp16) or 4 (bf16):
# most green ids of a row tie exactly, the arg-max takes the lowest id of the top bucket, and a last-bit difference between two
# passes can move an id across a bucket edge, which no near-tie bound explains.  The key is the first of those that meet the
# host tests' conditions on the plain texts (no mark on the plain texts, no EOS in a marked one) under which the device's runs
# hold no such column in front of column 24.
KEY = 345
HARD, SOFT = Watermark(KEY, 0.5, 1000.0), Watermark(KEY, 0.25, 2.0)


class MarkSpy:
    """The device's operator module with every row ``watermark_rows`` returned and the committed text it saw kept (host reads:
    for launch-by-launch runs only); row 0 of every call is checked against the oracle bit for bit."""

    def __init__(self):
        from longspec_amd import ops
        self._base, self.rows, self.seen = ops, [], []

    def __getattr__(self, name):
        return getattr(self._base, name)

    def watermark_rows(self, logits, table, output_ids, base=None, base_sub=None, base_add=0, **kw):
        before = logits.reshape(-1, logits.shape[-1])[:1].clone()
        out = self._base.watermark_rows(logits, table, output_ids, base=base, base_sub=base_sub, base_add=base_add, **kw)
        cpu = lambda t: None if t is None else t.cpu()
        text = bo.row_texts(1, 1, cpu(output_ids), cpu(base), cpu(base_sub), base_add)[0][0]
        want = wo.watermark_rows(before.cpu(), table.cpu(), torch.tensor([text + [0]]), base=torch.tensor([len(text)], dtype=torch.int32))
        got = out.reshape(-1, out.shape[-1])[:1].cpu()
        assert torch.equal(want.view(torch.int16), got.view(torch.int16)), "row 0 is not the oracle's marked row"
        self.seen.append(text)
        self.rows.append(got.float())
        return out


def device_vanilla(family, name, wm):
    """(text, the marked row of every column) of the device's launch-by-launch vanilla run under ``wm``."""
    if (family, name, wm) not in _ref:
        run, m = gk.model_of(family, name)
        spy = MarkSpy()
        m.ops, m.GRAPH_ROUNDS = spy, False
        try:
            out = m.vanilla_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"), max_gen_len=GEN,
                                     eos_id=run["eos_id"], watermark=wm)[0][0].tolist()
        finally:
            m.ops, m.GRAPH_ROUNDS = spy._base, True
        rows = torch.cat(spy.rows)
        assert rows.shape[0] == GEN and rows.argmax(dim=-1).tolist() == out, "a token is not the arg-max of its marked row"
        assert spy.seen == [out[:c] for c in range(GEN)], "a step did not see the text so far"
        _ref[family, name, wm] = (out, rows)
    return _ref[family, name, wm]


def glide_loop(family, name, loop, wm, graphs):
    run, m = gk.model_of(family, name)
    ids, pl = run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda")
    kw = dict(max_gen_len=GEN, eos_id=run["eos_id"], watermark=wm)
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
            out, count, num, _, _ = m.tree_spec_generate(ids, pl, tree_shape=hw.tree_shape_of(run, name), **kw)
            got = SimpleNamespace(out=out[0].tolist(), n=int(count) + int(num))        # (the tree loop's num starts at 1)
    finally:
        delattr(m, begin)
        m.GRAPH_ROUNDS = True
    st = states[0]
    assert st.watermark is not None and st.watermark.cfg == wm
    if loop in ("vanilla", "tree"):                                       # (the chain rounds are not captured)
        assert (st.replayer.captures > 0 and not st.replayer.disabled) == bool(graphs), "replayed / eager as asked"
    return got


def run_loop(family, name, loop, wm, graphs):
    if loop == "lookup1":
        return gk.lookup(family, name, graphs=graphs, watermark=wm)
    if loop == "lookup2":
        return gt.tree_lookup(family, name, graphs=graphs, b=2, tier_sized=not graphs, watermark=wm)
    return glide_loop(family, name, loop, wm, graphs)


@pytest.mark.parametrize("family,name", RUNS)
@pytest.mark.parametrize("wm", [HARD, SOFT], ids=["hard", "soft"])
def test_every_loop_eager_and_replayed_gives_the_watermarked_text(family, name, wm):
    run, m = gk.model_of(family, name)
    tol = sr.TOL[run["dtype"]]
    plain, _ = gk.vanilla(family, name)
    ref, rows = device_vanilla(family, name, wm)
    assert ref != plain
    on_host = wm.detect(torch.tensor(ref))
    on_device = wm.detect(torch.tensor(ref, device="cuda"))
    assert (int(on_device.scored[0]), int(on_device.green[0])) == (int(on_host.scored[0]), int(on_host.green[0])) == \
        wo.score(ref, wm.key, wm.gamma, wm.context)[:2]
    assert torch.equal(on_device.flags.cpu(), on_host.flags) and abs(float(on_device.z[0]) - float(on_host.z[0])) < 1e-12
    if wm is HARD:
        assert int(on_device.green[0]) == int(on_device.scored[0]) == GEN - 1 and float(on_device.z[0]) > 6
    host = hw.run_loop(family, name, "vanilla", wm).out
    same = explained(host, GEN, ref, rows, tol, (name, "the host oracle's text"))
    assert same >= 24
    best = rows.topk(2, dim=-1).values
    exact = float((best[:, 0] - best[:, 1]).min()) >= tol                 # no row of the device's run is a near-tie
    print(f"{name}: the host oracle's text agrees on {same} columns; smallest top-2 margin of the device's marked rows "
          f"{float((best[:, 0] - best[:, 1]).min()):.4f}, bound {tol}")
    for loop in ("vanilla", "chain", "tree", "lookup1", "lookup2"):
        got = {graphs: run_loop(family, name, loop, wm, graphs) for graphs in (False, True)}
        for graphs, g in got.items():
            n = min(g.n, GEN)
            assert n >= GEN - 24, (loop, graphs, n)
            upto = explained(g.out, n, ref, rows, tol, (name, loop, "replayed" if graphs else "eager"))
            assert upto >= 24, (loop, graphs)
            if wm is HARD:
                d = wm.detect(torch.tensor(g.out[:upto], device="cuda"))
                assert int(d.green[0]) == int(d.scored[0]) == upto - 1, (loop, graphs)
            assert upto == n or not exact, (loop, graphs)
        n = min(got[True].n, got[False].n, GEN)                          # replayed against launch by launch: the same text
        assert got[True].n == got[False].n and got[True].out[:n] == got[False].out[:n], loop


def test_magicdec_on_a_long_prompt():
    """The fourth loop needs a prompt beyond its streaming window: the `mixed` run behind a 1030-token prompt."""
    family, name = "llama", "mixed@1030"
    run, m = gk.model_of(family, name)
    tol = sr.TOL[run["dtype"]]
    wm = SOFT
    plain, _ = gk.vanilla(family, name)
    ref, rows = device_vanilla(family, name, wm)
    assert ref != plain
    for loop in ("magicdec", "chain"):
        g = glide_loop(family, name, loop, wm, graphs=True)
        n = min(g.n, GEN)
        upto = explained(g.out, n, ref, rows, tol, (name, loop))
        assert n >= GEN - 24 and upto >= 24, loop
