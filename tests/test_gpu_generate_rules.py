"""All six rules on the target's logits at once (``longspec_amd/target_rules.py``) on the HIP kernels: the greedy all-on
configuration of tests/test_host_generate_rules_parity.py -- penalties with a bias entry, log-probs, a stop with ``min_tokens``
and a sequence, a no-repeat n-gram ban, the parity guide -- on the device, every loop at 32 columns.  Rounds replayed from HIP
graphs leave the text, the log-prob buffers and the stop result of the launch-by-launch rounds, bit for bit; and the warm-up
rounds of ``prepare_tree_graphs`` put back every tensor the rules keep."""
import pytest
import torch

import test_gpu_generate_lookup as gk
import test_host_generate_guide as hg
import test_host_generate_logprobs as hl
import test_host_generate_rules_parity as hp

pytestmark = pytest.mark.gpu
GEN = hp.GEN
PAIRS = [(f, n, loop) for f, n, c, loop in hp.PAIRS if c == "greedy"]


def keywords(family, name):
    return hp.keywords(family, name, "greedy", hp.load()["settings"][f"{family}/{name}/greedy"])


def device_loop(family, name, loop, graphs, after_begin=None):
    """One loop on the device with all six keywords.  The launch-by-launch rounds of a loop that can replay get the size hints
    of the graph tier the replayed ones are captured for: attention's split count follows the hint, and the same round under
    two hints is two summation orders (tests/test_gpu_generate_lookup_tree.py)."""
    run, m = gk.model_of(family, name)
    ids, pl = run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda")
    kw = dict(max_gen_len=GEN, eos_id=run["eos_id"], **keywords(family, name))
    states, begin = [], hp.BEGIN[loop]
    orig, hints = getattr(m, begin), m._set_hints

    def wrapped(*a, **k):
        st = orig(*a, **k)
        states.append(st)
        if after_begin is not None:
            after_begin(m, st)
        if not graphs and hasattr(st, "replayer"):
            sized = st.replayer.hints(m._tier_bound(1, st.replayer.total))
            m._set_hints = lambda t, d: hints(*sized)
        return st

    setattr(m, begin, wrapped)
    m.GRAPH_ROUNDS = graphs
    try:
        if loop == "vanilla":
            out = m.vanilla_generate(ids, pl, **kw)[0]
        elif loop == "chain":
            out = m.spec_generate(ids, pl, gamma=hg.G, **kw)[0]
        elif loop == "magicdec":
            out = m.magicdec_generate(ids, pl, gamma=3, **kw)[0]
        elif loop == "tree":
            out = m.tree_spec_generate(ids, pl, tree_shape=hg.tree_shape_of(run, name), **kw)[0]
        else:
            out = m.lookup_generate(ids, pl, gamma=hg.G, max_ngram=3, min_ngram=1, branches=int(loop[-1]), **kw)[0]
    finally:
        delattr(m, begin)
        if "_set_hints" in vars(m):
            del m._set_hints
        m.GRAPH_ROUNDS = True
    st, lp, ls = states[0], m.last_logprobs, m.last_stop
    assert st.rules is not None and st.guide is not None and st.ban is not None and st.stop.min_tokens > 0 \
        and st.penalties is not None and st.logprobs is lp and st.sampling is None
    if hasattr(st, "replayer"):                                           # (the glide chain rounds are not captured)
        assert (st.replayer.captures > 0 and not st.replayer.disabled) == bool(graphs), "replayed / eager as asked"
    return dict(out=out.cpu(), lp=[t.clone().cpu() for t in (lp.token, lp.top, lp.top_ids)],
                stop=[t.clone().cpu() for t in (ls.length, ls.which, ls.match_start)])


@pytest.mark.parametrize("family,name,loop", PAIRS)
def test_replayed_rounds_leave_what_launch_by_launch_rounds_leave(family, name, loop):
    eager, replayed = device_loop(family, name, loop, graphs=False), device_loop(family, name, loop, graphs=True)
    assert torch.equal(eager["out"], replayed["out"]), "text"
    for what in ("lp", "stop"):
        for x, y in zip(eager[what], replayed[what]):
            assert torch.equal(hl.bits(x), hl.bits(y)), what
    assert int((~torch.isnan(eager["lp"][0])).sum()) >= 8, "the log-prob buffers hold the text's columns"


def test_prepare_tree_graphs_puts_back_every_tensor_the_rules_keep():
    seen = {}

    def prepare(m, st):
        tensors = st.rules.state_tensors() + [st.output_ids]
        assert len(tensors) == 7 and st.use_graphs          # token state, stop state, three log-prob buffers, guide state; the text
        before = [t.clone() for t in tensors]
        m.prepare_tree_graphs(st)
        torch.cuda.synchronize()
        seen["captured"] = [st.replayer.captured(a) for a in range(1, st.gamma + 2)]
        seen["same"] = [torch.equal(hl.bits(x), hl.bits(y)) for x, y in zip(before, tensors)]

    device_loop("llama", "mixed", "tree", graphs=True, after_begin=prepare)
    assert all(seen["captured"]), "every accepted-token count was warmed up and captured"
    assert all(seen["same"]), seen["same"]
