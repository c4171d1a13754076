"""``graphs._pin_generator_state``: torch creates the default generator's capture state at the first capture and keeps it while
a graph lives.  The loops capture inside ``torch.inference_mode``; created there the state is a pair of inference tensors, and
a caller's own capture or replay OUTSIDE inference mode fails on their in-place update while one of the loops' graphs is alive.
The replayer pins the state as ordinary tensors in front of a device's first capture.  Run alone, the loop's capture below is
the process's first, which is the order that failed before the pin existed."""
import pytest
import torch

from test_gpu_generate_sampled import build
from test_host_generate_sampled import get_run


def test_stand_in_streams_are_left_alone():
    """The recording stand-ins of tests/test_graph_replay.py have no generator behind them: nothing is captured for them."""
    from longspec_amd import graphs
    before = dict(graphs._pinned)
    graphs._pin_generator_state(object())
    graphs._pin_generator_state(None)
    assert graphs._pinned == before


@pytest.mark.gpu
def test_a_callers_graph_outside_inference_mode_works_while_a_loops_graph_is_alive():
    from longspec_amd import graphs, ops
    run = get_run("llama", "mixed")
    m = build(run)
    m.GRAPH_AFTER = 0
    states = []
    orig = m.begin_tree_decode
    m.begin_tree_decode = lambda *a, **k: states.append(orig(*a, **k)) or states[-1]
    out, _, _, _, _ = m.tree_spec_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"),
                                           tree_shape=run["tree_shape"], max_gen_len=run["max_gen_len"], eos_id=run["eos_id"])
    assert torch.equal(out.cpu(), run["tree_out"])
    st = states[0]
    assert st.replayer.captures > 0 and not st.replayer.disabled, "no round was captured: the test shows nothing"
    assert any(st.replayer.captured(k) for k in st.replayer.entries), "no graph of the loop is alive"
    pinned = graphs._pinned[torch.cuda.current_device()]
    assert isinstance(pinned, tuple), f"the capture state was not pinned: {pinned!r}"
    # a caller's own graph around an operator, captured and replayed outside inference mode
    assert not torch.is_inference_mode_enabled()
    x = torch.randn(5, 1000, device="cuda").half()
    want = x.float().argmax(dim=-1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.argmax_rows(x)                                            # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=side):
        got = ops.argmax_rows(x)
    for _ in range(2):
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, want)
    # and the loop's graphs still replay inside inference mode
    out2, _, _, _, _ = m.tree_spec_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"),
                                            tree_shape=run["tree_shape"], max_gen_len=run["max_gen_len"], eos_id=run["eos_id"])
    assert torch.equal(out2.cpu(), run["tree_out"])
