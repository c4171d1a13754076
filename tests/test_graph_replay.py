"""The HIP-graph state machine of `vanilla_step` / `tree_round` / `prepare_tree_graphs` / `lookup_round` (longspec_amd/graphs.py)
without a GPU.

The CUDA primitives the graph code touches are replaced by recording fakes: a fake capture stores the device-function calls made
inside it WITHOUT running them (a stream capture records, it does not execute), a fake `replay` runs them again on the live decode
state and copies the result into the tensor the capture handed out.  The real loops then run on the CPU toy models with the
oracle's operators, as in tests/test_host_generate.py, with `use_graphs` forced on right behind `begin_*`.

tests/golden/graph_replay_trace.json is what this harness records on the code BEFORE a change to the graph path
(`python tests/test_graph_replay.py --record` with the parent commit's longspec_amd/llama_glide.py in place); it is never
re-recorded from the code it is meant to check."""
import json
import os
import warnings

import pytest
import torch

import cases
import lookup_oracle
import lookup_tree_oracle
import oracle_ops


def build(run, ops=oracle_ops):
    from longspec_amd.llama_glide import LlamaGlide
    m = LlamaGlide(run["cfg"], ops=ops, dtype=run.get("dtype", torch.float16))
    m.load_state_dict({**run["target_sd"], **{"glide." + k: v for k, v in run["draft_sd"].items()}}, strict=True)
    return m


TRACE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_replay_trace.json")
RUNS = {r["name"]: r for r in cases.generate_runs() if r["name"] in ("mixed", "gqa_mixed")}
TIER = 8            # mixed emits 59 tokens, gqa_mixed 35: the tree rounds cross seven and five tiers
STATE_NAMES = ("cache_lens", "target_cache_lens_for_draft", "draft_cache_lens", "tree_mask", "all_spec", "history_logp_sum",
               "acc_pad", "output_ids", "emitted_dev", "spec_mask")


class Fakes:
    """Recording stand-ins of torch.cuda.{Stream, stream, current_stream, CUDAGraph, graph, is_current_stream_capturing}.
    `fail = {"wait" | "capture" | "replay": n}` raises from the n-th such call, once."""

    def __init__(self):
        fk = self
        self.events = []                 # [kind, key, [target hint, draft hint]] (+ the pool's graph number for a capture)
        self.hints = None                # the pair of the last _set_hints
        self.runs = 0                    # device-function executions (eager + warm + replayed)
        self.counts = {"wait": 0, "capture": 0, "replay": 0}
        self.fail = {}
        self.stuck_capturing = False     # a failing capture goes on reporting "capturing"
        self.capturing = None            # (graph, pool) while a fake capture is open
        self.n_graphs = 0
        self.like = {}                   # device function -> its last result: the shape a capture's result tensor takes

        class Stream:
            def wait_stream(self, other):
                fk.tick("wait")

        class StreamCtx:
            def __init__(self, stream):
                self.stream = stream

            def __enter__(self):
                fk.stack.append(self.stream)

            def __exit__(self, *exc):
                fk.stack.pop()

        class CUDAGraph:
            def __init__(self):
                self.calls, self.serial = [], fk.n_graphs
                fk.n_graphs += 1

            def pool(self):
                return ("pool", self.serial)

            def replay(self):
                fk.tick("replay")
                for fn, args, key, out in self.calls:
                    fk.events.append(["replay", key, list(fk.hints)])
                    fk.runs += 1
                    r = fn(*args)
                    if out is not None:
                        out.copy_(r)

        class GraphCtx:
            def __init__(self, graph, stream=None, pool=None):
                self.graph, self.stream, self.pool = graph, stream, pool

            def __enter__(self):
                assert self.stream is not None and self.stream is not fk.main, "capture on the capture stream"
                if fk.stuck_capturing:
                    fk.capturing = (self.graph, self.pool)
                fk.tick("capture")
                fk.capturing = (self.graph, self.pool)
                fk.stack.append(self.stream)

            def __exit__(self, *exc):
                fk.stack.pop()
                fk.capturing = None

        self.main = Stream()
        self.stack = [self.main]
        self.Stream, self.stream, self.CUDAGraph, self.graph = Stream, StreamCtx, CUDAGraph, GraphCtx

    def tick(self, what):
        self.counts[what] += 1
        if self.fail.get(what) == self.counts[what]:
            raise RuntimeError(f"injected: {what} {self.counts[what]} failed")

    def spy_hints(self, m):
        orig = m._set_hints

        def set_hints(target_bound, draft_bound):
            self.hints = (target_bound, draft_bound)
            return orig(target_bound, draft_bound)

        m._set_hints = set_hints

    def spy_device(self, m, name, key_of):
        """Wrap the device function `m.<name>`: classify every call by the stream it is issued on."""
        orig = getattr(m, name)

        def device(*args):
            key = key_of(*args)
            if self.capturing is not None:
                graph, pool = self.capturing
                self.events.append(["capture", key, list(self.hints), None if pool is None else pool[1]])
                last = self.like.get(name)
                out = torch.empty_like(last) if torch.is_tensor(last) else None
                graph.calls.append((orig, args, key, out))
                return out
            self.events.append(["warm" if self.stack[-1] is not self.main else "eager", key, list(self.hints)])
            self.runs += 1
            self.like[name] = r = orig(*args)
            return r

        setattr(m, name, device)


@pytest.fixture
def fakes(monkeypatch):
    fk = Fakes()
    for name in ("Stream", "stream", "CUDAGraph", "graph"):
        monkeypatch.setattr(torch.cuda, name, getattr(fk, name))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: fk.stack[-1])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: fk.capturing is not None)
    return fk


def _count_calls(m, name, calls):
    orig = getattr(m, name)

    def counted(*a, **k):
        calls[name] = calls.get(name, 0) + 1
        return orig(*a, **k)

    setattr(m, name, counted)


def _boom(*a, **k):
    raise RuntimeError("injected: tier sizing failed")


def run_tree(fk, run, prepare=False, tier_fails=False):
    """tree_spec_generate of a golden run through the real loop, graphs forced on behind begin_tree_decode."""
    m = build(run)
    m.GRAPH_AFTER, m.GRAPH_TIER = 0, TIER
    fk.spy_hints(m)
    fk.spy_device(m, "_round_device", lambda st, a: a)
    calls, states, begin = {}, [], m.begin_tree_decode
    _count_calls(m, "tree_round", calls)

    def begin_with_graphs(*a, **k):
        st = begin(*a, **k)
        st.use_graphs = True
        states.append(st)
        if tier_fails:
            m._tier_bound = _boom
        if prepare:
            snap = {n: getattr(st, n).clone() for n in STATE_NAMES}
            m.prepare_tree_graphs(st)
            prepared = [e[:2] for e in fk.events]
            assert prepared == [[k, a] for a in range(1, st.gamma + 2) for k in ("warm", "capture")], prepared
            for n in STATE_NAMES:                       # the warm-up rounds ran on a snapshot: restored bit for bit
                assert torch.equal(getattr(st, n), snap[n]), n
            assert (st.a, st.emitted, st.count, st.num) == (1, 1, 0, st.bsz)
            fk.runs = 0
        return st

    m.begin_tree_decode = begin_with_graphs
    out, count, num, _, _ = m.tree_spec_generate(run["prompt"], torch.tensor([run["prompt_len"]]), tree_shape=run["tree_shape"],
                                                 max_gen_len=run["max_gen_len"], eos_id=run["eos_id"])
    return dict(out=out, count=int(count), num=int(num), st=states[0], rounds=calls["tree_round"])


def run_vanilla(fk, run, tier_fails=False):
    m = build(run)
    m.GRAPH_AFTER, m.GRAPH_TIER = 0, TIER
    fk.spy_hints(m)
    fk.spy_device(m, "_vanilla_device", lambda vs: "step")
    calls, states, begin = {}, [], m.begin_vanilla_decode
    _count_calls(m, "vanilla_step", calls)

    def begin_with_graphs(*a, **k):
        vs = begin(*a, **k)
        vs.use_graphs = True
        states.append(vs)
        if tier_fails:
            m._tier_bound = _boom
        return vs

    m.begin_vanilla_decode = begin_with_graphs
    out, num, _ = m.vanilla_generate(run["prompt"], torch.tensor([run["prompt_len"]]), max_gen_len=run["max_gen_len"],
                                     eos_id=run["eos_id"])
    return dict(out=out, num=int(num), vs=states[0], steps=calls["vanilla_step"])


def run_lookup(fk, run, branches, tier_fails=False):
    """lookup_generate of a golden run through the real loop (branches=1: the chain round, 3: the tree round), graphs forced on
    behind begin_lookup_decode."""
    m = build(run, ops=lookup_oracle.ops if branches == 1 else lookup_tree_oracle.ops)
    m.GRAPH_AFTER, m.GRAPH_TIER = 0, TIER
    fk.spy_hints(m)
    if branches == 1:
        fk.spy_device(m, "_lookup_device", lambda st: "round")
    else:
        fk.spy_device(m, "_lookup_tree_device", lambda st, a: a)
    calls, states, begin = {}, [], m.begin_lookup_decode
    _count_calls(m, "lookup_round", calls)

    def begin_with_graphs(*a, **k):
        st = begin(*a, **k)
        st.use_graphs = True
        states.append(st)
        if tier_fails:
            m._tier_bound = _boom
        return st

    m.begin_lookup_decode = begin_with_graphs
    out, count, num, _, _ = m.lookup_generate(run["prompt"], torch.tensor([run["prompt_len"]]), gamma=4, max_ngram=3, min_ngram=1,
                                              max_gen_len=run["max_gen_len"], eos_id=run["eos_id"], branches=branches)
    return dict(out=out, count=int(count), num=int(num), st=states[0], rounds=calls["lookup_round"])


LOOKUP_BRANCHES = {"lookup": 1, "lookup_tree": 3}
SCENARIOS = [(name, kind) for name in RUNS for kind in ("tree", "tree_prepared", "vanilla")]
SCENARIOS += [(name, kind) for name in RUNS for kind in LOOKUP_BRANCHES]      # (behind the others: the trace file's key order)


def _check_lookup_text(r, run):
    """The text is the vanilla text over the columns the loop wrote (the vanilla golden is cut behind its first EOS)."""
    n = min(r["st"].emitted, run["vanilla_num"] + 1)
    assert n > 1 and torch.equal(r["out"][:, :n], run["vanilla_out"][:, :n])
    assert r["num"] == r["rounds"] and r["count"] == r["st"].emitted - 1 - r["rounds"]


def scenario(fk, name, kind):
    """One golden run with every round / step on the graph path; returns (result, what the trace file holds of it)."""
    run = RUNS[name]
    if kind == "vanilla":
        r = run_vanilla(fk, run)
        return r, {"events": fk.events, "graph_captures": r["vs"].graph_captures}
    if kind in LOOKUP_BRANCHES:
        r = run_lookup(fk, run, LOOKUP_BRANCHES[kind])
        return r, {"events": fk.events, "graph_tiers": r["st"].graph_tiers, "graph_captures": r["st"].graph_captures}
    r = run_tree(fk, run, prepare=kind == "tree_prepared")
    return r, {"events": fk.events, "graph_tiers": r["st"].graph_tiers, "graph_captures": r["st"].graph_captures}


@pytest.mark.parametrize("name,kind", SCENARIOS, ids=lambda x: str(x))
def test_graph_path_issues_the_recorded_trace(fakes, name, kind):
    """Every warm-up, capture, replay and eager run, in order, with the hints set in front of it, the pool a capture shares and
    the final counters: as recorded before the graph mechanics moved into one class.  The tokens are the golden's, so a replayed
    round really runs the round again."""
    run = RUNS[name]
    r, got = scenario(fakes, name, kind)
    if kind == "vanilla":
        assert torch.equal(r["out"], run["vanilla_out"]) and r["num"] == run["vanilla_num"]
        assert r["vs"].use_graphs is True and fakes.runs == r["steps"]
    elif kind in LOOKUP_BRANCHES:
        _check_lookup_text(r, run)
        assert r["st"].use_graphs is True and r["st"].graphs is not False and fakes.runs == r["rounds"]
        assert r["st"].graph_tiers >= 3
    else:
        assert torch.equal(r["out"], run["tree_out"])
        assert (r["count"], r["num"]) == (run["tree_count"], run["tree_num"])
        assert r["st"].graphs is not False and fakes.runs == r["rounds"]
        assert r["st"].graph_tiers >= 3
    kinds = {e[0] for e in got["events"]}
    assert {"warm", "capture", "replay"} <= kinds
    with open(TRACE) as f:
        want = json.load(f)[f"{name}/{kind}"]
    assert json.loads(json.dumps(got)) == want


FAILURES = {"tier_bound": dict(tier_fails=True), "wait_before_the_warm_up": dict(fail={"wait": 1}),
            "wait_behind_the_warm_up": dict(fail={"wait": 2}), "capture": dict(fail={"capture": 1}),
            "third_replay": dict(fail={"replay": 3})}


def _run_failing(fk, loop, how):
    fk.fail = dict(how.get("fail", {}))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = loop(fk, RUNS["mixed"], tier_fails=how.get("tier_fails", False))
    eagerly = [x for x in w if "running eagerly" in str(x.message)]
    assert len(eagerly) == 1 and "injected" in str(eagerly[0].message), [str(x.message) for x in w]
    return r


def _check_stream_wait(fk, where):
    if where == "wait_behind_the_warm_up":
        # the warm-up was issued on the capture stream: the main stream waits for it before it goes on
        assert fk.counts["wait"] == 3 and [e[0] for e in fk.events].count("warm") == 1


@pytest.mark.parametrize("where", list(FAILURES))
def test_tree_round_runs_every_round_once_when_its_graph_fails(fakes, where):
    """A failure anywhere in the graph path of a round: one warning, replay off, and the generation is the eager one -- every
    round executed exactly once.  Behind the warm-up the round has ALREADY run on the capture stream: its result is used (the
    code before GraphReplayer ran the round a second time on the advanced state there -- this test counted 31 executions for
    30 rounds on it -- and let a failing tier sizing escape from tree_round)."""
    run = RUNS["mixed"]
    r = _run_failing(fakes, run_tree, FAILURES[where])
    assert fakes.runs == r["rounds"], (fakes.runs, r["rounds"])
    assert torch.equal(r["out"], run["tree_out"])
    assert (r["count"], r["num"]) == (run["tree_count"], run["tree_num"])
    assert r["st"].graphs is False
    assert fakes.events[-1][0] == "eager"
    _check_stream_wait(fakes, where)


@pytest.mark.parametrize("where", list(FAILURES))
def test_vanilla_step_decodes_every_token_once_when_its_graph_fails(fakes, where):
    run = RUNS["mixed"]
    r = _run_failing(fakes, run_vanilla, FAILURES[where])
    assert fakes.runs == r["steps"], (fakes.runs, r["steps"])
    assert torch.equal(r["out"], run["vanilla_out"]) and r["num"] == run["vanilla_num"]
    assert r["vs"].use_graphs is False
    assert fakes.events[-1][0] == "eager"
    _check_stream_wait(fakes, where)


def _lookup_loop(branches):
    return lambda fk, run, tier_fails=False: run_lookup(fk, run, branches, tier_fails=tier_fails)


@pytest.mark.parametrize("kind", list(LOOKUP_BRANCHES))
@pytest.mark.parametrize("where", list(FAILURES))
def test_lookup_round_runs_every_round_once_when_its_graph_fails(fakes, where, kind):
    """The two failure tests above on the lookup loops.  The chain round switches ``use_graphs`` off as ``vanilla_step`` does;
    the tree round leaves it to ``replayer.disabled`` as ``tree_round`` does."""
    run = RUNS["mixed"]
    r = _run_failing(fakes, _lookup_loop(LOOKUP_BRANCHES[kind]), FAILURES[where])
    assert fakes.runs == r["rounds"], (fakes.runs, r["rounds"])
    _check_lookup_text(r, run)
    assert fakes.events[-1][0] == "eager"
    assert r["st"].replayer.disabled is True and r["st"].graphs is False
    assert r["st"].use_graphs is (kind == "lookup_tree")
    _check_stream_wait(fakes, where)


@pytest.mark.parametrize("loop", [run_tree, run_vanilla, _lookup_loop(1), _lookup_loop(3)],
                         ids=["tree", "vanilla", "lookup", "lookup_tree"])
def test_a_failure_inside_a_capture_propagates(fakes, loop):
    """While the stream is capturing nothing can run eagerly: the exception is the caller's."""
    fakes.fail, fakes.stuck_capturing = {"capture": 1}, True
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(RuntimeError, match="injected: capture 1 failed"):
            loop(fakes, RUNS["gqa_mixed" if loop in (run_tree, run_vanilla) else "mixed"])


def test_the_eager_loops_give_the_goldens_the_failure_tests_compare_with():
    """`graphs off` on the same harness: the goldens above are the eager generations."""
    run = RUNS["mixed"]
    fk = Fakes()
    m = build(run)
    fk.spy_hints(m)
    fk.spy_device(m, "_round_device", lambda st, a: a)
    fk.spy_device(m, "_vanilla_device", lambda vs: "step")
    pl = torch.tensor([run["prompt_len"]])
    out, count, num, _, _ = m.tree_spec_generate(run["prompt"], pl, tree_shape=run["tree_shape"], max_gen_len=run["max_gen_len"],
                                                 eos_id=run["eos_id"])
    assert torch.equal(out, run["tree_out"]) and (int(count), int(num)) == (run["tree_count"], run["tree_num"])
    v_out, v_num, _ = m.vanilla_generate(run["prompt"], pl, max_gen_len=run["max_gen_len"], eos_id=run["eos_id"])
    assert torch.equal(v_out, run["vanilla_out"]) and v_num == run["vanilla_num"]
    assert {e[0] for e in fk.events} == {"eager"}


if __name__ == "__main__":
    import sys
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_graph_replay.py --record   (on the parent commit's code only)"
    mp = pytest.MonkeyPatch()
    trace = {}
    for name, kind in SCENARIOS:
        fk = Fakes()
        for attr in ("Stream", "stream", "CUDAGraph", "graph"):
            mp.setattr(torch.cuda, attr, getattr(fk, attr))
        mp.setattr(torch.cuda, "current_stream", lambda *a, fk=fk: fk.stack[-1])
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda fk=fk: fk.capturing is not None)
        trace[f"{name}/{kind}"] = scenario(fk, name, kind)[1]
    mp.undo()
    with open(TRACE, "w") as f:
        json.dump(trace, f, separators=(",", ":"))
        f.write("\n")
