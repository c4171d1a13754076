"""All six rules on the target's logits at once -- ``sampling=`` (in one of the two configurations), ``penalties=`` with a bias
entry, ``logprobs=``, ``stop=`` with ``min_tokens > 0`` and a sequence that fires inside the text, ``ban=`` with a no-repeat
n-gram and the parity ``guide=`` -- through every host loop on the CPU oracle, on toy runs of test_host_generate_guide.py at 32
columns, against a recording (tests/golden/rules_parity.json) made by ``record()`` below BEFORE the rules moved out of the
loops into ``longspec_amd/target_rules.py``.  The oracle operators are deterministic, so everything a loop leaves behind -- the
text, the counters, the speculation mask, the three log-prob buffers, the stop result, the final penalty and guide states -- is
bit for bit the recording, the operators fetched are the same multiset, and the orders that matter hold:

* ``penalize_rows`` < ``stop_ban_rows`` < ``ban_rows`` < ``guide_rows`` < draw or arg-max < ``token_logprobs``;
* ``logprob_commit`` < ``stop_scan`` (the scan erases log-prob columns the commit wrote);
* ``token_state_add`` < ``guide_advance`` < ``stop_scan``.

``record()`` chose the rule settings (kept in the file's ``settings``) and checked them once: every loop runs two rounds or
more, the chain and the tree loop each have a round that accepts two tokens or more, and the stop fires behind column 0."""
import json
import os
from collections import Counter

import pytest
import torch

import guide_oracle as go
import test_host_generate_guide as hg
from longspec_amd import Ban, Logprobs, Penalties, Sampling, Stop
from test_host_generate_sampled import FP16

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rules_parity.json")
GEN = 32
RUNS = [("llama", "mixed"), ("llama", "mixed@1030"), ("qwen2_bf16", "qwen_bf16_g5")]
CONFIGS = ("greedy", "sampled")
BEGIN = {"vanilla": "begin_vanilla_decode", "chain": "begin_chain_decode", "magicdec": "begin_chain_decode",
         "tree": "begin_tree_decode", "lookup1": "begin_lookup_decode", "lookup2": "begin_lookup_decode"}
APPLY = ["penalize_rows", "stop_ban_rows", "ban_rows", "guide_rows", "pick", "token_logprobs"]
COMMIT = ("logprob_commit", "token_state_add", "guide_advance", "stop_scan")


class Spy(hg.Spy):
    """``hg.Spy`` that also keeps the names of the three operators ``hl.Spy`` wraps without naming them."""

    def token_logprobs(self, *a, **k):
        self.names.append("token_logprobs")
        return super().token_logprobs(*a, **k)

    def tree_collapse(self, *a, **k):
        self.names.append("tree_collapse")
        return super().tree_collapse(*a, **k)

    def chain_commit(self, *a, **k):
        self.names.append("chain_commit")
        return super().chain_commit(*a, **k)


def keywords(family, name, config, s):
    """The six keywords of a run from its recorded settings ``s``."""
    run, m = hg.model_of(family, name)
    kw = dict(penalties=Penalties(repetition=1.1, presence=0.2, bias={int(s["bias"][0]): float(s["bias"][1])}),
              logprobs=Logprobs(2), ban=Ban(no_repeat_ngram=2),
              guide=hg.parity_guide(run["cfg"].vocab_size, hg.eos_of(run, m), s["start"]))
    if s.get("stop_ids") is not None:
        kw["stop"] = Stop(token_ids=s["stop_ids"], sequences=[s["stop_seq"]] if s.get("stop_seq") else (),
                          min_tokens=s["min_tokens"])
    if config == "sampled":
        kw["sampling"] = Sampling(FP16["temperature"], FP16["top_k"], FP16["top_p"], s["seed"])
    return kw


def bits(t):
    return t.contiguous().view(torch.int32).tolist() if t.dtype == torch.float32 else t.tolist()


def run_pair(family, name, loop, kw):
    """One loop with ``kw`` under the spy: everything it leaves behind, as JSON values (floats as their bit patterns)."""
    run, m = hg.model_of(family, name)
    spy, states = Spy(go.ops), []
    begin = BEGIN[loop]
    orig = getattr(m, begin)
    setattr(m, begin, lambda *a, **k: states.append(orig(*a, **k)) or states[-1])
    saved, m.ops = m.ops, spy
    try:
        ids, pl = run["prompt"], torch.tensor([run["prompt_len"]])
        kw = dict(max_gen_len=GEN, eos_id=run["eos_id"], **kw)
        if loop == "vanilla":
            res = m.vanilla_generate(ids, pl, **kw)
        elif loop == "chain":
            res = m.spec_generate(ids, pl, gamma=hg.G, **kw)
        elif loop == "magicdec":
            res = m.magicdec_generate(ids, pl, gamma=3, **kw)
        elif loop == "tree":
            res = m.tree_spec_generate(ids, pl, tree_shape=hg.tree_shape_of(run, name), **kw)
        else:
            res = m.lookup_generate(ids, pl, gamma=hg.G, max_ngram=3, min_ngram=1, branches=int(loop[-1]), **kw)
    finally:
        m.ops = saved
        delattr(m, begin)
    st, lp, ls = states[0], m.last_logprobs, m.last_stop
    tree = loop in ("tree", "lookup2")
    rounds = [int(e[2][0]) for e in spy.events if e[0] == "tree"] if tree else \
        [int(e[1][0]) for e in spy.events if e[0] == "chain"]
    state = st.token_state[0]
    nz = state.nonzero().view(-1)
    return dict(out=res[0].tolist(), count=None if loop == "vanilla" else int(res[1]), num=int(res[1] if loop == "vanilla" else res[2]),
                spec_mask=None if loop == "vanilla" else res[4].tolist(),
                lp_token=bits(lp.token), lp_top=bits(lp.top), lp_top_ids=bits(lp.top_ids),
                stop=None if ls is None else [int(ls.length[0]), int(ls.which[0]), int(ls.match_start[0])],
                token_state=[[int(i), int(state[i])] for i in nz], guide_state=st.guide.state.tolist(),
                rounds=rounds, names=dict(sorted(Counter(spy.names).items())), order=list(spy.names))


def check_order(names, config, what):
    pick = "sample_rows" if config == "sampled" else "argmax_rows"
    seq = ["pick" if n == pick else n for n in names if n in APPLY or n == pick]
    seq = [n for i, n in enumerate(seq) if n != "pick" or (i and seq[i - 1] == "guide_rows")]     # (the drafter's arg-maxes)
    groups, cur = [], None
    for n in seq:
        if n == "penalize_rows":
            cur = []
            groups.append(cur)
        assert cur is not None, (what, "a rule in front of the penalties")
        cur.append(n)
    first = [n for n in APPLY if n != "pick"] if config == "greedy" else APPLY       # (the greedy first token: torch's arg-max)
    assert len(groups) >= 3 and groups[0] == first and all(g == APPLY for g in groups[1:]), (what, groups[:3])
    seq = [n for n in names if n in COMMIT]
    groups, cur = [], []
    for n in seq:
        cur.append(n)
        if n == "stop_scan":
            groups.append(cur)
            cur = []
    assert not cur and len(groups) >= 3, (what, "the stop scan comes last")
    assert groups[0] == ["token_state_add", "token_state_add", "guide_advance", "stop_scan"], (what, groups[0])   # prompt, first token
    for g in groups[1:]:
        assert sorted(g) == sorted(COMMIT) and g.index("token_state_add") < g.index("guide_advance"), (what, g)


def load(path=GOLDEN):
    with open(path) as f:
        return json.load(f)


PAIRS = [(family, name, config, loop) for family, name in RUNS for config in CONFIGS
         for loop in hg.loops_of(hg.get_run(family, name))]


@pytest.mark.parametrize("family,name,config,loop", PAIRS)
def test_every_loop_leaves_what_it_left_before_the_rules_moved(family, name, config, loop):
    gold = load()
    key = f"{family}/{name}/{config}"
    want = gold["records"][f"{key}/{loop}"]
    got = run_pair(family, name, loop, keywords(family, name, config, gold["settings"][key]))
    order = got.pop("order")
    for field in want:
        assert got[field] == want[field], (loop, field)
    assert set(got) == set(want)
    check_order(order, config, (key, loop))


def test_the_recording_shows_the_multi_token_commit_paths(path=GOLDEN):
    gold = load(path)
    assert sorted(gold["records"]) == sorted(f"{f}/{n}/{c}/{loop}" for f, n, c, loop in PAIRS)
    for key, rec in gold["records"].items():
        loop = key.rsplit("/", 1)[1]
        assert (rec["num"] if loop == "vanilla" else len(rec["rounds"])) >= 2, key
    for family, name in RUNS:
        for config in CONFIGS:
            recs = {loop: gold["records"][f"{family}/{name}/{config}/{loop}"] for loop in hg.loops_of(hg.get_run(family, name))}
            assert max(recs["chain"]["rounds"]) >= 2 and max(recs["tree"]["rounds"]) >= 2, (family, name, config)
            assert any(r["stop"][0] > 1 for r in recs.values()), (family, name, config)


def record(path=GOLDEN):
    """Choose the rule settings of every (run, configuration), check what the docstring says of them, run every loop and write
    the recording.  Run from a checkout of the commit to record (``python -c "import test_host_generate_rules_parity as t;
    t.record()"`` inside tests/)."""
    settings, records = {}, {}
    for family, name in RUNS:
        run, m = hg.model_of(family, name)
        eos = hg.eos_of(run, m)
        plain = hg.run_loop(family, name, "vanilla", None, gen=GEN).out
        start = next(s for s in (plain[0] % 2, 1 - plain[0] % 2) if not hg.in_parity(plain, s, eos))
        for config in CONFIGS:
            key = f"{family}/{name}/{config}"
            for seed in range(1, 200) if config == "sampled" else [0]:
                s = dict(start=start, bias=[plain[2], -3.0], seed=seed)
                text = run_pair(family, name, "vanilla", keywords(family, name, config, s))["out"][0]
                c0 = next(c for c in range(2, 8) if text[c] not in text[:c])
                s.update(stop_ids=[text[c0]], min_tokens=c0 + 4)
                text = run_pair(family, name, "vanilla", keywords(family, name, config, s))["out"][0]
                assert text[c0] != s["stop_ids"][0], "the min_tokens ban must bite"
                c = next((c for c in range(22, 29) if s["stop_ids"][0] not in text[s["min_tokens"]:c + 1]), None)
                if c is None:
                    continue
                s["stop_seq"] = text[c - 1:c + 1]
                kw = keywords(family, name, config, s)
                if all(max(run_pair(family, name, loop, kw)["rounds"]) >= 2 for loop in ("chain", "tree")):
                    break                     # (a seed under which both speculative loops accept a draft)
            else:
                raise AssertionError(f"{key}: no seed gives the chain and the tree loop a round of two")
            settings[key] = s
            for loop in hg.loops_of(run):
                rec = run_pair(family, name, loop, keywords(family, name, config, s))
                check_order(rec.pop("order"), config, (key, loop))
                records[f"{key}/{loop}"] = rec
                print(key, loop, "seed", s["seed"], "rounds", rec["rounds"], "stop", rec["stop"])
    with open(path, "w") as f:
        json.dump(dict(settings=settings, records=records), f, separators=(",", ":"))
        f.write("\n")
    test_the_recording_shows_the_multi_token_commit_paths(path)
