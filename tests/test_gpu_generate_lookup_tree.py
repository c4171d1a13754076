"""``lookup_generate(branches=B)`` end to end on the HIP kernels: the toy runs of tests/test_gpu_generate_lookup.py on the device.
The expectation is the DEVICE's own vanilla text, recorded launch by launch -- exact where the run keeps the near-tie bound,
else explained by it (a copy of a branch may part from its twin by a 16-bit near-tie: either is a valid path) --, every round
drafts what the oracle drafts from the text as it stood, and the rounds replayed from HIP graphs give the bits of the
launch-by-launch rounds."""
from types import SimpleNamespace

import pytest
import torch

import lookup_tree_oracle as lt
import sampled_runs as sr
import stop_oracle as so
import test_gpu_generate_lookup as gk
import test_host_generate_logprobs as hl
import test_host_generate_penalized as hp
from longspec_amd import Logprobs, Penalties, Sampling, Stop
from test_host_generate_sampled import FP16

pytestmark = pytest.mark.gpu
GEN, G, B, MX, MN = gk.GEN, 4, 4, 3, 1


class Spy(gk.Spy):
    """``gk.Spy`` that keeps what the tree rounds drafted, from which text, and accepted (host reads: launch-by-launch runs only)."""

    def __init__(self):
        super().__init__()
        self.texts, self.slots, self.infos, self.chain_calls = [], [], [], 0

    def ngram_tree_draft(self, prompt_ids, input_len, output_ids, written, len_bound, gamma, branches, *a, **k):
        info = self._base.ngram_tree_draft(prompt_ids, input_len, output_ids, written, len_bound, gamma, branches, *a, **k)
        all_spec = a[2]
        self.texts.append(lt.text_of(prompt_ids.cpu(), input_len.cpu(), output_ids.cpu(), written.cpu(), 0))
        self.slots.append(all_spec[0, 1:].view(gamma, branches).t().tolist())
        self.infos.append([tuple(x) for x in info[0].tolist()])
        assert len(self.texts[-1]) <= len_bound
        return info

    def tree_collapse(self, *a, **k):
        out = self._base.tree_collapse(*a, **k)
        self.rounds.append(int(out[1][0]))
        return out

    def ngram_draft(self, *a, **k):
        self.chain_calls += 1
        return self._base.ngram_draft(*a, **k)


def tree_lookup(family, name, graphs, spy=False, gen=GEN, g=G, b=B, short=False, tier_sized=False, **kw):
    """One ``lookup_generate(branches=b)`` on the device.  ``tier_sized``: the launch-by-launch rounds get the size hints of the
    graph tier the replayed rounds are captured for.  Attention cuts the prefix into ``n_splits`` parts, and ``n_splits`` follows
    the hint (csrc/attn.hip, ``pick_splits``): the same round under two hints is two summation orders, so "the bits of the
    launch-by-launch round" are those of the round launched at the size it is replayed at."""
    run, m = gk.model_of(family, name)
    states = []
    orig = m.begin_lookup_decode

    def begin(*a, **k):
        states.append(orig(*a, **k))
        if tier_sized:                                                  # (behind the prefill, which keeps its own hints)
            st = states[-1]
            big = st.P + m._tier_bound(1, st.output_ids.size(1)) + st.R
            hints = m._set_hints
            m._set_hints = lambda t, d: hints(big, big)
        return states[-1]

    m.begin_lookup_decode = begin
    s = Spy() if spy else None
    if s is not None:
        assert not graphs
        m.ops = s
    m.GRAPH_ROUNDS = graphs
    try:
        out, count, num, _, mask = m.lookup_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"), gamma=g,
                                                     max_ngram=MX, min_ngram=MN, max_gen_len=gen, eos_id=run["eos_id"], branches=b, **kw)
    finally:
        del m.begin_lookup_decode
        if "_set_hints" in vars(m):
            del m._set_hints
        m.GRAPH_ROUNDS = True
        if s is not None:
            m.ops = s._base
    st, ls, lp, ll = states[0], m.last_stop, m.last_logprobs, m.last_lookup
    if not short:                                                       # (a run that stops early may end before its first capture)
        assert (st.replayer.captures > 0 and not st.replayer.disabled) == bool(graphs), "replayed / eager as asked"
    assert not st.replayer.disabled and (graphs or st.replayer.captures == 0)
    assert out.shape == (1, gen + g + 1) == mask.shape and st.branches == b and st.rounds == int(num)
    assert int(ll.hist.sum()) == int(num) == int(ll.hist_nb.sum()) and int(ll.won.sum()) <= int(num)
    return SimpleNamespace(out=out[0].tolist(), n=1 + int(count) + int(num), num=int(num), st=st, hist=ll.hist.cpu().tolist(),
                           hist_nb=ll.hist_nb.cpu().tolist(), won=ll.won.cpu().tolist(), info=ll.info.cpu().tolist(), spy=s,
                           rounds=s.rounds if s else None,
                           stop=None if ls is None else (int(ls.length[0]), int(ls.which[0]), int(ls.match_start[0])),
                           lp=None if lp is None else [t.clone().cpu() for t in (lp.token, lp.top, lp.top_ids)])


def common(a, b):
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


def same_bits(a, b, what):
    gk.same_bits(a, b, what)
    assert a.hist_nb == b.hist_nb and a.won == b.won and a.info == b.info and a.num == b.num, what


def check_against_vanilla(family, name, got, g):
    """The text is the device's vanilla text up to a first column the near-tie bound explains; in front of it every round
    accepted exactly the longest branch that is the vanilla text.  Returns that column."""
    run, m = gk.model_of(family, name)
    text, rows = gk.vanilla(family, name)
    tol = sr.TOL[run["dtype"]]
    n = min(got.n, GEN)
    assert n >= GEN - g - 1
    diff = [c for c in range(n) if got.out[c] != text[c]]
    upto = diff[0] if diff else n
    if diff:
        c = diff[0]
        assert c >= 1, "the first token comes from the same prefill"
        best = rows[c - 1].topk(2)
        print(f"{name}: parts at column {c}: took {got.out[c]}, vanilla {text[c]}, gap {float(best.values[0] - best.values[1]):.4f}")
        # (the two best in either order: at an exact tie top-k and the arg-max kernel need not name the same first)
        assert {got.out[c], text[c]} == set(best.indices.tolist()) and float(best.values[0] - best.values[1]) < tol
    prompt = run["prompt"][0, :run["prompt_len"]].tolist()
    w, long_rounds = 1, 0
    for seen, slots, info, acc in zip(got.spy.texts, got.spy.slots, got.spy.infos, got.rounds):
        assert seen == prompt + got.out[:w]                             # the text is what emitted_dev says is written
        want, ne, nb = lt.tree_draft(seen, g, len(slots), MX, MN)
        assert slots == want and info == ne
        if w + g < upto:
            # a near-tie inside a branch may cut it short, never lengthen it: rows whose margin keeps the bound are exact
            best = max(common(s, text[w:w + g]) for s in slots)
            safe = best == g or gk.margin(rows[w - 1:w + best]) >= tol  # the vanilla rows of columns w .. w + best
            assert acc <= 1 + best and (acc == 1 + best or not safe), (w, acc, best)
        long_rounds += acc >= 2 and w + acc <= upto
        w += acc
    assert long_rounds >= 1, "no round in front of that column accepted a draft token"
    return upto


def test_forced_is_the_devices_vanilla_text_and_branches_win_rounds():
    run, m = gk.model_of("llama", "forced")
    text, rows = gk.vanilla("llama", "forced")
    tol = sr.TOL[run["dtype"]]
    assert gk.margin(rows) >= tol, "choose another run: a row of the device's vanilla run is a near-tie"
    eager = tree_lookup("llama", "forced", graphs=False, spy=True)
    assert check_against_vanilla("llama", "forced", eager, G) == min(eager.n, GEN)
    full = sum(a == G + 1 for a in eager.rounds)
    print(f"forced: {len(eager.rounds)} rounds, {full} full, nb histogram {eager.hist_nb}, won {eager.won}")
    assert full >= 10 and eager.spy.chain_calls == 0
    chain = gk.lookup("llama", "forced", graphs=False, spy=True)
    print(f"forced: the chain at the same gamma takes {len(chain.rounds)} rounds")
    assert sum(eager.won[0]) >= 10
    replayed = tree_lookup("llama", "forced", graphs=True)
    same_bits(replayed, tree_lookup("llama", "forced", graphs=False, tier_sized=True), "forced")
    assert replayed.out == eager.out


@pytest.mark.parametrize("family,name,g,b", [("llama", "mixed", 4, 4), ("qwen2_bf16", "qwen_bf16_g5", 7, 8), ("llama", "mixed", 15, 4),
                                             ("llama", "forced", 1, 2)])
def test_the_text_is_the_devices_vanilla_text_up_to_an_explained_near_tie(family, name, g, b):
    eager = tree_lookup(family, name, graphs=False, spy=True, g=g, b=b)
    check_against_vanilla(family, name, eager, g)
    replayed = tree_lookup(family, name, graphs=True, g=g, b=b, logprobs=Logprobs(2))
    same_bits(replayed, tree_lookup(family, name, graphs=False, g=g, b=b, tier_sized=True, logprobs=Logprobs(2)), name)
    assert replayed.out == eager.out
    keys = [1] + eager.rounds[:-1]                                      # a round's key: what the round before it accepted
    assert replayed.st.graph_captures == sum(keys.count(a) >= 2 for a in set(keys)), "one graph per accepted-token count"


def test_a_generation_that_outgrows_its_tier_captures_the_next():
    run, m = gk.model_of("llama", "forced")
    text, rows = gk.vanilla("llama", "forced", gen=96)
    assert gk.margin(rows) >= sr.TOL[run["dtype"]], "choose another run: a row of the device's vanilla run is a near-tie"
    m.GRAPH_TIER = 32
    try:
        got = tree_lookup("llama", "forced", graphs=True, gen=96)
    finally:
        del m.GRAPH_TIER
    assert got.st.graph_tiers >= 2 and got.st.graph_captures >= 2
    n = min(got.n, 96)
    assert n >= 96 - G - 1 and got.out[:n] == text[:n]


def test_sampling_penalties_logprobs_and_stop_together_replay_the_bits_of_the_eager_rounds():
    name, seed = FP16["pairs"][0]
    s = Sampling(FP16["temperature"], FP16["top_k"], FP16["top_p"], seed)
    pen = Penalties(**hp.QWQ)
    kw = dict(sampling=s, penalties=pen, logprobs=Logprobs(2))
    plain = tree_lookup("llama", name, graphs=False, spy=True, tier_sized=True, **kw)
    assert plain.out != tree_lookup("llama", name, graphs=False).out, "sampling and the penalty do not bite"
    same_bits(tree_lookup("llama", name, graphs=True, **kw), plain, "sampled and penalised")
    # stop=: the oracle's cut of the device's own text under the same options -- inside a round that accepted drafts where
    # there is one (its overshoot is erased), else in the middle of the text
    text = plain.out[:plain.n]
    fill = plain.out[-1]                                               # (nothing wrote the last column)
    starts, c = [], 1
    for acc in plain.rounds:
        starts.append((c, acc))
        c += acc
    ends = [j for c0, acc in starts for j in range(c0, c0 + acc - 1)] + list(range(plain.n // 2, plain.n - 8))
    stop = None
    for j, k in ((j, k) for j in ends for k in range(1, 17)):
        seq = text[max(j - k + 1, 0):j + 1]
        if stop is None and so.scan(text, Stop(sequences=[seq]))[0] == j + 1:
            stop = Stop(sequences=[seq])
    assert stop is not None
    want, triple = so.cut(plain.out, plain.n, stop, fill)
    got = {}
    for graphs in (True, False):
        got[graphs] = tree_lookup("llama", name, graphs=graphs, stop=stop, short=True, tier_sized=not graphs, **kw)
        assert got[graphs].stop == triple and got[graphs].out[:plain.n] == want[:plain.n], graphs
        assert got[graphs].out[triple[0]:] == [fill] * (len(got[graphs].out) - triple[0]) and got[graphs].st.stopped
        assert torch.equal(hl.bits(got[graphs].lp[0][0, :triple[0]].contiguous()), hl.bits(plain.lp[0][0, :triple[0]].contiguous()))
        assert torch.isnan(got[graphs].lp[0][0, triple[0]:]).all()
    same_bits(got[True], got[False], "stopped")
