"""``lookup_generate(branches=B)`` through the host loop on the CPU oracle (tests/lookup_tree_oracle.py), on the toy runs of
test_host_generate_lookup.py: the text is the vanilla text for every parameter set and for ANY tree, every round accepts
exactly the longest verified branch, copies of a branch change nothing, the glide layer is not used, the loop composes with
``sampling=`` / ``penalties=`` / ``logprobs=`` / ``stop=``, ``branches=1`` is the chain loop, and the keyword's checks."""
from types import SimpleNamespace

import pytest
import torch

import lookup_oracle as lo
import lookup_tree_oracle as lt
import sampled_runs as sr
import stop_oracle as so
import test_host_generate_logprobs as hl
import test_host_generate_lookup as hk
import test_host_generate_penalized as hp
from longspec_amd import Logprobs, Sampling, Stop
from test_host_generate_sampled import FP16, build as _build, get_run

GEN = hk.GEN
RUNS = hk.RUNS
PARAMS = [(4, 2, 3, 1), (7, 4, 2, 1), (1, 8, 1, 1), (15, 4, 8, 2), (8, 8, 3, 1)]     # (gamma, branches, max_ngram, min_ngram)
G, B, MX, MN = 4, 4, 3, 1                # the parameters of the other tests


class Spy(hl.Spy):
    """``hl.Spy`` that also keeps the text and the slots of every ``ngram_tree_draft`` call, may replace the slots --
    ``override(call number, text, gamma, branches) -> branches lists of gamma ids`` -- and counts the chain's operators."""

    def __init__(self, base, override=None):
        super().__init__(base)
        self.texts, self.slots, self.nb, self.override, self.chain_calls = [], [], [], override, 0

    def ngram_tree_draft(self, prompt_ids, input_len, output_ids, written, len_bound, gamma, branches, max_ngram, min_ngram,
                         all_spec, tree_mask, info=None, hist=None, hist_nb=None):
        info = self._base.ngram_tree_draft(prompt_ids, input_len, output_ids, written, len_bound, gamma, branches, max_ngram,
                                           min_ngram, all_spec, tree_mask, info=info, hist=hist, hist_nb=hist_nb)
        text = lt.text_of(prompt_ids, input_len, output_ids, written, 0)
        assert len(text) <= len_bound
        if self.override is not None:
            slots = self.override(len(self.texts), text, gamma, branches)
            all_spec[0, 1:] = torch.tensor(lt.tree_layout(slots, gamma, branches)[0], dtype=torch.int64)
        nodes = all_spec[0, 1:].view(gamma, branches)                          # level-major: [depth - 1, branch]
        self.slots.append(nodes.t().tolist())
        self.texts.append(text)
        self.nb.append(int((info[0, :, 0] > 0).sum()))
        return info

    def ngram_draft(self, *a, **k):
        self.chain_calls += 1
        return self._base.ngram_draft(*a, **k)


def tree_lookup(family, name, g=G, b=B, mx=MX, mn=MN, gen=GEN, override=None, m=None, **kw):
    """One ``lookup_generate(branches=b)`` under the spy: out (a list), n text columns, the rounds' accepted counts, slots, texts."""
    run, m0 = hk.model_of(family, name)
    m = m or m0
    spy = Spy(lt.ops, override)
    saved, m.ops = m.ops, spy
    try:
        out, count, num, elapsed, mask = m.lookup_generate(run["prompt"], torch.tensor([run["prompt_len"]]), gamma=g, max_ngram=mx,
                                                           min_ngram=mn, max_gen_len=gen, eos_id=run["eos_id"], branches=b, **kw)
    finally:
        m.ops = saved
    rounds = [int(e[2][0]) for e in spy.events if e[0] == "tree"]
    last = [int(e[1][0, int(e[2][0]) - 1]) for e in spy.events if e[0] == "tree"]       # the deepest accepted node
    assert (int(count), int(num)) == (sum(rounds) - len(rounds), len(rounds)) and out.shape == (1, gen + g + 1) == mask.shape
    ll, ls = m.last_lookup, m.last_stop
    assert ll.branches == b and tuple(ll.info.shape) == (1, b, 2) and int(ll.hist.sum()) == len(rounds) == int(ll.hist_nb.sum())
    won = [0] * b
    for node, acc in zip(last, rounds):
        if acc >= 2:
            won[(node - 1) % b] += 1
    assert ll.won.tolist() == [won]
    return SimpleNamespace(out=out[0].tolist(), n=1 + sum(rounds), rounds=rounds, slots=spy.slots, texts=spy.texts, nb=spy.nb,
                           hist_nb=ll.hist_nb.clone(), events=spy.events, lp=m.last_logprobs, m=m, spy=spy,
                           stop=None if ls is None else (int(ls.length[0]), int(ls.which[0]), int(ls.match_start[0])))


def common(a, b):
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


_top2 = {}


def vanilla_or_tie(got, family, name, what):
    """The text is the vanilla text -- or parts from it at a column where the vanilla loop's own two best log-probs are closer
    than the project's near-tie bound of the dtype (``sr.TOL``) and takes the other of the two: a W-row verification pass and a
    one-row step round differently, and no loop can be asked which side of a tie to take.  Behind such a column the texts are
    two valid texts and are not compared.  Returns the number of columns that are the vanilla text.

    Two such columns exist in the toy runs, and only there a text parts: ``rand`` column 40 (ids 51 and 349 at the same fp16
    log-prob, gap 0.0) and ``qwen_bf16_g5`` column 49 (388 and 342, one bf16 step apart, 0.0156).  The chain loop's 5-row passes
    happen to round like the one-row step there; passes of 9 to 76 rows do not."""
    text = hk.vanilla_text(family, name)
    n = min(got.n, len(text))
    assert n >= len(text) - 16, (what, n)                              # the loop ran to the end of its buffer
    same = common(got.out[:n], text[:n])
    if same == n:
        return n
    if (family, name) not in _top2:
        run, m = hk.model_of(family, name)
        m.vanilla_generate(run["prompt"], torch.tensor([run["prompt_len"]]), max_gen_len=GEN, eos_id=run["eos_id"], logprobs=Logprobs(2))
        _top2[family, name] = (m.last_logprobs.top_ids[0].tolist(), m.last_logprobs.top[0].tolist(), sr.TOL[run["dtype"]])
    ids, vals, tol = _top2[family, name]
    print(f"{what}: column {same}: vanilla's two best {ids[same]} at {vals[same]}, the loop took {got.out[same]}; bound {tol}")
    assert ids[same][0] == text[same] and got.out[same] == ids[same][1] and vals[same][0] - vals[same][1] <= tol, what
    return same


def assert_rounds_take_the_longest_branch(got, text, g, upto=None):
    """Every round accepts 1 + the longest common prefix of a slot and what the vanilla text goes on with (checked where the
    vanilla text is long enough to tell, and in front of column ``upto``)."""
    w, checked, upto = 1, 0, len(text) if upto is None else upto
    for slots, acc in zip(got.slots, got.rounds):
        if w + g <= upto:
            assert acc == 1 + max(common(s, text[w:w + g]) for s in slots), (w, slots, text[w:w + g])
            checked += 1
        w += acc
    assert checked >= 1 and (upto < len(text) or checked >= len(got.rounds) - g - 1)


def rounds_in_front_of(got, upto, g):
    """The accepted counts of the rounds that end in front of column ``upto - g``: where a planted draft had the whole vanilla
    continuation to plant."""
    w, out = 1, []
    for acc in got.rounds:
        if w + 2 * g + 1 <= upto:
            out.append(acc)
        w += acc
    return out


@pytest.mark.parametrize("family,name", RUNS)
@pytest.mark.parametrize("g,b,mx,mn", PARAMS)
def test_the_tree_lookup_text_is_the_vanilla_text(family, name, g, b, mx, mn):
    got = tree_lookup(family, name, g, b, mx, mn)
    text = hk.vanilla_text(family, name)
    upto = vanilla_or_tie(got, family, name, (name, g, b, mx, mn))
    assert upto >= 32
    assert_rounds_take_the_longest_branch(got, text, g, upto)
    run = get_run(family, name)
    prompt = run["prompt"][0, :run["prompt_len"]].tolist()
    w, hist_nb = 1, [0] * (b + 1)
    for seen, slots, nb, acc in zip(got.texts, got.slots, got.nb, got.rounds):
        assert seen == prompt + got.out[:w]                             # the text the drafter saw: written = emitted_dev
        want, info, want_nb = lt.tree_draft(seen, g, b, mx, mn)
        assert slots == want and nb == want_nb
        assert slots[0] == lo.draft(seen, g, mx, mn)[0]                 # slot 0 is the chain's draft
        hist_nb[nb] += 1
        w += acc
    assert got.hist_nb.tolist() == [hist_nb]


def test_more_branches_accept_no_fewer_tokens_per_round_on_the_mixed_run():
    """Slot 0 is the chain's draft whatever B: from the same text a wider tree accepts at least as much."""
    one = hk.lookup("llama", "mixed", 7, 3, 1)
    wide = tree_lookup("llama", "mixed", 7, 8, 3, 1)
    print(f"mixed, gamma 7: {len(one.rounds)} chain rounds, {len(wide.rounds)} rounds of 8 branches; nb histogram {wide.hist_nb.tolist()}")
    assert len(wide.rounds) <= len(one.rounds) and max(wide.nb) >= 2


@pytest.mark.parametrize("family,name", [("llama", "mixed"), ("qwen2_bf16", "qwen_bf16_g5")])
def test_the_loop_is_lossless_for_any_tree(family, name):
    text = hk.vanilla_text(family, name)
    run = get_run(family, name)
    P, V = run["prompt_len"], run["cfg"].vocab_size
    gen = torch.Generator().manual_seed(7)

    def truth(seen, gamma):
        w = len(seen) - P
        return (text[w:w + gamma] + [0] * gamma)[:gamma]

    def wrong(seen, gamma):
        w = len(seen) - P
        d = torch.randint(0, V, (gamma,), generator=gen).tolist()
        d[0] = (text[w] + 1) % V if w < len(text) else d[0]            # never the true next token
        return d

    def noise(i, seen, gamma, b):
        return [wrong(seen, gamma) for _ in range(b)]

    def equal(i, seen, gamma, b):
        d = truth(seen, gamma)[:2] + wrong(seen, gamma)[:gamma - 2]    # two true tokens, then one that is not
        return [list(d) for _ in range(b)]

    def planted(i, seen, gamma, b):                                    # slot 0 wrong, the last slot right
        return [wrong(seen, gamma) for _ in range(b - 1)] + [truth(seen, gamma)]

    def partial(i, seen, gamma, b):                                    # slot j is right for j tokens
        t = truth(seen, gamma)
        return [t[:j] + wrong(seen, gamma)[:gamma - j] for j in range(b)]

    a = tree_lookup(family, name, override=noise)
    assert vanilla_or_tie(a, family, name, "random trees") >= 32
    assert all(acc == 1 for acc in a.rounds) and len(a.rounds) == GEN - 1
    for what, override, want in (("all slots equal", equal, 3), ("planted", planted, G + 1), ("partial", partial, B)):
        got = tree_lookup(family, name, override=override)
        upto = vanilla_or_tie(got, family, name, what)
        front = rounds_in_front_of(got, upto, G)
        assert upto >= 32 and len(front) >= 3 and all(acc == want for acc in front), (what, upto, got.rounds)
        assert_rounds_take_the_longest_branch(got, text, G, upto)


def test_with_all_slots_equal_the_rounds_are_the_chains():
    """The chain loop under a draft, and the tree loop with that draft in every slot: the same rounds, the same text."""
    run = get_run("llama", "mixed")
    V = run["cfg"].vocab_size

    def draft(seen, gamma):                                            # a function of the text alone: part lookup, part garbage
        d = lo.draft(seen, gamma, 2, 1)[0]
        return d if len(seen) % 3 else [(x + 1) % V for x in d]

    chain = hk.lookup("llama", "mixed", override=lambda i, seen, gamma: draft(seen, gamma))
    tree = tree_lookup("llama", "mixed", override=lambda i, seen, gamma, b: [draft(seen, gamma) for _ in range(b)])
    assert tree.rounds == chain.rounds and tree.texts == chain.texts and len(set(tree.rounds)) >= 2
    assert tree.out[:tree.n] == chain.out[:chain.n]


def test_a_model_without_a_draft_checkpoint_works_and_the_glide_layer_is_never_called():
    run = get_run("llama", "mixed")
    m = _build(run, ops=lt.ops)                                        # (built from the config: glide_path=None)
    with torch.no_grad():
        for p in m.glide.parameters():
            p.fill_(float("nan"))
    called = []
    m.glide.register_forward_pre_hook(lambda *a: called.append(1))
    got = tree_lookup("llama", "mixed", m=m)
    assert not called and got.out == tree_lookup("llama", "mixed").out
    assert vanilla_or_tie(got, "llama", "mixed", "NaN glide") >= 32


@pytest.mark.parametrize("name,seed", FP16["pairs"][:1])
def test_sampling_gives_the_sampled_vanilla_text(name, seed):
    s = Sampling(FP16["temperature"], FP16["top_k"], FP16["top_p"], seed)
    text = hk.vanilla_text("llama", name, sampling=s)
    got = tree_lookup("llama", name, sampling=s)
    hk.assert_is_vanilla(got, text, ("sampled", name, seed))
    assert text != hk.vanilla_text("llama", name)


def test_penalties_give_the_penalised_vanilla_text():
    kind, (name, kw) = "fp16", hp.PAIRS["fp16"]["pairs"][0]
    run, m = hk.model_of("llama", name)
    run, m, pen, gen, text = hp.checked_vanilla(kind, name, kw, m=m)   # (asserts the pair's near-tie margin)
    got = tree_lookup("llama", name, gen=gen, penalties=pen)
    assert got.n >= gen - G - 1 and got.out[:min(got.n, gen)] == text.tolist()[:min(got.n, gen)]
    assert text.tolist() != hk.vanilla_text("llama", name, gen=gen)[:gen], "the penalty does not bite"


def test_logprobs_hold_the_accepted_rows_values():
    """As tests/test_host_generate_logprobs.py has it for the tree loop: every emitted column holds the bits of the verification
    row (the tree node) that produced it, the rest the fill; and the values agree with the vanilla loop's within 2 tol."""
    family, name, top_n = "llama", "mixed", 3
    got = tree_lookup(family, name, logprobs=Logprobs(top_n))
    plain = tree_lookup(family, name)
    assert got.out == plain.out and plain.lp is None and not [e for e in plain.events if e[0] == "rows"]
    want, emitted = hl.expected_buffers("tree", got.events, GEN + G + 1, top_n)
    assert emitted == got.n
    for f in ("token", "top", "top_ids"):
        assert torch.equal(hl.bits(getattr(got.lp, f)), hl.bits(getattr(want, f))), f
    assert not torch.isnan(got.lp.token[0, :emitted]).any() and torch.isnan(got.lp.token[0, emitted:]).all()
    assert torch.equal(got.lp.top_ids[0, :emitted, 0], torch.tensor(got.out[:emitted]))
    run, m = hk.model_of(family, name)
    m.vanilla_generate(run["prompt"], torch.tensor([run["prompt_len"]]), max_gen_len=GEN, eos_id=run["eos_id"], logprobs=Logprobs(top_n))
    v_lp = m.last_logprobs
    n = min(emitted, GEN)
    err = (got.lp.token[0, :n].double() - v_lp.token[0, :n].double()).abs().max().item()
    bound = 2 * sr.TOL[run["dtype"]]
    print(f"{name}: {n} common tokens, largest log-prob difference {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_stop_cuts_the_loops_own_plain_text():
    plain = tree_lookup("llama", "mixed", logprobs=Logprobs(2))
    text = plain.out[:plain.n]
    fill = plain.out[-1]                                               # the tree loop's fill: nothing wrote the last column
    starts, c = [], 1
    for acc in plain.rounds:
        starts.append((c, acc))
        c += acc
    stops = {"column-0": Stop(token_ids=[text[0]])}
    # a stop that ends strictly inside a round, in front of tokens the round accepted as well (its overshoot)
    for j, k in ((j, k) for c, acc in starts for j in range(c, c + acc - 1) for k in range(1, 17)):
        seq = text[max(j - k + 1, 0):j + 1]
        if "inside" not in stops and so.scan(text, Stop(sequences=[seq]))[0] == j + 1:
            stops["inside"] = Stop(sequences=[seq])
    assert set(stops) == {"column-0", "inside"}
    for what, stop in stops.items():
        got = tree_lookup("llama", "mixed", logprobs=Logprobs(2), stop=stop)
        want, triple = so.cut(plain.out, plain.n, stop, fill)
        assert triple[0] > 0 and got.stop == triple, what
        assert got.out[:plain.n] == want[:plain.n] and got.out[triple[0]:] == [fill] * (len(got.out) - triple[0]), what
        assert torch.isnan(got.lp.token[0, triple[0]:]).all(), what
        assert torch.equal(hl.bits(got.lp.token[0, :triple[0]].contiguous()), hl.bits(plain.lp.token[0, :triple[0]].contiguous()))
        assert len(got.rounds) == (1 if what == "column-0" else len([s for s in starts if s[0] < triple[0]])), what
    st_rounds = []
    run, m = hk.model_of("llama", "mixed")
    orig = m.begin_lookup_decode
    m.begin_lookup_decode = lambda *a, **k: st_rounds.append(orig(*a, **k)) or st_rounds[-1]
    try:
        tree_lookup("llama", "mixed", stop=stops["inside"])
    finally:
        del m.begin_lookup_decode
    assert st_rounds[0].branches == B and st_rounds[0].stopped and m.lookup_round(st_rounds[0]) is False   # a stopped state is final


def test_min_tokens_bans_the_stop_on_the_tree_rows():
    plain = tree_lookup("llama", "mixed")
    tok = plain.out[5]
    first = plain.out.index(tok)
    stop = Stop(token_ids=[tok], min_tokens=first + 2)
    want = hk.vanilla_text("llama", "mixed", stop=stop)
    got = tree_lookup("llama", "mixed", stop=stop)
    n = got.stop[0] if got.stop[0] > 0 else min(got.n, GEN)
    assert tok not in got.out[:first + 2] and got.out[:n] == want[:n]


def test_branches_1_is_the_chain_loop():
    run, m = hk.model_of("llama", "mixed")
    spy = Spy(lt.ops)
    saved, m.ops = m.ops, spy
    try:
        out = m.lookup_generate(run["prompt"], torch.tensor([run["prompt_len"]]), gamma=G, max_ngram=MX, min_ngram=MN, max_gen_len=GEN,
                                eos_id=run["eos_id"], branches=1)[0]
    finally:
        m.ops = saved
    chains = [e for e in spy.events if e[0] == "chain"]
    assert spy.chain_calls == len(chains) >= 10 and not spy.texts and not [e for e in spy.events if e[0] == "tree"]
    assert out[0].tolist() == hk.lookup("llama", "mixed").out and out.shape == (1, GEN + G)
    ll = m.last_lookup
    assert tuple(ll.info.shape) == (1, 2) and sorted(vars(ll)) == ["hist", "info"]


def test_bad_branches_are_refused_before_the_model_is_touched():
    run, m = hk.model_of("llama", "mixed")
    pl = torch.tensor([run["prompt_len"]])
    real = m.model.forward
    m.model.forward = lambda *a, **k: (_ for _ in ()).throw(AssertionError("prefill before the refusal"))
    try:
        for bad in (dict(branches=True), dict(branches=2.0), dict(branches=0), dict(branches=9), dict(branches=8, gamma=15),
                    dict(branches=-1), dict(branches=6, gamma=12)):
            with pytest.raises(ValueError, match="lookup"):
                m.lookup_generate(run["prompt"], pl, max_gen_len=16, **bad)
            with pytest.raises(ValueError, match="lookup"):
                m.begin_lookup_decode(torch.tensor([3]), torch.tensor([8], dtype=torch.int32), pl, 8, run["prompt"], **bad)
    finally:
        m.model.forward = real
    from longspec_amd import lookup
    assert lookup.check(15, 3, 1, 4) == (15, 3, 1) and lookup.check(8, 3, 1, 8) == (8, 3, 1) and lookup.check(15, 3, 1) == (15, 3, 1)
    assert lookup.tree_rows(15, 4) == 76 and lookup.tree_rows(8, 8) == 73 and lookup.tree_rows(15, 8) > lookup.MAX_ROWS
