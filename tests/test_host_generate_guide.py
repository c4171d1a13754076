"""Guided decoding (``guide=``) through the host loops on the CPU oracle (tests/guide_oracle.py), on the toy runs of
test_host_generate_ban.py at 64 columns, under two guides: the parity guide -- even and odd ids must alternate, the loops' EOS id
legal in both states, which takes a class of its own (S = 2, C = 3) -- and a ``Guide.choice`` of three sequences.  The plain
texts leave the parity language and the guided texts do not, every loop returns the guided vanilla text, every prefix of it
walks to a live state, every operator call saw the state of the committed text, ``guide_advance`` follows ``token_state_add``,
the keyword composes with ``penalties=`` / ``sampling=`` / ``logprobs=`` / ``stop=`` / ``ban=``, and the keyword's checks."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import guide_oracle as go
import sampled_runs as sr
import test_host_generate_ban as hb
import test_host_generate_lookup as hk
from longspec_amd import Ban, Guide, Logprobs, Penalties, Sampling, Stop
from test_host_generate_sampled import FP16, build as _build, get_run
from test_host_generate_stop import CallSpy

GEN = 64
RUNS = hk.RUNS
G = 4                                   # gamma of the chain and lookup loops
_models, _cache = {}, {}
loops_of, tree_shape_of, common = hb.loops_of, hb.tree_shape_of, hb.common


def model_of(family, name):
    if (family, name) not in _models:
        run = get_run(family, name)
        _models[family, name] = (run, _build(run, ops=go.ops))
    return _models[family, name]


def eos_of(run, m):
    """The id the guides end a text with: the one the loops' built-in EOS test looks for, or -- where that lies outside the toy
    vocabulary, so that no text can hold it -- id 1, on which no loop stops: the text then goes on with it to the last column."""
    eos = m._stop_id(run["eos_id"], "vanilla")
    eos = run["eos_id"] if eos is None else eos
    return eos if 0 <= eos < run["cfg"].vocab_size else 1


def parity_guide(V, eos, start):
    """State 0 wants an even id, state 1 an odd one; ``eos`` is legal in both and keeps the state."""
    tc = np.arange(V) % 2
    if 0 <= eos < V:
        tc[eos] = 2
    return Guide([[1, -1, 0], [-1, 0, 1]], tc, start=start)


def in_parity(text, start, eos):
    s = start
    for t in text:
        if t == eos:
            continue
        if t % 2 != s:
            return False
        s ^= 1
    return True


class Spy(CallSpy):
    """``CallSpy`` (operator names, ``chain_commit`` / ``tree_collapse`` events) that keeps, per ``guide_rows`` call, the state
    handed over, the states of all rows and the rows returned, and the arguments of every ``guide_advance`` and (non-prompt)
    ``token_state_add`` call."""

    def __init__(self, base):
        super().__init__(base)
        self.states, self.row_states, self.rows, self.advanced, self.counted, self.deepest = [], [], [], [], [], 0

    def guide_rows(self, logits, table, state, extra_ids=None, extra_mask=None):
        self.names.append("guide_rows")
        R = logits.shape[1] if logits.dim() == 3 else 1
        assert state.dtype == torch.int32 and tuple(state.shape) == (logits.shape[0],)
        if extra_ids is not None:
            mask = extra_mask if extra_mask.dim() == 3 else extra_mask[None]
            assert tuple(mask.shape[1:]) == (R, extra_ids.shape[1]) and R == extra_ids.shape[1] + 1
            depth = [int(mask[0, c + 1].ne(0).sum()) for c in range(extra_ids.shape[1])]     # column c is row c + 1's own token
            for r in range(R):
                on_path = [depth[c] for c in range(extra_ids.shape[1]) if int(mask[0, r, c]) != 0]
                assert on_path == list(range(1, len(on_path) + 1)), (r, on_path)
        self.states.append(state.clone())
        rs = go.row_states(go.parse(table), logits.shape[-1], state, R, extra_ids, extra_mask)[0]
        self.row_states.append(rs)
        out = self._base.guide_rows(logits, table, state, extra_ids=extra_ids, extra_mask=extra_mask)
        self.rows.append(out.detach().clone().reshape(-1, out.shape[-1]))
        return out

    def guide_advance(self, state, table, ids, num=None):
        self.names.append("guide_advance")
        self.advanced.append((ids.clone().view(state.shape[0], -1), None if num is None else num.clone()))
        return self._base.guide_advance(state, table, ids, num)

    def token_state_add(self, state, ids, num=None, prompt=False):
        self.names.append("token_state_add")
        if not prompt:
            self.counted.append((ids.clone().view(state.shape[0], -1), None if num is None else num.clone()))
        return self._base.token_state_add(state, ids, num=num, prompt=prompt)


def run_loop(family, name, loop, guide, gen=GEN, **kw):
    """One loop under the spy: out (a list), n text columns, the rounds' accepted counts, the spy, last_logprobs, last_stop."""
    key = (family, name, loop, guide, gen)
    if not kw and key in _cache:
        return _cache[key]
    run, m = model_of(family, name)
    spy = Spy(go.ops)
    saved, m.ops = m.ops, spy
    try:
        ids, pl = run["prompt"], torch.tensor([run["prompt_len"]])
        kw = dict(max_gen_len=gen, eos_id=run["eos_id"], guide=guide, **kw)
        if loop == "vanilla":
            out = m.vanilla_generate(ids, pl, **kw)[0]
        elif loop == "chain":
            out = m.spec_generate(ids, pl, gamma=G, **kw)[0]
        elif loop == "magicdec":
            out = m.magicdec_generate(ids, pl, gamma=3, **kw)[0]
        elif loop == "tree":
            out = m.tree_spec_generate(ids, pl, tree_shape=tree_shape_of(run, name), **kw)[0]
        else:
            out = m.lookup_generate(ids, pl, gamma=G, max_ngram=3, min_ngram=1, branches=int(loop[-1]), **kw)[0]
    finally:
        m.ops = saved
    tree = loop in ("tree", "lookup2")
    rounds = [int(e[2][0]) for e in spy.events if e[0] == "tree"] if tree else \
        [int(e[1][0]) for e in spy.events if e[0] == "chain"] if loop != "vanilla" else [1] * (len(spy.rows) - 1 if spy.rows else gen - 1)       # (a guided vanilla loop may end at an EOS)
    ls = m.last_stop
    got = SimpleNamespace(out=out[0].tolist(), n=min(1 + sum(rounds), out.shape[1]), rounds=rounds, spy=spy, lp=m.last_logprobs,
                          stop=None if ls is None else (int(ls.length[0]), int(ls.which[0]), int(ls.match_start[0])))
    if set(kw) == {"max_gen_len", "eos_id", "guide"}:
        _cache[key] = got
    return got


def text_of(got, eos=None):
    """The text: the written columns, cut behind the first ``eos``."""
    t = got.out[:got.n]
    return t[:t.index(eos) + 1] if eos is not None and eos in t else t


def parity_for(family, name):
    """The parity guide of a run, with the start state under which the run's plain text leaves the language (asserted), and the
    column where it leaves it."""
    run, m = model_of(family, name)
    eos = eos_of(run, m)
    plain = run_loop(family, name, "vanilla", None)
    for start in (plain.out[0] % 2, 1 - plain.out[0] % 2):                 # (first: the text's own first parity, if that leaves too)
        if not in_parity(plain.out, start, eos):
            first = next(c for c in range(1, GEN + 1) if not in_parity(plain.out[:c], start, eos))
            return parity_guide(run["cfg"].vocab_size, eos, start), start, first - 1
    raise AssertionError("the plain text must leave the parity language, or the test shows nothing")


def assert_text_or_tie(got, ref, family, name, what, eos, upto=None):
    """``hb.assert_text_or_tie`` on the rows ``guide_rows`` handed back: ``got`` is the text ``ref`` (the vanilla loop's, same
    keywords) -- or parts from it at a column where the vanilla loop's own two best entries are closer than the dtype's near-tie
    bound (``sr.TOL``) and takes the other of the two: a W-row pass and a one-row step round differently.  Returns the number
    of columns that agree."""
    run, m = model_of(family, name)
    a, b = text_of(got, eos), text_of(ref, eos)
    n = min(len(a), len(b), upto or len(b))
    same = common(a[:n], b[:n])
    if same == n:
        return n
    margin = sr.TOL[run["dtype"]]
    row = ref.spy.rows[same][0].float()
    top, took, other = float(row.max()), float(row[b[same]]), float(row[a[same]])
    print(f"{what}: column {same}: vanilla took {b[same]} at {took}, the loop {a[same]} at {other}; bound {margin}")
    assert took == top and top - other <= margin, what
    return same


@pytest.mark.parametrize("family,name", RUNS)
def test_the_plain_texts_leave_the_language_and_the_guided_texts_do_not(family, name):
    run, m = model_of(family, name)
    eos, V = eos_of(run, m), run["cfg"].vocab_size
    plain = run_loop(family, name, "vanilla", None)
    assert "guide_rows" not in plain.spy.names and "guide_advance" not in plain.spy.names
    guide, start, first = parity_for(family, name)
    print(f"{name}: start {start}; the plain text leaves the parity language at column {first}")
    got = run_loop(family, name, "vanilla", guide)
    text = text_of(got, eos)
    assert in_parity(text, start, eos) and got.out != plain.out
    assert got.out[:first] == plain.out[:first] and got.out[first] != plain.out[first]      # guided decoding parts exactly there
    steps = len(got.spy.rows)
    assert got.spy.names.count("guide_rows") == steps and got.spy.names.count("guide_advance") == steps
    # every token is the arg-max of the row the operator handed back, the row saw the state of the text so far, and every
    # prefix of the text walks to a live state
    rows = torch.cat(got.spy.rows)
    assert rows.float().argmax(dim=-1).tolist()[:len(text)] == text
    p = go.parse(guide.table(V, "cpu"))
    for c in range(len(text) + 1):
        s = go.walk(p, guide.start, text[:c])
        assert s >= 0 and s == guide.walk(text[:c], vocab=V), c
        if c < steps:
            assert got.spy.states[c].tolist() == [s], c
            assert torch.isinf(rows[c]).nonzero().view(-1).tolist() == np.flatnonzero(~go.allowed(p, s, V)).tolist(), c


def choice_for(family, name):
    """A choice of three sequences that bites at column 2 of the run's plain text: two go on from its first two tokens with
    other ids, the third starts elsewhere."""
    run, m = model_of(family, name)
    eos, V = eos_of(run, m), run["cfg"].vocab_size
    plain = run_loop(family, name, "vanilla", None).out
    other = [t for t in range(3, V) if t not in (plain[0], plain[1], plain[2], eos)]
    seqs = [plain[:2] + other[0:3], plain[:2] + [other[5], other[4]], [other[6], other[7], other[8]]]
    return Guide.choice(seqs, eos), seqs, eos


@pytest.mark.parametrize("family,name", RUNS)
def test_every_loop_returns_the_guided_vanilla_text(family, name):
    run, m = model_of(family, name)
    V = run["cfg"].vocab_size
    parity, start, first = parity_for(family, name)
    choice, seqs, eos = choice_for(family, name)
    for guide in (parity, choice):
        ref = run_loop(family, name, "vanilla", guide)
        want = text_of(ref, eos)
        if guide is choice:
            assert want in [s + [eos] for s in seqs] and want[:2] == seqs[0][:2], want
        else:
            assert len(want) >= GEN - 24
        p = go.parse(guide.table(V, "cpu"))
        for loop in loops_of(run):
            if loop == "vanilla":
                continue
            got = run_loop(family, name, loop, guide)
            text = text_of(got, eos)
            same = assert_text_or_tie(got, ref, family, name, (name, loop, guide), eos)
            assert same >= min(24, len(want)) and len(text) >= len(want) - 24, (loop, same, len(text))
            assert all(go.walk(p, guide.start, text[:c]) >= 0 for c in range(len(text) + 1)), loop
            if guide is choice:
                assert text == want, loop
            # every round's operator call saw the state of the committed text, and every advance the round's tokens
            w = 1
            assert got.spy.states[0].tolist() == [guide.start] and len(got.spy.states) == 1 + len(got.rounds)
            assert len(got.spy.advanced) == 1 + len(got.rounds) and got.spy.advanced[0][0].tolist() == [[got.out[0]]]
            for state, (ids, num), acc in zip(got.spy.states[1:], got.spy.advanced[1:], got.rounds):
                assert state.tolist() == [go.walk(p, guide.start, got.out[:w])], (loop, w)
                assert int(num[0]) == acc and ids[0, :acc].tolist() == got.out[w:w + acc], (loop, w)
                w += acc


def late_parity_guide(family, name, loop):
    """A guide that lets the first round of the loop's plain run that accepts a draft happen: that round starts at column c and
    writes columns c and c + 1; the guide counts k = c + 2 free columns (one state per column, every id legal) and is the parity
    guide from there on, in the start state the rest of the plain text leaves.  (guide, c, k)."""
    run, m = model_of(family, name)
    eos, V = eos_of(run, m), run["cfg"].vocab_size
    plain = run_loop(family, name, loop, None)
    c = 1
    for acc in plain.rounds:
        if acc >= 2:
            break
        c += acc
    else:
        raise AssertionError(f"{name} {loop}: the plain run accepts no draft")
    k = c + 2
    start = next(s for s in (0, 1) if not in_parity(plain.out[k:plain.n], s, eos))
    nx = [[i + 1] * 3 for i in range(k - 1)] + [[k + start] * 3, [k + 1, -1, k], [-1, k, k + 1]]
    return Guide(nx, parity_guide(V, eos, 0).token_class), c, k


@pytest.mark.parametrize("family,name", RUNS)
def test_the_speculative_loops_accept_drafts_under_the_guide(family, name):
    """Without a round of two or more tokens no row with a path decides a token.  The chain and the tree loop must have such
    rounds under the parity guide, inside the columns that are compared with the vanilla text; and rows must die: a guide under
    which no draft ever leaves the language tests no dead row.

    The chain loop of `rand` has no such round under any parity assignment: its random draft layer has a single guess per step
    (one accepted draft token in 62 plain rounds, as test_host_generate_ban.py records).  It runs under a third guide built to
    let that one round happen -- free columns up to it, parity behind it (listed and asserted)."""
    run, m = model_of(family, name)
    parity, start, first = parity_for(family, name)
    eos, V = eos_of(run, m), run["cfg"].vocab_size
    ref = run_loop(family, name, "vanilla", parity)
    fallback = []
    for loop in ("chain", "tree"):
        got = run_loop(family, name, loop, parity)
        same = assert_text_or_tie(got, ref, family, name, (name, loop), eos)
        inside, w = [], 1
        for acc in got.rounds:
            inside.append(acc >= 2 and w + acc <= same)
            w += acc
        dead = sum(1 for rs in got.spy.row_states for s in rs if s < 0)
        deepest = max(acc for acc in got.rounds)
        print(f"{name} {loop}: {sum(inside)} rounds of two or more inside the {same} compared columns, widest {deepest}; {dead} dead rows")
        assert dead > 0, loop
        if any(inside):
            continue
        fallback.append(loop)
        late, c, k = late_parity_guide(family, name, loop)
        late_ref, got = run_loop(family, name, "vanilla", late), run_loop(family, name, loop, late)
        plain = run_loop(family, name, loop, None)
        same = assert_text_or_tie(got, late_ref, family, name, (name, loop, "late"), eos)
        starts, w = {}, 1
        for acc in got.rounds:
            starts[w] = acc
            w += acc
        print(f"{name} {loop}: free up to column {k}: the round at column {c} accepts {starts.get(c)}, {same} columns are the vanilla text")
        assert starts.get(c, 0) >= 2 and same > k, "the round the guide was built for accepts no draft"
        text = text_of(got, eos)
        assert text[:k] == plain.out[:k] and text != plain.out[:len(text)]
        p = go.parse(late.table(V, "cpu"))
        assert all(go.walk(p, late.start, text[:i]) >= 0 for i in range(len(text) + 1))
    assert fallback == {"rand": ["chain"]}.get(name, []), fallback


def test_magicdec_returns_the_guided_vanilla_text_on_a_long_prompt():
    family, name = "llama", "mixed@1030"
    run, m = model_of(family, name)
    assert "magicdec" in loops_of(run)
    eos = eos_of(run, m)
    plain = run_loop(family, name, "vanilla", None, gen=32)
    start = next(s for s in (0, 1) if not in_parity(plain.out, s, eos))
    guide = parity_guide(run["cfg"].vocab_size, eos, start)
    ref = run_loop(family, name, "vanilla", guide, gen=32)
    assert in_parity(text_of(ref, eos), start, eos)
    got = run_loop(family, name, "magicdec", guide, gen=32)
    assert assert_text_or_tie(got, ref, family, name, "magicdec", eos) >= 24 and in_parity(text_of(got, eos), start, eos)


COMPOSED = {"penalties": ("mixed", dict(penalties=Penalties(repetition=1.1, presence=0.2))),
            "sampling": (FP16["pairs"][0][0], dict(sampling=Sampling(FP16["temperature"], FP16["top_k"], FP16["top_p"], FP16["pairs"][0][1]))),
            "logprobs": ("mixed", dict(logprobs=Logprobs(3))),
            "stop": ("mixed", {}),
            "ban": ("mixed", {})}


@pytest.mark.parametrize("what", sorted(COMPOSED))
def test_composition(what):
    """``guide=`` with each of the other request keywords: the parity guide whose start state the keyword's own vanilla text
    leaves, and every loop returns the vanilla loop's text."""
    family = "llama"
    name, kw = COMPOSED[what]
    run, m = model_of(family, name)
    eos, V = eos_of(run, m), run["cfg"].vocab_size
    plain = run_loop(family, name, "vanilla", None, **kw)
    start = next(s for s in (plain.out[0] % 2, 1 - plain.out[0] % 2) if not in_parity(plain.out, s, eos))
    guide = parity_guide(V, eos, start)
    if what in ("stop", "ban"):
        base = run_loop(family, name, "vanilla", guide).out
        if what == "stop":
            # a stop id the guided text would emit at a column in front of min_tokens, for the first time there: the
            # min_tokens ban and the guide bite in the same rows
            c = next(c for c in range(3, 12) if base[c] not in base[:c])
            kw = dict(stop=Stop(token_ids=[base[c]], min_tokens=12))
        else:
            c = 9                         # a trigram of the guided text: the ban parts the text there, inside the language
            kw = dict(ban=Ban(sequences=[base[c - 2:c + 1]]))
    ref = run_loop(family, name, "vanilla", guide, **kw)
    n_ref = ref.stop[0] if ref.stop is not None and ref.stop[0] > 0 else len(text_of(ref, eos))
    assert n_ref >= 12 and in_parity(ref.out[:n_ref], start, eos) and ref.out[:n_ref] != plain.out[:n_ref], what
    if what in ("stop", "ban"):
        assert ref.out[:c] == base[:c] and ref.out[c] != base[c], what
    for loop in ("chain", "tree", "lookup1", "lookup2"):
        got = run_loop(family, name, loop, guide, **kw)
        assert got.stop == ref.stop or got.n < n_ref, (what, loop, got.stop, ref.stop)
        assert assert_text_or_tie(got, ref, family, name, (what, loop), eos, upto=n_ref) >= 12
        if what == "penalties":           # guide_advance gets the ids and num of token_state_add, call for call
            assert len(got.spy.advanced) == len(got.spy.counted) >= 2
            for (ids_a, num_a), (ids_c, num_c) in zip(got.spy.advanced, got.spy.counted):
                assert torch.equal(ids_a, ids_c) and (num_a is None) == (num_c is None)
                assert num_a is None or torch.equal(num_a, num_c)


def test_forbidden_ids_are_never_listed_with_a_finite_logprob():
    """The log-probs are those of the guided distribution: a forbidden id that reaches the top-n listing shows -inf, the emitted
    token is never forbidden and its own log-prob is finite.  Under the choice guide all but a few ids are forbidden, so the
    top 20 hold forbidden ones at every column."""
    family, name = "llama", "mixed"
    run, m = model_of(family, name)
    V = run["cfg"].vocab_size
    guide, seqs, eos = choice_for(family, name)
    p = go.parse(guide.table(V, "cpu"))
    for loop in ("vanilla", "tree", "lookup2"):
        got = run_loop(family, name, loop, guide, gen=24, logprobs=Logprobs(20))
        lp, text = got.lp, text_of(got, eos)
        assert text in [s + [eos] for s in seqs]
        for c in range(len(text)):
            ok = go.allowed(p, go.walk(p, guide.start, text[:c]), V)
            assert ok.sum() <= 3 and ok[text[c]] and torch.isfinite(lp.token[0, c]), (loop, c)
            listed = dict(zip(lp.top_ids[0, c].tolist(), lp.top[0, c].tolist()))
            assert all((v == float("-inf")) == (not ok[t]) for t, v in listed.items()), (loop, c, listed)
            assert int(lp.top_ids[0, c, 0]) == text[c]


def test_without_the_keyword_no_new_operator_is_fetched(monkeypatch):
    from longspec_amd.guide import GUIDE_ENV
    monkeypatch.delenv(GUIDE_ENV, raising=False)
    for family, name in (("llama", "mixed"), ("llama", "mixed@1030")):
        run, m = model_of(family, name)
        V = run["cfg"].vocab_size
        free = Guide([[0]], np.zeros(V, dtype=np.int64))                   # everything allowed: the text does not change
        for loop in loops_of(run):
            plain = run_loop(family, name, loop, None, gen=16)
            assert "guide_rows" not in plain.spy.names and "guide_advance" not in plain.spy.names, loop
            got = run_loop(family, name, loop, free, gen=16)
            assert got.out == plain.out, loop
            assert got.spy.names.count("guide_rows") == 1 + len(plain.rounds), loop        # the first token, then one per round
            assert got.spy.names.count("guide_advance") == 1 + len(plain.rounds), loop
            # every other operator is called as before, in the same order
            assert [n for n in got.spy.names if n not in ("guide_rows", "guide_advance")] == plain.spy.names, loop


def test_refusals():
    run, m = model_of("llama", "mixed")
    pl = torch.tensor([run["prompt_len"]])
    guide = parity_guide(run["cfg"].vocab_size, eos_of(run, m), 0)
    real = m.model.forward
    m.model.forward = lambda *a, **k: (_ for _ in ()).throw(AssertionError("prefill before the refusal"))
    try:
        for call in (lambda: m.tree_spec_generate(run["prompt"], pl, tree_shape=run["tree_shape"], max_gen_len=16, temperature=0.5, guide=guide),
                     lambda: m.spec_generate(run["prompt"], pl, max_gen_len=16, temperature=0.5, guide=guide),
                     lambda: m.magicdec_generate(run["prompt"], pl, max_gen_len=16, temperature=0.5, guide=guide)):
            with pytest.raises(ValueError, match="temperature"):
                call()
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.tree_spec_generate(run["prompt"], pl, max_gen_len=16, shard=SimpleNamespace(vocab_parallel=True), guide=guide)
        for call in (lambda: m.vanilla_generate(run["prompt"], pl, max_gen_len=16, guide=[[3]]),
                     lambda: m.lookup_generate(run["prompt"], pl, max_gen_len=16, guide="g.npz"),
                     lambda: m.lookup_generate(run["prompt"], pl, max_gen_len=16, branches=2, guide=2)):
            with pytest.raises(TypeError, match="longspec_amd.Guide"):
                call()
        dead_end = Guide([[1], [-1]])                                       # a reachable state that allows nothing: before any prefill
        with pytest.raises(ValueError, match="state 1 is reachable"):
            m.vanilla_generate(run["prompt"], pl, max_gen_len=16, guide=dead_end)
    finally:
        m.model.forward = real
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    with pytest.raises(ValueError, match="temperature"):
        m.begin_tree_decode(first, lens, run["prompt_len"], temperature=0.5, guide=guide)
    with pytest.raises(ValueError, match="temperature"):
        m.begin_chain_decode(first, lens, lens, run["prompt_len"], temperature=0.5, guide=guide)
    m.model.layers[-1].self_attn.shard = SimpleNamespace(vocab_parallel=True)
    try:
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_tree_decode(first, lens, run["prompt_len"], guide=guide)
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_chain_decode(first, lens, lens, run["prompt_len"], guide=guide)
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_vanilla_decode(torch.zeros((1, 8), dtype=torch.int64), lens.clone(), lens, run["prompt_len"], guide=guide)
        for branches in (1, 2):
            with pytest.raises(ValueError, match="vocabulary-parallel"):
                m.begin_lookup_decode(first, lens, lens, run["prompt_len"], run["prompt"], branches=branches, guide=guide)
    finally:
        m.model.layers[-1].self_attn.shard = None


def test_environment_default(monkeypatch, tmp_path):
    from longspec_amd.guide import GUIDE_ENV
    run, m = model_of("llama", "mixed")
    eos, V = eos_of(run, m), run["cfg"].vocab_size
    pl = torch.tensor([run["prompt_len"]])
    first, lens = torch.tensor([2]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    monkeypatch.delenv(GUIDE_ENV, raising=False)
    assert m.begin_tree_decode(first, lens, run["prompt_len"]).guide is None
    plain = m.vanilla_generate(run["prompt"], pl, max_gen_len=GEN, eos_id=run["eos_id"])[0][0].tolist()
    start = next(s for s in (0, 1) if not in_parity(plain, s, eos))
    want = parity_guide(V, eos, start)
    path = str(tmp_path / "parity.npz")
    want.save(path)
    monkeypatch.setenv(GUIDE_ENV, path)
    st = m.begin_tree_decode(first, lens, run["prompt_len"])
    assert st.guide.cfg == want and st.guide.state.dtype == torch.int32
    assert st.guide.state.tolist() == [want.walk([2], vocab=V)]                                           # start advanced by the first token
    assert m.begin_tree_decode(first, lens, run["prompt_len"], temperature=0.5).guide is None
    other = Guide([[0]], np.zeros(V, dtype=np.int64))
    assert m.begin_tree_decode(first, lens, run["prompt_len"], guide=other).guide.cfg == other            # the argument wins
    assert m.begin_chain_decode(first, lens, lens, run["prompt_len"]).guide.cfg == want
    for branches in (1, 2):
        assert m.begin_lookup_decode(first, lens, lens, run["prompt_len"], run["prompt"], branches=branches).guide.cfg == want
    out = torch.zeros((1, 8), dtype=torch.int64)
    out[0, 0] = 2
    st = m.begin_vanilla_decode(out, lens.clone(), lens, run["prompt_len"])
    assert st.guide.cfg == want and st.guide.table.dtype == torch.int32 and torch.equal(st.guide.table, want.table(V, "cpu"))
    got = m.vanilla_generate(run["prompt"], pl, max_gen_len=GEN, eos_id=run["eos_id"])[0][0].tolist()
    assert got != plain and in_parity(got[:got.index(eos) + 1] if eos in got else got, start, eos)
    monkeypatch.delenv(GUIDE_ENV)
    assert m.vanilla_generate(run["prompt"], pl, max_gen_len=GEN, eos_id=run["eos_id"])[0][0].tolist() == plain
