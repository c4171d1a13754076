"""Banned sequences and no-repeat n-grams (``ban=``) through the host loops on the CPU oracle (tests/ban_oracle.py), on the toy
runs of test_host_generate_lookup.py at 64 columns: the plain texts repeat themselves and the banned texts do not, a banned
sequence stays out and changes nothing in front of it, every loop returns the banned vanilla text, every round hands the
operator the text so far and paths in depth order, the keyword composes with ``penalties=`` / ``sampling=`` / ``logprobs=`` /
``stop=``, and the keyword's checks."""
from types import SimpleNamespace

import pytest
import torch

import ban_oracle as bo
import sampled_runs as sr
import test_host_generate_logprobs as hl
import test_host_generate_lookup as hk
from longspec_amd import Ban, Logprobs, Penalties, Sampling, Stop
from test_host_generate_sampled import FP16, build as _build, get_run
from test_host_generate_stop import CallSpy, loops_of as _glide_loops

GEN = 64
RUNS = hk.RUNS
G = 4                                   # gamma of the chain and lookup loops
_models, _cache = {}, {}


def model_of(family, name):
    if (family, name) not in _models:
        run = get_run(family, name)
        _models[family, name] = (run, _build(run, ops=bo.ops))
    return _models[family, name]


# The `rand` run's draft layer is random weights: its first guess is rarely the target's token, and under the run's own shape
# 4/16/16/16/16 no round of the banned tree loop accepts a draft.  Sixteen root children give the target's token a place in the
# tree often enough (rounds of two under both bans below, asserted).
TREE_SHAPES = {"rand": [16, 16]}


def tree_shape_of(run, name):
    return TREE_SHAPES.get(name, run["tree_shape"])


def loops_of(run):
    return _glide_loops(run) + ["lookup1", "lookup2"]


class Spy(CallSpy):
    """``CallSpy`` (operator names, ``chain_commit`` / ``tree_collapse`` events) that checks every ``ban_rows`` call as it
    comes -- the selected extras of every row, in increasing column, lie at depths 1, 2, 3 ... -- and keeps the committed text
    the call saw and the rows it returned."""

    def __init__(self, base):
        super().__init__(base)
        self.seen, self.rows, self.deepest = [], [], 0

    def ban_rows(self, logits, table, output_ids, base=None, base_sub=None, base_add=0, extra_ids=None, extra_mask=None):
        self.names.append("ban_rows")
        R = logits.shape[1] if logits.dim() == 3 else 1
        if extra_ids is not None:
            mask = extra_mask if extra_mask.dim() == 3 else extra_mask[None]
            assert tuple(mask.shape[1:]) == (R, extra_ids.shape[1]) and R == extra_ids.shape[1] + 1
            depth = [int(mask[0, c + 1].ne(0).sum()) for c in range(extra_ids.shape[1])]     # column c is row c + 1's own token
            for r in range(R):
                on_path = [depth[c] for c in range(extra_ids.shape[1]) if int(mask[0, r, c]) != 0]
                assert on_path == list(range(1, len(on_path) + 1)), (r, on_path)
                self.deepest = max(self.deepest, len(on_path))
        texts = bo.row_texts(logits.shape[0], R, output_ids, base, base_sub, base_add, extra_ids, extra_mask)
        out = self._base.ban_rows(logits, table, output_ids, base=base, base_sub=base_sub, base_add=base_add, extra_ids=extra_ids,
                                  extra_mask=extra_mask)
        self.seen.append(texts[0][0])                                     # row 0 follows no extra: the committed text
        self.rows.append(out.detach().clone().reshape(-1, out.shape[-1]))
        return out


def run_loop(family, name, loop, ban, gen=GEN, **kw):
    """One loop under the spy: out (a list), n text columns, the rounds' accepted counts, the spy, last_logprobs, last_stop."""
    key = (family, name, loop, ban, gen)
    if not kw and key in _cache:
        return _cache[key]
    run, m = model_of(family, name)
    spy = Spy(bo.ops)
    saved, m.ops = m.ops, spy
    try:
        ids, pl = run["prompt"], torch.tensor([run["prompt_len"]])
        kw = dict(max_gen_len=gen, eos_id=run["eos_id"], ban=ban, **kw)
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
        [int(e[1][0]) for e in spy.events if e[0] == "chain"] if loop != "vanilla" else [1] * (gen - 1)
    ls = m.last_stop
    got = SimpleNamespace(out=out[0].tolist(), n=min(1 + sum(rounds), out.shape[1]), rounds=rounds, spy=spy, lp=m.last_logprobs,
                          stop=None if ls is None else (int(ls.length[0]), int(ls.which[0]), int(ls.match_start[0])))
    if set(kw) == {"max_gen_len", "eos_id", "ban"}:
        _cache[key] = got
    return got


def text_of(got):
    return got.out[:got.n]


def common(a, b):
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


def assert_text_or_tie(got, ref, family, name, what, upto=None):
    """``got`` is the text ``ref`` (the vanilla loop's, same keywords) -- or parts from it at a column where the vanilla loop's
    own two best entries are closer than the dtype's near-tie bound (``sr.TOL``, the measure of
    ``test_host_generate_penalized.top2_margin``) and takes the other of the two: a W-row pass and a one-row step round
    differently.  Returns the number of columns that agree."""
    run, m = model_of(family, name)
    n = min(got.n, ref.n, upto or ref.n)
    same = common(text_of(got)[:n], text_of(ref)[:n])
    if same == n:
        return n
    margin = sr.TOL[run["dtype"]]
    row = ref.spy.rows[same][0].float()
    top, took, other = float(row.max()), float(row[ref.out[same]]), float(row[got.out[same]])
    print(f"{what}: column {same}: vanilla took {ref.out[same]} at {took}, the loop {got.out[same]} at {other}; bound {margin}")
    assert took == top and top - other <= margin, what
    return same


@pytest.mark.parametrize("family,name", RUNS)
def test_the_plain_texts_repeat_and_the_banned_texts_do_not(family, name):
    plain = run_loop(family, name, "vanilla", None)
    assert plain.n == GEN and "ban_rows" not in plain.spy.names
    for n in (2, 3):
        first = bo.repeats(plain.out, n)
        print(f"{name}: the plain text first repeats a {n}-gram at column {first}")
        assert first is not None, "the plain text must violate the ban, or the test shows nothing"
        got = run_loop(family, name, "vanilla", Ban(no_repeat_ngram=n))
        assert bo.repeats(got.out, n) is None and got.out != plain.out
        assert got.out[:first] == plain.out[:first] and got.out[first] != plain.out[first]      # banned decoding parts exactly there
        assert got.spy.names.count("ban_rows") == GEN                     # the first token's row and one per step
        # every token is the arg-max of the row the operator handed back, and the row saw the text so far
        rows = torch.cat(got.spy.rows)
        assert rows.float().argmax(dim=-1).tolist() == got.out
        assert got.spy.seen == [got.out[:c] for c in range(GEN)]


@pytest.mark.parametrize("family,name", RUNS)
def test_a_banned_sequence_stays_out_and_nothing_in_front_of_it_changes(family, name):
    plain = run_loop(family, name, "vanilla", None).out
    for k in (0, 5, 17):
        seq = plain[k:k + 3]
        first = next(c for c in range(len(plain) - 2) if plain[c:c + 3] == seq)      # (the forced run repeats itself)
        got = run_loop(family, name, "vanilla", Ban(sequences=[seq])).out
        assert all(got[c:c + 3] != seq for c in range(GEN - 2)), (k, seq)
        assert got[:first + 2] == plain[:first + 2] and got[first + 2] != plain[first + 2], (k, seq)
    # a one-token sequence is banned from column 0 on
    got = run_loop(family, name, "vanilla", Ban(sequences=[[plain[0]], [plain[1]]])).out
    assert plain[0] not in got and plain[1] not in got


BANS = [Ban(no_repeat_ngram=2), Ban(no_repeat_ngram=3)]


def check_loop_against_vanilla(family, name, loop, ban):
    """The loop's text under ``ban`` is the vanilla loop's up to an explained near-tie, and every round's operator call saw the
    text so far.  Returns the run."""
    ref = run_loop(family, name, "vanilla", ban)
    got = run_loop(family, name, loop, ban)
    same = assert_text_or_tie(got, ref, family, name, (name, loop, ban))
    assert same >= 24 and got.n >= GEN - 24, (loop, same, got.n)
    w = 1
    assert got.spy.seen[0] == [] and len(got.spy.seen) == 1 + len(got.rounds)
    for seen, acc in zip(got.spy.seen[1:], got.rounds):
        assert seen == got.out[:w], (loop, w)
        w += acc
    return got, same


@pytest.mark.parametrize("family,name", RUNS)
@pytest.mark.parametrize("ban", BANS, ids=lambda b: f"ngram{b.no_repeat_ngram}")
def test_every_loop_returns_the_banned_vanilla_text(family, name, ban):
    run, m = model_of(family, name)
    for loop in loops_of(run):
        if loop == "vanilla":
            continue
        got, same = check_loop_against_vanilla(family, name, loop, ban)
        assert bo.repeats(text_of(got), ban.no_repeat_ngram) is None, loop


def late_sequence_ban(family, name, loop):
    """A ban that bites INSIDE the first round of the loop's plain run that accepts a draft: that round starts at column c and
    its row 1 -- which follows the draft token of column c -- decides column c + 1; the banned sequence is columns c - 1 .. c + 1
    of the plain text, so it matches across the text / path boundary of that row.  (ban, c)."""
    plain = run_loop(family, name, loop, None)
    c = 1
    for acc in plain.rounds:
        if acc >= 2:
            break
        c += acc
    else:
        raise AssertionError(f"{name} {loop}: the plain run accepts no draft")
    return Ban(sequences=[plain.out[c - 1:c + 2]]), c


@pytest.mark.parametrize("family,name", RUNS)
def test_every_speculative_loop_accepts_drafts_under_the_ban(family, name):
    """Without a round of two or more tokens no row with a path decides a token; and the round has to lie in front of the
    column up to which the text is compared with the vanilla loop's.  (Under ``no_repeat_ngram=2`` a lookup draft from the
    generated text is always the repeat of a bigram and is rejected, as it must be: the lookup loops accept under 3.)

    Where the n-gram bans leave no round of two at all, the loop runs under a third ban built to bite inside the first round of
    its plain run that accepts a draft: the chain loop of `rand`, whose random draft layer has a single guess per step (one
    accepted draft token in 62 plain rounds, behind where the n-gram bans part the text).  The two-branch lookup of `rand` has its
    rounds of two (columns 41, 45, 50 under n = 3), but only behind column 40, where two ids tie exactly and the wider pass takes
    the other one: behind a tie the texts are two valid texts and are not compared; what needs no reference still holds them
    (no repeated n-gram, every call saw the text so far), and the single-branch lookup accepts in front of column 64."""
    run, m = model_of(family, name)
    fallback = []
    for loop in loops_of(run):
        if loop == "vanilla":
            continue
        inside, deepest = [], []
        for ban in BANS:
            got, same = check_loop_against_vanilla(family, name, loop, ban)
            deepest.append(got.spy.deepest)
            w = 1
            for acc in got.rounds:
                inside.append(acc >= 2 and w + acc <= same)
                w += acc
        print(f"{name} {loop}: {sum(inside)} rounds of two or more inside the compared columns, deepest path {deepest}")
        assert min(deepest) >= 2, (loop, deepest)
        if any(inside):
            continue
        wide = max(max(run_loop(family, name, loop, ban).rounds) for ban in BANS)
        fallback.append((loop, wide))
        if wide >= 2:
            continue
        ban, c = late_sequence_ban(family, name, loop)
        got, same = check_loop_against_vanilla(family, name, loop, ban)
        plain = run_loop(family, name, loop, None)
        starts, w = {}, 1
        for acc in got.rounds:
            starts[w] = acc
            w += acc
        print(f"{name} {loop}: {ban}: the round at column {c} accepts {starts.get(c)}, {same} columns are the vanilla text")
        assert starts.get(c, 0) >= 2, "the round the ban was built for accepts no draft"
        assert same > c + 1 and got.out[:c + 1] == plain.out[:c + 1] and got.out[c + 1] != plain.out[c + 1]
        assert all(got.out[i:i + 3] != list(ban.sequences[0]) for i in range(got.n - 2))
    assert fallback == {"rand": [("chain", 1), ("lookup2", 2)]}.get(name, []), fallback


def test_magicdec_returns_the_banned_vanilla_text_on_a_long_prompt():
    family, name = "llama", "mixed@1030"
    run, m = model_of(family, name)
    assert "magicdec" in loops_of(run)
    ban = Ban(no_repeat_ngram=2)
    plain = run_loop(family, name, "vanilla", None, gen=32)
    ref = run_loop(family, name, "vanilla", ban, gen=32)
    assert bo.repeats(plain.out, 2) is not None and bo.repeats(ref.out, 2) is None
    got = run_loop(family, name, "magicdec", ban, gen=32)
    assert assert_text_or_tie(got, ref, family, name, "magicdec") >= 24 and max(got.rounds) >= 2


COMPOSED = {"penalties": ("mixed", dict(penalties=Penalties(repetition=1.1, presence=0.2))),
            "sampling": (FP16["pairs"][0][0], dict(sampling=Sampling(FP16["temperature"], FP16["top_k"], FP16["top_p"], FP16["pairs"][0][1]))),
            "logprobs": ("mixed", dict(logprobs=Logprobs(3))),
            "stop": ("mixed", {})}


@pytest.mark.parametrize("what", sorted(COMPOSED))
def test_composition(what):
    """``ban=`` with each of the other request keywords: the ban is built from the keyword's own vanilla text so that it bites
    (a bigram of that text as a banned sequence, and no repeated 2-gram), and every loop returns the vanilla loop's text."""
    family = "llama"
    name, kw = COMPOSED[what]
    run, m = model_of(family, name)
    plain = run_loop(family, name, "vanilla", None, **kw)
    seq = plain.out[5:7]
    ban = Ban(no_repeat_ngram=2, sequences=[seq])
    if what == "stop":
        # a stop id the banned text would emit at a column in front of min_tokens, for the first time there: the min_tokens
        # ban bites at that column, next to the sequence ban at column 6
        base = run_loop(family, name, "vanilla", ban).out
        c = next(c for c in range(8, 12) if base[c] not in base[:c])
        kw = dict(stop=Stop(token_ids=[base[c]], min_tokens=12))
    ref = run_loop(family, name, "vanilla", ban, **kw)
    n_ref = ref.stop[0] if ref.stop is not None and ref.stop[0] > 0 else ref.n
    assert n_ref >= 12 and ref.out[:6] == plain.out[:6] and ref.out[6] != plain.out[6], what
    assert bo.repeats(ref.out[:n_ref], 2) is None and all(ref.out[i:i + 2] != seq for i in range(n_ref - 1)), what
    if what == "stop":
        assert ref.out[:c] == base[:c] and base[c] not in ref.out[:12], what
    for loop in ("chain", "tree", "lookup1", "lookup2"):
        got = run_loop(family, name, loop, ban, **kw)
        assert got.stop == ref.stop or got.n < n_ref, (what, loop, got.stop, ref.stop)
        assert assert_text_or_tie(got, ref, family, name, (what, loop), upto=n_ref) >= 12


def test_forbidden_ids_are_never_listed_with_a_finite_logprob():
    """The log-probs are those of the banned distribution: a forbidden id that reaches the top-n listing shows -inf, the
    emitted token is never forbidden and its own log-prob is finite."""
    family, name = "llama", "mixed"
    run, m = model_of(family, name)
    V = run["cfg"].vocab_size
    first = run_loop(family, name, "vanilla", None).out[0]
    ban = Ban(no_repeat_ngram=1, sequences=[[t] for t in range(V) if t != first][:64])
    for loop in ("vanilla", "tree", "lookup2"):
        got = run_loop(family, name, loop, ban, gen=24, logprobs=Logprobs(20))
        lp = got.lp
        for c in range(got.n):
            bad = {t for t in bo.forbidden(got.out[:c], ban) if 0 <= t < V}
            assert len(bad) >= 64 and got.out[c] not in bad and torch.isfinite(lp.token[0, c]), (loop, c)
            listed = dict(zip(lp.top_ids[0, c].tolist(), lp.top[0, c].tolist()))
            assert all((v == float("-inf")) == (t in bad) for t, v in listed.items()), (loop, c, listed)
            assert int(lp.top_ids[0, c, 0]) == got.out[c]


def test_without_the_keyword_no_new_operator_is_fetched(monkeypatch):
    from longspec_amd.ban import BAN_ENV
    monkeypatch.delenv(BAN_ENV, raising=False)
    for family, name in (("llama", "mixed"), ("llama", "mixed@1030")):
        run, m = model_of(family, name)
        never = Ban(sequences=[[run["cfg"].vocab_size + 5, 3]])           # an id >= vocab is legal and never bans anything
        for loop in loops_of(run):
            plain = run_loop(family, name, loop, None, gen=16)
            assert "ban_rows" not in plain.spy.names, loop
            got = run_loop(family, name, loop, never, gen=16)
            assert got.out == plain.out, loop
            assert got.spy.names.count("ban_rows") == 1 + len(plain.rounds), loop          # the first token, then one per round
            # every other operator is called as before, in the same order
            assert [n for n in got.spy.names if n != "ban_rows"] == plain.spy.names, loop


def test_refusals():
    run, m = model_of("llama", "mixed")
    pl = torch.tensor([run["prompt_len"]])
    ban = Ban(no_repeat_ngram=2)
    real = m.model.forward
    m.model.forward = lambda *a, **k: (_ for _ in ()).throw(AssertionError("prefill before the refusal"))
    try:
        for call in (lambda: m.tree_spec_generate(run["prompt"], pl, tree_shape=run["tree_shape"], max_gen_len=16, temperature=0.5, ban=ban),
                     lambda: m.spec_generate(run["prompt"], pl, max_gen_len=16, temperature=0.5, ban=ban),
                     lambda: m.magicdec_generate(run["prompt"], pl, max_gen_len=16, temperature=0.5, ban=ban)):
            with pytest.raises(ValueError, match="temperature"):
                call()
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.tree_spec_generate(run["prompt"], pl, max_gen_len=16, shard=SimpleNamespace(vocab_parallel=True), ban=ban)
        for call in (lambda: m.vanilla_generate(run["prompt"], pl, max_gen_len=16, ban=[[3]]),
                     lambda: m.lookup_generate(run["prompt"], pl, max_gen_len=16, ban="ngram=2"),
                     lambda: m.lookup_generate(run["prompt"], pl, max_gen_len=16, branches=2, ban=2)):
            with pytest.raises(TypeError, match="longspec_amd.Ban"):
                call()
    finally:
        m.model.forward = real
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    with pytest.raises(ValueError, match="temperature"):
        m.begin_tree_decode(first, lens, run["prompt_len"], temperature=0.5, ban=ban)
    with pytest.raises(ValueError, match="temperature"):
        m.begin_chain_decode(first, lens, lens, run["prompt_len"], temperature=0.5, ban=ban)
    m.model.layers[-1].self_attn.shard = SimpleNamespace(vocab_parallel=True)
    try:
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_tree_decode(first, lens, run["prompt_len"], ban=ban)
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_chain_decode(first, lens, lens, run["prompt_len"], ban=ban)
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_vanilla_decode(torch.zeros((1, 8), dtype=torch.int64), lens.clone(), lens, run["prompt_len"], ban=ban)
        for branches in (1, 2):
            with pytest.raises(ValueError, match="vocabulary-parallel"):
                m.begin_lookup_decode(first, lens, lens, run["prompt_len"], run["prompt"], branches=branches, ban=ban)
    finally:
        m.model.layers[-1].self_attn.shard = None


def test_environment_default(monkeypatch):
    from longspec_amd.ban import BAN_ENV
    run, m = model_of("llama", "mixed")
    pl = torch.tensor([run["prompt_len"]])
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    monkeypatch.delenv(BAN_ENV, raising=False)
    assert m.begin_tree_decode(first, lens, run["prompt_len"]).ban is None
    plain = m.vanilla_generate(run["prompt"], pl, max_gen_len=GEN, eos_id=run["eos_id"])[0][0].tolist()
    monkeypatch.setenv(BAN_ENV, f"seq={plain[3]}+{plain[4]}|7,ngram=2")
    want = Ban([[plain[3], plain[4]], [7]], 2)
    assert m.begin_tree_decode(first, lens, run["prompt_len"]).ban.cfg == want
    assert m.begin_tree_decode(first, lens, run["prompt_len"], temperature=0.5).ban is None
    assert m.begin_tree_decode(first, lens, run["prompt_len"], ban=Ban([[5]])).ban.cfg == Ban([[5]])              # the argument wins
    assert m.begin_chain_decode(first, lens, lens, run["prompt_len"]).ban.cfg == want
    for branches in (1, 2):
        assert m.begin_lookup_decode(first, lens, lens, run["prompt_len"], run["prompt"], branches=branches).ban.cfg == want
    out = torch.zeros((1, 8), dtype=torch.int64)
    st = m.begin_vanilla_decode(out, lens.clone(), lens, run["prompt_len"])
    assert st.ban.cfg == want and st.ban.table.dtype == torch.int32 and bo.ban_of_table(st.ban.table) == want
    got = m.vanilla_generate(run["prompt"], pl, max_gen_len=GEN, eos_id=run["eos_id"])[0][0].tolist()
    assert got[:4] == plain[:4] and got[4] != plain[4] and bo.repeats(got, 2) is None and 7 not in got
    monkeypatch.delenv(BAN_ENV)
    assert m.vanilla_generate(run["prompt"], pl, max_gen_len=GEN, eos_id=run["eos_id"])[0][0].tolist() == plain
