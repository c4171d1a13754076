"""The DRY penalty (``dry=``) through the host loops on the CPU oracle (tests/dry_oracle.py), on the toy runs of
test_host_generate_ban.py at 64 columns: the plain texts loop and the DRY texts do not, every loop returns the DRY vanilla text,
every round hands the operator the text so far, paths in depth order and a zeroed scratch that is large enough, the rule sits
behind the penalties and in front of the bans, the keyword composes with ``sampling=`` / ``penalties=`` / ``logprobs=`` /
``stop=`` / ``ban=`` / ``guide=``, and without the keyword no new operator is fetched."""
from types import SimpleNamespace

import pytest
import torch

import ban_oracle as bo
import dry_oracle as do
import test_host_generate_ban as hb
import test_host_generate_guide as hg
from longspec_amd import Ban, Dry, Logprobs, Penalties, Sampling, Stop
from test_host_generate_sampled import FP16, build as _build, get_run
from test_host_generate_stop import CallSpy

GEN = 64
RUNS = hb.RUNS
G = 4                                   # gamma of the chain and lookup loops
_models, _cache = {}, {}
loops_of, tree_shape_of, text_of = hb.loops_of, hb.tree_shape_of, hb.text_of

# HARD: a repeat of two tokens may not be extended -- the penalty of 1000 is beyond every logit of the toy models, so the text
# holds no 3-gram twice (what Ban(no_repeat_ngram=3) enforces with -inf).  SOFT: the arithmetic decides, token by token.
HARD = Dry(1000.0, 1.0, 2)
SOFT = Dry(1.5, 1.75, 2)
DRYS = [HARD, SOFT]


def model_of(family, name):
    if (family, name) not in _models:
        run = get_run(family, name)
        _models[family, name] = (run, _build(run, ops=do.ops))
    return _models[family, name]


class Spy(CallSpy):
    """``CallSpy`` (operator names, ``chain_commit`` / ``tree_collapse`` events) that checks every ``dry_rows`` call as it
    comes -- the selected extras of every row, in increasing column, lie at depths 1, 2, 3 ...; the scratch is int32, all zero
    and holds an element per logit -- and keeps the committed text the call saw and the rows it returned."""

    def __init__(self, base):
        super().__init__(base)
        self.seen, self.rows, self.deepest = [], [], 0

    def dry_rows(self, logits, table, output_ids, scratch, base=None, base_sub=None, base_add=0, extra_ids=None, extra_mask=None):
        self.names.append("dry_rows")
        R = logits.shape[1] if logits.dim() == 3 else 1
        assert scratch.dtype == torch.int32 and scratch.is_contiguous() and scratch.numel() >= logits.numel()
        assert int(scratch.count_nonzero()) == 0
        if extra_ids is not None:
            mask = extra_mask if extra_mask.dim() == 3 else extra_mask[None]
            assert tuple(mask.shape[1:]) == (R, extra_ids.shape[1]) and R == extra_ids.shape[1] + 1
            depth = [int(mask[0, c + 1].ne(0).sum()) for c in range(extra_ids.shape[1])]     # column c is row c + 1's own token
            for r in range(R):
                on_path = [depth[c] for c in range(extra_ids.shape[1]) if int(mask[0, r, c]) != 0]
                assert on_path == list(range(1, len(on_path) + 1)), (r, on_path)
                self.deepest = max(self.deepest, len(on_path))
        texts = bo.row_texts(logits.shape[0], R, output_ids, base, base_sub, base_add, extra_ids, extra_mask)
        out = self._base.dry_rows(logits, table, output_ids, scratch, base=base, base_sub=base_sub, base_add=base_add,
                                  extra_ids=extra_ids, extra_mask=extra_mask)
        self.seen.append(texts[0][0])                                     # row 0 follows no extra: the committed text
        self.rows.append(out.detach().clone().reshape(-1, out.shape[-1]))
        return out


def run_loop(family, name, loop, dry, gen=GEN, **kw):
    """One loop under the spy: out (a list), n text columns, the rounds' accepted counts, the spy, last_logprobs, last_stop."""
    key = (family, name, loop, dry, gen)
    if not kw and key in _cache:
        return _cache[key]
    run, m = model_of(family, name)
    spy = Spy(do.ops)
    saved, m.ops = m.ops, spy
    try:
        ids, pl = run["prompt"], torch.tensor([run["prompt_len"]])
        kw = dict(max_gen_len=gen, eos_id=run["eos_id"], dry=dry, **kw)
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
    if set(kw) == {"max_gen_len", "eos_id", "dry"}:
        _cache[key] = got
    return got


def assert_text_or_tie(got, ref, family, name, what, upto=None):
    """``hb.assert_text_or_tie`` on this module's models: the loop's text is the vanilla loop's (same keywords), or parts from
    it at a column where the vanilla loop's own two best entries are closer than the dtype's near-tie bound."""
    saved = hb.model_of
    hb.model_of = model_of
    try:
        return hb.assert_text_or_tie(got, ref, family, name, what, upto)
    finally:
        hb.model_of = saved


def longest_repeat(text):
    """The longest verbatim repeat the text holds: the largest n with a repeated n-gram."""
    n = 0
    while bo.repeats(text, n + 1) is not None:
        n += 1
    return n


@pytest.mark.parametrize("family,name", RUNS)
def test_the_plain_texts_loop_and_the_dry_texts_do_not(family, name):
    plain = run_loop(family, name, "vanilla", None)
    assert plain.n == GEN and "dry_rows" not in plain.spy.names
    first = bo.repeats(plain.out, 3)
    assert first is not None, "the plain text must extend a repeat, or the test shows nothing"
    print(f"{name}: the plain text first repeats a 3-gram at column {first}; its longest repeat has {longest_repeat(plain.out)} tokens")
    for dry in DRYS:
        got = run_loop(family, name, "vanilla", dry)
        assert got.spy.names.count("dry_rows") == GEN                     # the first token's row and one per step
        rows = torch.cat(got.spy.rows)
        assert rows.float().argmax(dim=-1).tolist() == got.out            # every token is the arg-max of the row handed back
        assert got.spy.seen == [got.out[:c] for c in range(GEN)]          # ... and the row saw the text so far
        print(f"{name} {dry}: longest repeat {longest_repeat(got.out)}")
        assert got.out != plain.out and longest_repeat(got.out) <= longest_repeat(plain.out)
        same = hb.common(got.out, plain.out)
        assert same >= min(first, 2)                                      # nothing is penalised in front of the first repeat of two
        if dry is HARD:
            assert bo.repeats(got.out, 3) is None and same == first      # parts exactly where the plain text repeats a 3-gram
    assert longest_repeat(run_loop(family, name, "vanilla", HARD).out) < longest_repeat(plain.out)


def check_loop_against_vanilla(family, name, loop, dry):
    """The loop's text under ``dry`` is the vanilla loop's up to an explained near-tie, and every round's operator call saw the
    text so far.  Returns the run."""
    ref = run_loop(family, name, "vanilla", dry)
    got = run_loop(family, name, loop, dry)
    same = assert_text_or_tie(got, ref, family, name, (name, loop, dry))
    assert same >= 24 and got.n >= GEN - 24, (loop, same, got.n)
    w = 1
    assert got.spy.seen[0] == [] and len(got.spy.seen) == 1 + len(got.rounds)
    for seen, acc in zip(got.spy.seen[1:], got.rounds):
        assert seen == got.out[:w], (loop, w)
        w += acc
    return got, same


@pytest.mark.parametrize("family,name", RUNS)
@pytest.mark.parametrize("dry", DRYS, ids=["hard", "soft"])
def test_every_loop_returns_the_dry_vanilla_text(family, name, dry):
    run, m = model_of(family, name)
    deepest = 0
    for loop in loops_of(run):
        if loop == "vanilla":
            continue
        got, same = check_loop_against_vanilla(family, name, loop, dry)
        deepest = max(deepest, got.spy.deepest)
        if dry is HARD:
            assert bo.repeats(text_of(got)[:same], 3) is None, loop
    assert deepest >= 2                                                   # rows with a path of two draft tokens were ruled


def test_magicdec_returns_the_dry_vanilla_text_on_a_long_prompt():
    family, name = "llama", "mixed@1030"
    run, m = model_of(family, name)
    assert "magicdec" in loops_of(run)
    plain = run_loop(family, name, "vanilla", None, gen=32)
    ref = run_loop(family, name, "vanilla", HARD, gen=32)
    assert bo.repeats(plain.out, 3) is not None and bo.repeats(ref.out, 3) is None
    got = run_loop(family, name, "magicdec", HARD, gen=32)
    assert assert_text_or_tie(got, ref, family, name, "magicdec") >= 24 and max(got.rounds) >= 2


def composed(what, run, m):
    V = run["cfg"].vocab_size
    if what == "penalties":
        return dict(penalties=Penalties(presence=0.05))                   # (mild: the penalised text still repeats a 3-gram)
    if what == "sampling":
        return dict(sampling=Sampling(FP16["temperature"], FP16["top_k"], FP16["top_p"], FP16["pairs"][0][1]))
    if what == "logprobs":
        return dict(logprobs=Logprobs(3))
    if what == "ban":
        return dict(ban=Ban(no_repeat_ngram=4))
    if what == "guide":
        return dict(guide=hg.parity_guide(V, hg.eos_of(run, m), 0))
    return {}


@pytest.mark.parametrize("what", ["ban", "guide", "logprobs", "penalties", "sampling", "stop"])
def test_composition(what):
    """``dry=`` with each of the other request keywords: every loop returns the vanilla loop's text under the same keywords,
    the DRY penalty changes that text, and the operators of a pass come in the documented order."""
    family = "llama"
    name = FP16["pairs"][0][0] if what == "sampling" else "mixed"
    run, m = model_of(family, name)
    kw = composed(what, run, m)
    # (the sampled text repeats a 2-gram in its 64 columns and no 3-gram: there no repeat of ONE token may be extended)
    dry = SOFT if what == "logprobs" else Dry(1000.0, 1.0, 1) if what == "sampling" else HARD
    if what == "stop":
        # a stop id the DRY text emits at a column in front of min_tokens, for the first time there: the min_tokens ban bites
        base = run_loop(family, name, "vanilla", dry).out
        c = next(c for c in range(8, 14) if base[c] not in base[:c])
        kw = dict(stop=Stop(token_ids=[base[c]], min_tokens=14))
    without = run_loop(family, name, "vanilla", None, **kw)
    ref = run_loop(family, name, "vanilla", dry, **kw)
    n_ref = ref.stop[0] if ref.stop is not None and ref.stop[0] > 0 else ref.n
    assert n_ref >= 12 and ref.out[:n_ref] != without.out[:n_ref], what
    if dry.multiplier == 1000.0:
        assert bo.repeats(ref.out[:n_ref], dry.allowed_length + 1) is None, what
    rules = ("penalize_rows", "dry_rows", "stop_ban_rows", "ban_rows", "guide_rows")
    order = [n for n in ref.spy.names if n in rules]
    want = [n for n in rules if n in order]                               # the documented order of a pass
    assert len(want) == (1 if what in ("logprobs", "sampling") else 2) and order == want * ref.spy.names.count("dry_rows"), order[:6]
    if what == "logprobs":                                                # the log-probs are those of the penalised rows
        lp = torch.log_softmax(torch.cat(ref.spy.rows).float(), dim=-1)
        for c in range(GEN):
            assert abs(float(ref.lp.token[0, c]) - float(lp[c, ref.out[c]])) < 1e-3, c
    for loop in ("chain", "tree", "lookup1", "lookup2"):
        got = run_loop(family, name, loop, dry, **kw)
        assert got.stop == ref.stop or got.n < n_ref, (what, loop, got.stop, ref.stop)
        assert assert_text_or_tie(got, ref, family, name, (what, loop), upto=n_ref) >= 12


def test_without_the_keyword_no_new_operator_is_fetched(monkeypatch):
    from longspec_amd.dry import DRY_ENV
    monkeypatch.delenv(DRY_ENV, raising=False)
    never = Dry(1.0, last_n=1)                                            # one token is looked at: nothing can match
    for family, name in (("llama", "mixed"), ("llama", "mixed@1030")):
        run, m = model_of(family, name)
        for loop in loops_of(run):
            plain = run_loop(family, name, loop, None, gen=16)
            assert "dry_rows" not in plain.spy.names, loop
            # the operator names of a run without the keyword are those of the same run on the operators of the ban tests
            old = hb.run_loop(family, name, loop, None, gen=16)
            assert plain.spy.names == old.spy.names and plain.out == old.out, loop
            got = run_loop(family, name, loop, never, gen=16)
            assert got.out == plain.out, loop
            assert got.spy.names.count("dry_rows") == 1 + len(plain.rounds), loop          # the first token, then one per round
            assert [n for n in got.spy.names if n != "dry_rows"] == plain.spy.names, loop


def test_refusals():
    run, m = model_of("llama", "mixed")
    pl = torch.tensor([run["prompt_len"]])
    dry = Dry(0.8)
    real = m.model.forward
    m.model.forward = lambda *a, **k: (_ for _ in ()).throw(AssertionError("prefill before the refusal"))
    try:
        for call in (lambda: m.tree_spec_generate(run["prompt"], pl, tree_shape=run["tree_shape"], max_gen_len=16, temperature=0.5, dry=dry),
                     lambda: m.spec_generate(run["prompt"], pl, max_gen_len=16, temperature=0.5, dry=dry),
                     lambda: m.magicdec_generate(run["prompt"], pl, max_gen_len=16, temperature=0.5, dry=dry)):
            with pytest.raises(ValueError, match="temperature"):
                call()
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.tree_spec_generate(run["prompt"], pl, max_gen_len=16, shard=SimpleNamespace(vocab_parallel=True), dry=dry)
        for call in (lambda: m.vanilla_generate(run["prompt"], pl, max_gen_len=16, dry=0.8),
                     lambda: m.lookup_generate(run["prompt"], pl, max_gen_len=16, dry="mult=0.8"),
                     lambda: m.lookup_generate(run["prompt"], pl, max_gen_len=16, branches=2, dry=Ban(no_repeat_ngram=2))):
            with pytest.raises(TypeError, match="longspec_amd.Dry"):
                call()
    finally:
        m.model.forward = real
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    with pytest.raises(ValueError, match="temperature"):
        m.begin_tree_decode(first, lens, run["prompt_len"], temperature=0.5, dry=dry)
    with pytest.raises(ValueError, match="temperature"):
        m.begin_chain_decode(first, lens, lens, run["prompt_len"], temperature=0.5, dry=dry)
    m.model.layers[-1].self_attn.shard = SimpleNamespace(vocab_parallel=True)
    try:
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_tree_decode(first, lens, run["prompt_len"], dry=dry)
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_chain_decode(first, lens, lens, run["prompt_len"], dry=dry)
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_vanilla_decode(torch.zeros((1, 8), dtype=torch.int64), lens.clone(), lens, run["prompt_len"], dry=dry)
        for branches in (1, 2):
            with pytest.raises(ValueError, match="vocabulary-parallel"):
                m.begin_lookup_decode(first, lens, lens, run["prompt_len"], run["prompt"], branches=branches, dry=dry)
    finally:
        m.model.layers[-1].self_attn.shard = None


def test_environment_default(monkeypatch):
    from longspec_amd.dry import DRY_ENV
    run, m = model_of("llama", "mixed")
    pl = torch.tensor([run["prompt_len"]])
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    monkeypatch.delenv(DRY_ENV, raising=False)
    assert m.begin_tree_decode(first, lens, run["prompt_len"]).dry is None
    plain = m.vanilla_generate(run["prompt"], pl, max_gen_len=GEN, eos_id=run["eos_id"])[0][0].tolist()
    monkeypatch.setenv(DRY_ENV, do.spec_of(HARD))
    assert m.begin_tree_decode(first, lens, run["prompt_len"]).dry.cfg == HARD
    assert m.begin_tree_decode(first, lens, run["prompt_len"], temperature=0.5).dry is None
    assert m.begin_tree_decode(first, lens, run["prompt_len"], dry=SOFT).dry.cfg == SOFT                          # the argument wins
    assert m.begin_chain_decode(first, lens, lens, run["prompt_len"]).dry.cfg == HARD
    for branches in (1, 2):
        assert m.begin_lookup_decode(first, lens, lens, run["prompt_len"], run["prompt"], branches=branches).dry.cfg == HARD
    out = torch.zeros((1, 8), dtype=torch.int64)
    st = m.begin_vanilla_decode(out, lens.clone(), lens, run["prompt_len"])
    assert st.dry.cfg == HARD and st.dry.table.dtype == torch.int32 and do.params_of_table(st.dry.table).pen == HARD.penalties()
    got = m.vanilla_generate(run["prompt"], pl, max_gen_len=GEN, eos_id=run["eos_id"])[0][0].tolist()
    assert got == run_loop("llama", "mixed", "vanilla", HARD).out and got != plain and bo.repeats(got, 3) is None
    monkeypatch.delenv(DRY_ENV)
    assert m.vanilla_generate(run["prompt"], pl, max_gen_len=GEN, eos_id=run["eos_id"])[0][0].tolist() == plain
