"""Watermarked decoding (``watermark=``) through the host loops on the CPU oracle (tests/watermark_oracle.py), on the toy runs of
test_host_generate_ban.py at 64 columns: the plain texts carry no mark and the marked texts do, every loop returns the
watermarked vanilla text, every round hands the operator the text so far and paths in depth order, the rule sits behind the
penalties and the DRY penalty and in front of the bans (``stop=`` under ``min_tokens`` among them), the keyword composes with
``sampling=`` / ``penalties=`` / ``logprobs=`` / ``ban=`` / ``guide=`` / ``dry=``, and without the keyword no new operator is fetched."""
from types import SimpleNamespace

import pytest
import torch

import ban_oracle as bo
import test_host_generate_ban as hb
import test_host_generate_dry as hd
import test_host_generate_guide as hg
import watermark_oracle as wo
from longspec_amd import Ban, Dry, Logprobs, Penalties, Sampling, Stop, Watermark
from test_host_generate_sampled import FP16, build as _build, get_run
from test_host_generate_stop import CallSpy

GEN = 64
RUNS = hb.RUNS
G = 4                                   # gamma of the chain and lookup loops
_models, _cache = {}, {}
loops_of, tree_shape_of, text_of = hb.loops_of, hb.tree_shape_of, hb.text_of

# HARD: the delta of 1000 is beyond every logit of the toy models, so every token behind the first h is green.  SOFT: the
# arithmetic decides, token by token.
# The key was picked on the CPU, by a scan of the keys 1 .. 43200 over the toy runs, for three conditions on the inputs:
# * no plain text looks marked under HARD, for contexts 1 and 3: |z| < 2.5 (asserted below).  (Not under SOFT: the `forced` run's
#   plain text says two tokens in turn, two positions said 31 times each, so at p = 0.25 its z is one of -4.6 / 4.6 / 13.7
#   whatever the key; there the test counts every distinct position once, ``unique=True``.)
# * no marked text emits EOS inside its 64 columns (asserted below: every vanilla run has 64 steps).
# * the toy models' logits are flat -- the two best entries of a row are often a few units in the last place apart -- and a
#   loop may part from the vanilla text at such a row, which ``assert_text_or_tie`` explains but which must not happen inside
#   the first 24 columns (12 in the composition test).  Which of two such entries wins there is a matter of the machine's last
#   bit, so the key is one under which the marked vanilla runs hold no such row (two best entries closer than 3 units in the
#   last place of the 16-bit type) inside those windows under SOFT: two keys of the 43 200 do, and this one also has none in the
#   composition runs.  Under HARD nearly every row is one -- x + 1000 lies on a grid of 0.5 (fp16) or 4 (bf16), most green ids
#   tie exactly and a last-bit difference can move an id across a bucket edge -- and under a context of 3 the bf16 run has five
#   or more in its first 24 columns under every key.  So the loops are held to the vanilla text under SOFT; HARD and the
#   context of 3 are held to their counts on the vanilla loop, the context of 3 runs through every loop in the operator-order
#   test, and HARD through the loops on the device (tests/test_gpu_generate_watermark.py), where the arithmetic is one machine's.
KEY = 14496
HARD = Watermark(KEY, 0.5, 1000.0)
HARD3 = Watermark(KEY, 0.5, 1000.0, context=3)
SOFT = Watermark(KEY, 0.25, 2.0)
SOFT3 = Watermark(KEY, 0.25, 2.0, context=3)                              # (the context straddles the text / path seam)


def model_of(family, name):
    if (family, name) not in _models:
        run = get_run(family, name)
        _models[family, name] = (run, _build(run, ops=wo.ops))
    return _models[family, name]


class Spy(CallSpy):
    """``CallSpy`` (operator names, ``chain_commit`` / ``tree_collapse`` events) that checks every ``watermark_rows`` call as it
    comes -- the selected extras of every row, in increasing column, lie at depths 1, 2, 3 ... -- and keeps the committed text
    the call saw and the rows it returned."""

    def __init__(self, base):
        super().__init__(base)
        self.seen, self.rows, self.deepest = [], [], 0

    def watermark_rows(self, logits, table, output_ids, base=None, base_sub=None, base_add=0, extra_ids=None, extra_mask=None):
        self.names.append("watermark_rows")
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
        out = self._base.watermark_rows(logits, table, output_ids, base=base, base_sub=base_sub, base_add=base_add,
                                        extra_ids=extra_ids, extra_mask=extra_mask)
        self.seen.append(texts[0][0])                                     # row 0 follows no extra: the committed text
        self.rows.append(out.detach().clone().reshape(-1, out.shape[-1]))
        return out


def run_loop(family, name, loop, watermark, gen=GEN, **kw):
    """One loop under the spy: out (a list), n text columns, the rounds' accepted counts, the spy, last_logprobs, last_stop."""
    key = (family, name, loop, watermark, gen)
    if not kw and key in _cache:
        return _cache[key]
    run, m = model_of(family, name)
    spy = Spy(wo.ops)
    saved, m.ops = m.ops, spy
    try:
        ids, pl = run["prompt"], torch.tensor([run["prompt_len"]])
        kw = dict(max_gen_len=gen, eos_id=run["eos_id"], watermark=watermark, **kw)
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
    if set(kw) == {"max_gen_len", "eos_id", "watermark"}:
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


def detect(wm, text):
    got = wm.detect(torch.tensor(text))
    return int(got.scored[0]), int(got.green[0]), float(got.z[0])


@pytest.mark.parametrize("family,name", RUNS)
def test_the_plain_texts_carry_no_mark_and_the_marked_texts_do(family, name):
    plain = run_loop(family, name, "vanilla", None)
    assert plain.n == GEN and "watermark_rows" not in plain.spy.names
    for wm in (HARD, HARD3, SOFT):
        h = wm.context
        N, Gn, z = detect(wm, plain.out)
        if wm is SOFT:
            z = float(wm.detect(torch.tensor(plain.out), unique=True).z[0])
        print(f"{name} {wm}: the plain text has {Gn} green of {N}, z = {z:.2f}")
        assert N == GEN - h and abs(z) < 2.5, "the plain text must not look marked, or the test shows nothing"
        got = run_loop(family, name, "vanilla", wm)
        assert got.spy.names.count("watermark_rows") == GEN               # the first token's row and one per step
        rows = torch.cat(got.spy.rows)
        assert rows.float().argmax(dim=-1).tolist() == got.out            # every token is the arg-max of the row handed back
        assert got.spy.seen == [got.out[:c] for c in range(GEN)]          # ... and the row saw the text so far
        assert got.out != plain.out
        assert got.out[:h] == plain.out[:h]                               # the first h rows are unmarked
        N, Gn, z = detect(wm, got.out)
        print(f"{name} {wm}: the marked text has {Gn} green of {N}, z = {z:.2f}")
        assert (N, Gn, z) == wo.score(got.out, wm.key, wm.gamma, h)[:3]
        if wm is not SOFT:
            assert Gn == N == GEN - h and z > 6                            # (p = 0.5, N = 63: 7.9)
        else:
            assert z > detect(wm, plain.out)[2]


def check_loop_against_vanilla(family, name, loop, wm):
    """The loop's text under ``wm`` is the vanilla loop's up to an explained near-tie, and every round's operator call saw the
    text so far.  Returns the run."""
    ref = run_loop(family, name, "vanilla", wm)
    got = run_loop(family, name, loop, wm)
    same = assert_text_or_tie(got, ref, family, name, (name, loop, wm))
    assert same >= 24 and got.n >= GEN - 24, (loop, same, got.n)
    w = 1
    assert got.spy.seen[0] == [] and len(got.spy.seen) == 1 + len(got.rounds)
    for seen, acc in zip(got.spy.seen[1:], got.rounds):
        assert seen == got.out[:w], (loop, w)
        w += acc
    return got, same


@pytest.mark.parametrize("family,name", RUNS)
def test_every_loop_returns_the_watermarked_vanilla_text(family, name, wm=SOFT):
    run, m = model_of(family, name)
    deepest = 0
    for loop in loops_of(run):
        if loop == "vanilla":
            continue
        got, same = check_loop_against_vanilla(family, name, loop, wm)
        deepest = max(deepest, got.spy.deepest)
    assert deepest >= 2                                                   # rows with a path of two draft tokens were ruled


def test_magicdec_returns_the_watermarked_vanilla_text_on_a_long_prompt():
    family, name = "llama", "mixed@1030"
    run, m = model_of(family, name)
    assert "magicdec" in loops_of(run)
    plain = run_loop(family, name, "vanilla", None, gen=32)
    ref = run_loop(family, name, "vanilla", SOFT, gen=32)
    assert ref.out != plain.out
    got = run_loop(family, name, "magicdec", SOFT, gen=32)
    assert assert_text_or_tie(got, ref, family, name, "magicdec") >= 24 and max(got.rounds) >= 2


def test_the_operator_order_of_a_pass():
    """penalties, dry, watermark, the ``min_tokens`` ban, ban, guide: the documented order, in every pass of every loop."""
    family, name = "llama", "mixed"
    run, m = model_of(family, name)
    V = run["cfg"].vocab_size
    kw = dict(penalties=Penalties(presence=0.05), dry=Dry(0.8), stop=Stop(token_ids=[V - 1], min_tokens=60),
              ban=Ban(no_repeat_ngram=4), guide=hg.parity_guide(V, hg.eos_of(run, m), 0))
    rules = ["penalize_rows", "dry_rows", "watermark_rows", "stop_ban_rows", "ban_rows", "guide_rows"]
    for loop in ("vanilla", "chain", "tree", "lookup1", "lookup2"):
        got = run_loop(family, name, loop, SOFT3, gen=24, **kw)             # (a context that straddles the text / path seam)
        order = [n for n in got.spy.names if n in rules]
        passes = got.spy.names.count("watermark_rows")
        assert passes >= 2 and order == rules * passes, (loop, order[:8])


def composed(what, run, m):
    V = run["cfg"].vocab_size
    if what == "penalties":
        return dict(penalties=Penalties(presence=0.05))
    if what == "sampling":
        return dict(sampling=Sampling(FP16["temperature"], FP16["top_k"], FP16["top_p"], FP16["pairs"][0][1]))
    if what == "logprobs":
        return dict(logprobs=Logprobs(3))
    if what == "ban":
        return dict(ban=Ban(no_repeat_ngram=4))
    if what == "dry":
        return dict(dry=hd.HARD)
    if what == "guide":
        return dict(guide=hg.parity_guide(V, hg.eos_of(run, m), 0))
    return {}


@pytest.mark.parametrize("what", ["ban", "dry", "guide", "logprobs", "penalties", "sampling"])
def test_composition(what):
    """``watermark=`` with each of the other request keywords: every loop returns the vanilla loop's text under the same
    keywords, the watermark changes that text, and the operators of a pass come in the documented order."""
    family = "llama"
    name = FP16["pairs"][0][0] if what == "sampling" else "mixed"
    run, m = model_of(family, name)
    kw = composed(what, run, m)
    wm = SOFT
    without = run_loop(family, name, "vanilla", None, **kw)
    ref = run_loop(family, name, "vanilla", wm, **kw)
    n_ref = ref.stop[0] if ref.stop is not None and ref.stop[0] > 0 else ref.n
    assert n_ref >= 12 and ref.out[:n_ref] != without.out[:n_ref], what
    rules = ("penalize_rows", "dry_rows", "watermark_rows", "stop_ban_rows", "ban_rows", "guide_rows")
    order = [n for n in ref.spy.names if n in rules]
    want = [n for n in rules if n in order]                               # the documented order of a pass
    assert len(want) == (1 if what in ("logprobs", "sampling") else 2) and order == want * ref.spy.names.count("watermark_rows"), order[:6]
    if what == "logprobs":                                                # the log-probs are those of the marked rows
        lp = torch.log_softmax(torch.cat(ref.spy.rows).float(), dim=-1)
        for c in range(GEN):
            assert abs(float(ref.lp.token[0, c]) - float(lp[c, ref.out[c]])) < 1e-3, c
    for loop in ("chain", "tree", "lookup1", "lookup2"):
        got = run_loop(family, name, loop, wm, **kw)
        assert got.stop == ref.stop or got.n < n_ref, (what, loop, got.stop, ref.stop)
        assert assert_text_or_tie(got, ref, family, name, (what, loop), upto=n_ref) >= 12


def test_without_the_keyword_no_new_operator_is_fetched(monkeypatch):
    from longspec_amd.watermark import WATERMARK_ENV
    monkeypatch.delenv(WATERMARK_ENV, raising=False)
    for family, name in (("llama", "mixed"), ("llama", "mixed@1030")):
        run, m = model_of(family, name)
        for loop in loops_of(run):
            plain = run_loop(family, name, loop, None, gen=16)
            assert "watermark_rows" not in plain.spy.names, loop
            # the operator names and the text of a run without the keyword are those of the dry tests' run without dry=
            old = hd.run_loop(family, name, loop, None, gen=16)
            assert plain.spy.names == old.spy.names and plain.out == old.out, loop
            got = run_loop(family, name, loop, SOFT, gen=16)
            assert got.spy.names.count("watermark_rows") == 1 + len(got.rounds), loop        # the first token, then one per round
            assert "watermark_rows" in got.spy.names and set(got.spy.names) - {"watermark_rows"} == set(plain.spy.names), loop


def test_refusals():
    run, m = model_of("llama", "mixed")
    pl = torch.tensor([run["prompt_len"]])
    wm = Watermark(5)
    real = m.model.forward
    m.model.forward = lambda *a, **k: (_ for _ in ()).throw(AssertionError("prefill before the refusal"))
    try:
        for call in (lambda: m.tree_spec_generate(run["prompt"], pl, tree_shape=run["tree_shape"], max_gen_len=16, temperature=0.5, watermark=wm),
                     lambda: m.spec_generate(run["prompt"], pl, max_gen_len=16, temperature=0.5, watermark=wm),
                     lambda: m.magicdec_generate(run["prompt"], pl, max_gen_len=16, temperature=0.5, watermark=wm)):
            with pytest.raises(ValueError, match="temperature"):
                call()
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.tree_spec_generate(run["prompt"], pl, max_gen_len=16, shard=SimpleNamespace(vocab_parallel=True), watermark=wm)
        for call in (lambda: m.vanilla_generate(run["prompt"], pl, max_gen_len=16, watermark=5),
                     lambda: m.lookup_generate(run["prompt"], pl, max_gen_len=16, watermark="key=5"),
                     lambda: m.lookup_generate(run["prompt"], pl, max_gen_len=16, branches=2, watermark=Ban(no_repeat_ngram=2))):
            with pytest.raises(TypeError, match="longspec_amd.Watermark"):
                call()
    finally:
        m.model.forward = real
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    with pytest.raises(ValueError, match="temperature"):
        m.begin_tree_decode(first, lens, run["prompt_len"], temperature=0.5, watermark=wm)
    with pytest.raises(ValueError, match="temperature"):
        m.begin_chain_decode(first, lens, lens, run["prompt_len"], temperature=0.5, watermark=wm)
    m.model.layers[-1].self_attn.shard = SimpleNamespace(vocab_parallel=True)
    try:
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_tree_decode(first, lens, run["prompt_len"], watermark=wm)
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_chain_decode(first, lens, lens, run["prompt_len"], watermark=wm)
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_vanilla_decode(torch.zeros((1, 8), dtype=torch.int64), lens.clone(), lens, run["prompt_len"], watermark=wm)
        for branches in (1, 2):
            with pytest.raises(ValueError, match="vocabulary-parallel"):
                m.begin_lookup_decode(first, lens, lens, run["prompt_len"], run["prompt"], branches=branches, watermark=wm)
    finally:
        m.model.layers[-1].self_attn.shard = None


def test_environment_default(monkeypatch):
    from longspec_amd.watermark import WATERMARK_ENV
    run, m = model_of("llama", "mixed")
    pl = torch.tensor([run["prompt_len"]])
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    monkeypatch.delenv(WATERMARK_ENV, raising=False)
    assert m.begin_tree_decode(first, lens, run["prompt_len"]).watermark is None
    plain = m.vanilla_generate(run["prompt"], pl, max_gen_len=GEN, eos_id=run["eos_id"])[0][0].tolist()
    monkeypatch.setenv(WATERMARK_ENV, wo.spec_of(HARD))
    assert m.begin_tree_decode(first, lens, run["prompt_len"]).watermark.cfg == HARD
    assert m.begin_tree_decode(first, lens, run["prompt_len"], temperature=0.5).watermark is None
    assert m.begin_tree_decode(first, lens, run["prompt_len"], watermark=SOFT).watermark.cfg == SOFT             # the argument wins
    assert m.begin_chain_decode(first, lens, lens, run["prompt_len"]).watermark.cfg == HARD
    for branches in (1, 2):
        assert m.begin_lookup_decode(first, lens, lens, run["prompt_len"], run["prompt"], branches=branches).watermark.cfg == HARD
    out = torch.zeros((1, 8), dtype=torch.int64)
    st = m.begin_vanilla_decode(out, lens.clone(), lens, run["prompt_len"])
    p = wo.params_of_table(st.watermark.table)
    assert st.watermark.cfg == HARD and st.watermark.table.dtype == torch.int32 and (p.key, p.h, p.delta) == (HARD.key, 1, 1000.0)
    got = m.vanilla_generate(run["prompt"], pl, max_gen_len=GEN, eos_id=run["eos_id"])[0][0].tolist()
    assert got == run_loop("llama", "mixed", "vanilla", HARD).out and got != plain and detect(HARD, got)[:2] == (63, 63)
    monkeypatch.delenv(WATERMARK_ENV)
    assert m.vanilla_generate(run["prompt"], pl, max_gen_len=GEN, eos_id=run["eos_id"])[0][0].tolist() == plain
