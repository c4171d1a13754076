"""Token penalties and logit bias (``penalties=``) through the host loops on the CPU oracle (tests/penalty_oracle.py): the
vanilla loop is penalised decoding as ``longspec_amd/penalties.py`` defines it, the chain, tree and MagicDec loops emit the
vanilla text, the state word table is right after every loop, and the keyword's checks."""
import math

import pytest
import torch

import penalty_oracle as po
import sampled_runs as sr
from longspec_amd import Penalties, Sampling
from test_host_generate_sampled import build as _build, get_run

# (run, penalties) pairs, chosen from this file's own vanilla oracle run alone: those where the two best entries of EVERY
# penalised row are at least the project's near-tie bound apart (sampled_runs.TOL: 0.02 on fp16 logits, 0.25 on bf16) --
# asserted below; it is a condition on the inputs, not a tolerance on the code.  `name@n`: the prompt tiled to n tokens, for
# MagicDec.  fp16: the toy Llama; bf16: the Qwen2 twin.  The toy models' logits lie close together: of 7 parameter sets x 6
# runs tried in fp16, these six pairs have the margin over 20 tokens.  In bf16 (bound 0.25) no run keeps it beyond its third
# token under any of 60 sets of the three scalars, so the bf16 pairs add a steering bias -- a seeded N(0, scale^2) table over
# the vocabulary (`bias_seed`, `bias_scale`) -- under which the rows are spread far enough; that the three scalars still
# decide the text there is asserted (it differs from the text under the bias alone).
QWQ = dict(repetition=1.1, presence=0.5, frequency=0.2)
STRONG = dict(repetition=1.3, presence=0.5, frequency=0.25)
PAIRS = {
    "fp16": dict(family="llama", max_gen_len=20,
                 pairs=[("gqa_mixed", QWQ), ("gqa_mixed", dict(repetition=1.1, presence=1.0, frequency=0.5)), ("mixed@1030", STRONG),
                        ("mixed@1030", dict(presence=1e4)), ("mixed@1030", dict(repetition=1.2)),
                        ("mixed@1030", dict(presence=0.25, frequency=0.5))]),
    "bf16": dict(family="qwen2_bf16", max_gen_len=12,
                 pairs=[("qwen_bf16_g7", dict(STRONG, bias_seed=10, bias_scale=1.0)),
                        ("qwen_bf16_g5@1030", dict(STRONG, bias_seed=5, bias_scale=2.0))]),
}
# sampled with penalties: (run, seed) found as test_host_generate_sampled.py documents, on the PENALISED logits
SAMPLED = dict(family="llama", temperature=0.8, top_k=40, top_p=0.95, max_gen_len=20, penalties=QWQ,
               pairs=[("forced", 772), ("mixed", 854), ("gqa_mixed", 133), ("gqa_mixed", 206), ("mixed@1030", 287)])


def build(run):
    return _build(run, ops=po.ops)


def make_penalties(kw, V, scalars=True):
    """``Penalties`` of a pair's parameters (`scalars=False`: its bias alone)."""
    kw = dict(kw)
    seed, scale = kw.pop("bias_seed", None), kw.pop("bias_scale", None)
    bias = None
    if seed is not None:
        table = (torch.randn(V, generator=torch.Generator().manual_seed(seed)) * scale).tolist()
        bias = {i: round(v, 3) for i, v in enumerate(table)}
    return Penalties(bias=bias, **(kw if scalars else {}))


def all_pairs():
    return [pytest.param(kind, name, kw, id=f"{kind}-{name}-" + "-".join(f"{k[:3]}{v:g}" for k, v in kw.items()))
            for kind, g in PAIRS.items() for name, kw in g["pairs"]]


class RawSpy:
    """An operator namespace that forwards to `base` and keeps the raw logits of every ``penalize_rows`` call."""

    def __init__(self, base):
        self._base = base
        self.raw = []

    def __getattr__(self, name):
        return getattr(self._base, name)

    def penalize_rows(self, logits, state, penalties, extra_ids=None, extra_mask=None, bias=None):
        self.raw.append(logits.detach().clone().cpu())
        return self._base.penalize_rows(logits, state, penalties, extra_ids, extra_mask, bias=bias)


def vanilla_with_raw(m, base_ops, run, pen, gen, device=None, sampling=None):
    """(text [gen] on the CPU, the raw logits row of every token) of a spied, launch-by-launch vanilla run."""
    spy = RawSpy(base_ops)
    saved, saved_graphs = m.ops, m.GRAPH_ROUNDS
    m.ops, m.GRAPH_ROUNDS = spy, False
    try:
        ids = run["prompt"].to(device) if device else run["prompt"]
        out, _, _ = m.vanilla_generate(ids, torch.tensor([run["prompt_len"]], device=device), max_gen_len=gen,
                                       eos_id=run["eos_id"], penalties=pen, sampling=sampling)
    finally:
        m.ops, m.GRAPH_ROUNDS = saved, saved_graphs
    return out[0].cpu(), [r.reshape(-1) for r in spy.raw]


def penalised_rows(run, text, raw, pen):
    """Every token's penalised row, recomputed from the prompt and the text in front of it: [len(raw), V] in the logits' type."""
    prompt = run["prompt"][0, :run["prompt_len"]]
    rows = []
    for i, x in enumerate(raw):
        state = po.state_of(prompt, text[:i], x.numel())
        rows.append(po.penalize_rows(x.view(1, -1), state, pen).view(-1))
    return torch.stack(rows)


def top2_margin(rows):
    best = rows.float().topk(2, dim=-1).values
    return float((best[:, 0] - best[:, 1]).min())


def loops(m, run, gen, device=None, **kw):
    """{loop: (output_ids on the CPU, tokens that count)} of the speculative loops."""
    ids = run["prompt"].to(device) if device else run["prompt"]
    pl = torch.tensor([run["prompt_len"]], device=device)
    kw = dict(max_gen_len=gen, eos_id=run["eos_id"], **kw)
    outs = {}
    out, count, num, _, _ = m.spec_generate(ids, pl, gamma=4, **kw)
    outs["chain"] = (out.cpu(), min(int(count) + int(num), gen))
    if run["prompt_len"] >= 1024:
        out, count, num, _, _ = m.magicdec_generate(ids, pl, gamma=3, **kw)
        outs["magicdec"] = (out.cpu(), min(int(count) + int(num), gen))
    out, count, num, _, _ = m.tree_spec_generate(ids, pl, tree_shape=run["tree_shape"], **kw)
    outs["tree"] = (out.cpu(), min(int(count) + int(num), gen))
    return outs


def checked_vanilla(kind, name, kw, m=None):
    """The vanilla text of a pair with its conditions asserted: every token is the arg-max of its penalised row, recomputed
    from the prompt and the text so far, and the top-2 margin of every such row is at least the near-tie bound."""
    g = PAIRS[kind]
    run = get_run(g["family"], name)
    pen, gen = make_penalties(kw, run["cfg"].vocab_size), g["max_gen_len"]
    m = m or build(run)
    text, raw = vanilla_with_raw(m, po.ops, run, pen, gen)
    assert len(raw) == gen
    rows = penalised_rows(run, text, raw, pen)
    assert torch.equal(rows.float().argmax(dim=-1), text), "a token is not the arg-max of its penalised row"
    margin = top2_margin(rows)
    print(f"{kind} {name} {kw}: smallest top-2 margin of a penalised row {margin:.4f}, bound {sr.TOL[run['dtype']]}")
    assert margin >= sr.TOL[run["dtype"]], "choose another (run, penalties) pair: a penalised row is a near-tie"
    for eos in (run["eos_id"], getattr(run["cfg"], "eos_token_id", None)):
        assert eos not in text.tolist(), "the pair was chosen so that no loop stops early"
    return run, m, pen, gen, text


@pytest.mark.parametrize("kind,name,kw", all_pairs())
def test_vanilla_is_penalised_decoding_and_the_loops_agree(kind, name, kw):
    run, m, pen, gen, text = checked_vanilla(kind, name, kw)
    outs = loops(m, run, gen, penalties=pen)
    assert ("magicdec" in outs) == ("@" in name)
    for loop, (out, n) in outs.items():
        assert n >= gen - 7, (loop, n)
        assert torch.equal(out[0, :n], text[:n]), f"{loop} parts from the penalised vanilla text"


def test_the_penalty_bites():
    """Every pair's text differs from the text without its three scalars (greedy, or under the pair's bias alone)."""
    for kind, g in PAIRS.items():
        for name, kw in g["pairs"]:
            run = get_run(g["family"], name)
            m = build(run)
            V = run["cfg"].vocab_size
            pl = torch.tensor([run["prompt_len"]])
            texts = [m.vanilla_generate(run["prompt"], pl, max_gen_len=g["max_gen_len"], eos_id=run["eos_id"], penalties=p)[0]
                     for p in (make_penalties(kw, V, scalars=False), make_penalties(kw, V))]
            assert not torch.equal(texts[0], texts[1]), (kind, name, kw)


@pytest.mark.parametrize("family,name", [("llama", "forced"), ("llama", "mixed@1030"), ("qwen2_bf16", "qwen_bf16_g5")])
def test_a_large_presence_penalty_never_repeats_a_token(family, name):
    """Model-independent: 1e4 is beyond every logit of these models, so a generated token cannot win again."""
    run = get_run(family, name)
    m = build(run)
    gen = 24
    pen = Penalties(presence=1e4)
    v_out, _, _ = m.vanilla_generate(run["prompt"], torch.tensor([run["prompt_len"]]), max_gen_len=gen, eos_id=run["eos_id"], penalties=pen)
    texts = {"vanilla": (v_out, gen), **loops(m, run, gen, penalties=pen)}
    for loop, (out, n) in texts.items():
        row = out[0, :n].tolist()
        assert len(set(row)) == len(row), (loop, row)


@pytest.mark.parametrize("family,name", [("llama", "forced"), ("llama", "mixed@1030")])
def test_banned_tokens_are_never_emitted(family, name):
    run = get_run(family, name)
    m = build(run)
    gen = 20
    pl = torch.tensor([run["prompt_len"]])
    plain, _, _ = m.vanilla_generate(run["prompt"], pl, max_gen_len=gen, eos_id=run["eos_id"])
    banned = set(plain[0].tolist())
    pen = Penalties(bias={t: -math.inf for t in banned})
    v_out, _, _ = m.vanilla_generate(run["prompt"], pl, max_gen_len=gen, eos_id=run["eos_id"], penalties=pen)
    texts = {"vanilla": (v_out, gen), **loops(m, run, gen, penalties=pen)}
    for loop, (out, n) in texts.items():
        assert not banned & set(out[0, :n].tolist()), loop


def _expected_state(run, text):
    V = run["cfg"].vocab_size
    return po.state_of(run["prompt"][0, :run["prompt_len"]], text, V)


def drive_tree(m, run, pen, gen, prepare=False, sampling=None):
    """``tree_spec_generate`` spelled out through ``begin_tree_decode`` + ``tree_round``, so that the state stays in reach."""
    states = []
    orig = m.begin_tree_decode
    m.begin_tree_decode = lambda *a, **k: states.append(orig(*a, **k)) or (prepare and m.prepare_tree_graphs(states[-1])) or states[-1]
    try:
        dev = next(m.parameters()).device
        m.tree_spec_generate(run["prompt"].to(dev), torch.tensor([run["prompt_len"]], device=dev), tree_shape=run["tree_shape"],
                             max_gen_len=gen, eos_id=run["eos_id"], penalties=pen, sampling=sampling)
    finally:
        del m.begin_tree_decode
    return states[0]


def drive_chain(m, run, pen, gen, magic=False):
    states = []
    orig = m.begin_chain_decode
    m.begin_chain_decode = lambda *a, **k: states.append(orig(*a, **k)) or states[-1]
    try:
        dev = next(m.parameters()).device
        fn = m.magicdec_generate if magic else m.spec_generate
        fn(run["prompt"].to(dev), torch.tensor([run["prompt_len"]], device=dev), gamma=3 if magic else 4, max_gen_len=gen,
           eos_id=run["eos_id"], penalties=pen)
    finally:
        del m.begin_chain_decode
    return states[0]


def drive_vanilla(m, run, pen, gen):
    states = []
    orig = m.begin_vanilla_decode
    m.begin_vanilla_decode = lambda *a, **k: states.append(orig(*a, **k)) or states[-1]
    try:
        dev = next(m.parameters()).device
        m.vanilla_generate(run["prompt"].to(dev), torch.tensor([run["prompt_len"]], device=dev), max_gen_len=gen, eos_id=run["eos_id"],
                           penalties=pen)
    finally:
        del m.begin_vanilla_decode
    return states[0]


def assert_state_is_the_bincount(run, st, loop):
    """Bits 0-30 = bincount of the tokens written so far, bit 31 = membership in the prompt."""
    if loop == "vanilla":
        written = int(st.cache_lens[0]) - run["prompt_len"] + 1
    else:
        written = st.emitted
    text = st.output_ids[0, :written].cpu()
    assert torch.equal(st.token_state.cpu(), _expected_state(run, text)), f"{loop}: token_state is not the bincount of the text"


@pytest.mark.parametrize("family,name", [("llama", "mixed"), ("llama", "mixed@1030"), ("qwen2_bf16", "qwen_bf16_g5")])
def test_the_state_is_right_at_the_end_of_every_loop(family, name):
    run = get_run(family, name)
    m = build(run)
    pen = Penalties(**STRONG)
    assert_state_is_the_bincount(run, drive_vanilla(m, run, pen, 24), "vanilla")
    assert_state_is_the_bincount(run, drive_chain(m, run, pen, 24), "chain")
    assert_state_is_the_bincount(run, drive_tree(m, run, pen, 24), "tree")
    if run["prompt_len"] >= 1024:
        assert_state_is_the_bincount(run, drive_chain(m, run, pen, 24, magic=True), "magicdec")


def test_the_state_without_a_prompt_has_no_flags():
    """``prompt_ids=None``: the synthetic-KV benchmark case."""
    run = get_run("llama", "mixed")
    m = build(run)
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    for st in (m.begin_tree_decode(first, lens, run["prompt_len"], penalties=Penalties(**QWQ)),
               m.begin_chain_decode(first, lens, lens, run["prompt_len"], penalties=Penalties(**QWQ))):
        want = torch.zeros((1, run["cfg"].vocab_size), dtype=torch.int32)
        want[0, 3] = 1
        assert torch.equal(st.token_state, want)
    out = torch.zeros((1, 8), dtype=torch.int64)
    out[0, 0] = 3
    vs = m.begin_vanilla_decode(out, lens.clone(), lens, run["prompt_len"], penalties=Penalties(**QWQ), prompt_ids=run["prompt"])
    assert torch.equal(vs.token_state, _expected_state(run, torch.tensor([3])))


@pytest.mark.parametrize("name,seed", SAMPLED["pairs"])
def test_sampled_with_penalties_one_seed_one_text(name, seed):
    """The rule of tests/sampled_runs.py as it stands: its spy sees the penalised logits."""
    g = SAMPLED
    run = get_run(g["family"], name)
    T, gen, P = g["temperature"], g["max_gen_len"], run["prompt_len"]
    tol = sr.TOL[run["dtype"]]
    sampling, pen = Sampling(T, g["top_k"], g["top_p"], seed), Penalties(**g["penalties"])
    m = build(run)
    spy = sr.Top2Spy(po.ops)
    m.ops, m.GRAPH_ROUNDS = spy, False
    try:
        v_out, _, _ = m.vanilla_generate(run["prompt"], torch.tensor([P]), max_gen_len=gen, eos_id=run["eos_id"], sampling=sampling,
                                         penalties=pen)
    finally:
        m.ops, m.GRAPH_ROUNDS = po.ops, True
    rec = {pos: v for (s, pos), v in spy.rec.items() if s == 0}
    rec["rows"] = {pos: v for (s, pos), v in spy.rows.items() if s == 0}
    for eos in (run["eos_id"], getattr(run["cfg"], "eos_token_id", None)):
        assert eos not in v_out[0].tolist()
    gap, robust = sr.min_gap(rec, gen, P), sr.min_robust_gap(rec, gen, P, sampling, tol)
    print(f"{name} seed {seed}: smallest key gap {gap:.3f}, against the tokens a filter could keep {robust:.3f}, wide margin {8 * tol / T:.3f}")
    assert gap >= 8 * tol / T and robust >= 8 * tol / T, "choose another (seed, prompt) pair"
    for loop, (out, n) in loops(m, run, gen, penalties=pen, sampling=sampling).items():
        assert n >= gen - 7, (loop, n)
        assert sr.parting(out, n, v_out, rec, P, T, tol, loop) is None, f"{loop} parts from the vanilla text"


def test_refusals_come_before_any_device_work():
    from types import SimpleNamespace
    run = get_run("llama", "mixed")
    m = build(run)

    class NoWork:
        def __getattr__(self, name):
            raise AssertionError(f"device work ({name}) before the refusal")

    real = m.model.forward
    m.model.forward = lambda *a, **k: (_ for _ in ()).throw(AssertionError("prefill before the refusal"))
    try:
        pl = torch.tensor([run["prompt_len"]])
        pen = Penalties(**QWQ)
        for call in (lambda: m.tree_spec_generate(run["prompt"], pl, tree_shape=run["tree_shape"], max_gen_len=16, temperature=0.5, penalties=pen),
                     lambda: m.spec_generate(run["prompt"], pl, max_gen_len=16, temperature=0.5, penalties=pen),
                     lambda: m.magicdec_generate(run["prompt"], pl, max_gen_len=16, temperature=0.5, penalties=pen)):
            with pytest.raises(ValueError, match="temperature"):
                call()
        shard = SimpleNamespace(vocab_parallel=True)
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.tree_spec_generate(run["prompt"], pl, max_gen_len=16, shard=shard, penalties=pen)
    finally:
        m.model.forward = real
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    with pytest.raises(ValueError, match="temperature"):
        m.begin_tree_decode(first, lens, run["prompt_len"], temperature=0.5, penalties=pen)
    with pytest.raises(ValueError, match="temperature"):
        m.begin_chain_decode(first, lens, lens, run["prompt_len"], temperature=0.5, penalties=pen)
    m.model.layers[-1].self_attn.shard = SimpleNamespace(vocab_parallel=True)
    with pytest.raises(ValueError, match="vocabulary-parallel"):
        m.begin_tree_decode(first, lens, run["prompt_len"], penalties=pen)
    with pytest.raises(ValueError, match="vocabulary-parallel"):
        m.begin_chain_decode(first, lens, lens, run["prompt_len"], penalties=pen)
    with pytest.raises(ValueError, match="vocabulary-parallel"):
        m.begin_vanilla_decode(torch.zeros((1, 8), dtype=torch.int64), lens.clone(), lens, run["prompt_len"], penalties=pen)
    m.model.layers[-1].self_attn.shard = None
    with pytest.raises(TypeError):
        m.vanilla_generate(run["prompt"], pl, max_gen_len=16, penalties=1.1)


def test_penalties_validate_their_arguments():
    p = Penalties(1.1, 0.5, 0.2, bias={3: -math.inf, 1: 0.5})
    assert (p.repetition, p.presence, p.frequency, dict(p.bias)) == (1.1, 0.5, 0.2, {1: 0.5, 3: -math.inf})
    assert p == Penalties(1.1, 0.5, 0.2, {1: 0.5, 3: -math.inf}) and p != Penalties(1.1, 0.5, 0.2)
    assert Penalties() == Penalties(1.0, 0.0, 0.0, None) and Penalties().changes_nothing and not p.changes_nothing
    for bad in (dict(repetition=0), dict(repetition=-1), dict(repetition=math.nan), dict(repetition=math.inf), dict(presence=math.inf),
                dict(presence=math.nan), dict(frequency=-math.inf), dict(frequency=math.nan), dict(bias={1: math.nan}),
                dict(bias={1: math.inf}), dict(bias={-1: 0.5}), dict(bias={1.5: 0.5})):
        with pytest.raises(ValueError):
            Penalties(**bad)
    with pytest.raises(TypeError):
        Penalties(bias=[1, 2])
    with pytest.raises(ValueError, match="vocabulary"):
        Penalties(bias={512: 1.0}).bias_table(512, "cpu")
    t = p.bias_table(8, "cpu")
    assert t.dtype == torch.float32 and t.tolist() == [0.0, 0.5, 0.0, -math.inf, 0.0, 0.0, 0.0, 0.0] and p.bias_table(8, "cpu") is not t


def test_environment_default_and_a_penalty_that_changes_nothing(monkeypatch):
    from longspec_amd.penalties import PENALTIES_ENV, env_penalties, resolve
    monkeypatch.delenv(PENALTIES_ENV, raising=False)
    assert env_penalties() is None
    monkeypatch.setenv(PENALTIES_ENV, "rep=1.1,pres=0.5,freq=0.2")
    assert env_penalties() == Penalties(1.1, 0.5, 0.2) == Penalties.parse("freq=0.2, rep=1.1,pres=0.5")
    for bad in ("rep", "rep=abc", "rep=1.1,rep=1.2", "k=3", "rep=0", "1.1"):
        monkeypatch.setenv(PENALTIES_ENV, bad)
        with pytest.raises(ValueError):
            env_penalties()
    run = get_run("llama", "mixed")
    m = build(run)
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    monkeypatch.setenv(PENALTIES_ENV, "rep=1.3,pres=0.5,freq=0.25")
    assert m.begin_tree_decode(first, lens, run["prompt_len"]).penalties == Penalties(**STRONG)
    assert m.begin_tree_decode(first, lens, run["prompt_len"], temperature=0.5).penalties is None
    assert m.begin_tree_decode(first, lens, run["prompt_len"], penalties=Penalties(**QWQ)).penalties == Penalties(**QWQ)
    assert m.begin_tree_decode(first, lens, run["prompt_len"], penalties=Penalties()).penalties is None      # the argument wins
    assert m.begin_chain_decode(first, lens, lens, run["prompt_len"]).penalties == Penalties(**STRONG)
    out = torch.zeros((1, 8), dtype=torch.int64)
    assert m.begin_vanilla_decode(out, lens.clone(), lens, run["prompt_len"]).penalties == Penalties(**STRONG)
    pl = torch.tensor([run["prompt_len"]])
    env_out, _, _ = m.vanilla_generate(run["prompt"], pl, max_gen_len=12, eos_id=run["eos_id"])
    monkeypatch.setenv(PENALTIES_ENV, "rep=1.0")
    assert m.begin_tree_decode(first, lens, run["prompt_len"]).penalties is None
    monkeypatch.delenv(PENALTIES_ENV)
    assert m.begin_tree_decode(first, lens, run["prompt_len"]).penalties is None
    arg_out, _, _ = m.vanilla_generate(run["prompt"], pl, max_gen_len=12, eos_id=run["eos_id"], penalties=Penalties(**STRONG))
    assert torch.equal(env_out, arg_out)
    # Penalties() resolves to None: a loop given it makes exactly the calls it makes today
    assert resolve(Penalties(), None, True) is None and resolve(Penalties(bias={4: 0.0}), None, True) is None

    class Counting:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            fn = getattr(po.ops, name)
            if not callable(fn):
                return fn

            def call(*a, **k):
                self.calls.append(name)
                return fn(*a, **k)
            return call

    traces = []
    for pen in (None, Penalties()):
        m.ops = spy = Counting()
        out, count, num, _, _ = m.tree_spec_generate(run["prompt"], pl, tree_shape=run["tree_shape"], max_gen_len=16,
                                                     eos_id=run["eos_id"], penalties=pen)
        traces.append((spy.calls, out.tolist(), int(count), int(num)))
    m.ops = po.ops
    assert traces[0] == traces[1] and "penalize_rows" not in traces[0][0] and "token_state_add" not in traces[0][0]
