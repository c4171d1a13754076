"""Stop conditions (``stop=``) through the host loops on the CPU oracle (tests/stop_oracle.py): every loop returns exactly the
oracle's cut of its own plain text -- inside a round, across rounds, on column 0 --, ``last_stop`` is the oracle's triple, the
four loops agree, the log-probs are cut with the text, ``min_tokens`` is banned decoding, and the keyword's checks."""
from types import SimpleNamespace

import pytest
import torch

import sampled_runs as sr
import stop_oracle as so
import test_host_generate_logprobs as hl
from longspec_amd import Logprobs, Penalties, Stop
from test_host_generate_penalized import top2_margin
from test_host_generate_sampled import build as _build, get_run

KEYS = ["greedy-mixed", "greedy-bf16", "greedy-long", "sampled-forced"]
GEN = 16
TOP_N = 2
# Every speculative loop of every configuration has a round that accepts two tokens or more (asserted), with one exception: the
# chain loop's greedy drafter never gets a second SAMPLED token accepted on `sampled-forced` (15 rounds of one token).  That
# loop derives no stops of its own there; it still runs with every stop the tree loop of that configuration derives.
NO_WIDE_ROUND = {("sampled-forced", "chain")}
LAST_COL = 9          # the tree loop emits only 10-14 columns at this GEN: stop columns come from the columns every loop emits


def build(run):
    return _build(run, ops=so.ops)


def loops_of(run):
    return ["vanilla", "chain", "tree"] + (["magicdec"] if run["prompt_len"] >= 1024 else [])


def fill_of(m, run, loop):
    return m._tree_output_fill(run["eos_id"]) if loop == "tree" else 0


class CallSpy(hl.Spy):
    """``hl.Spy`` that also keeps the name of every operator a loop fetches, in order."""

    def __init__(self, base):
        super().__init__(base)
        self.names = []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._base, name)


def run_loop(m, loop, run, sampling, stop, logprobs=Logprobs(TOP_N), pen=None, device=None, spy_on=so.ops):
    """One loop: a namespace of out [W] (a list), lp, last_stop (a triple, or None), the accepted count of every round, the
    number n of text columns and the operator names.  ``spy_on=None``: the model's own operators, unspied (a device run that
    may replay graphs): no rounds, and n is the number of columns that hold a log-prob."""
    spy = CallSpy(spy_on) if spy_on is not None else None
    saved = m.ops
    if spy is not None:
        m.ops = spy
    try:
        ids, pl = run["prompt"].to(device or "cpu"), torch.tensor([run["prompt_len"]], device=device)
        kw = dict(max_gen_len=GEN, eos_id=run["eos_id"], sampling=sampling, penalties=pen, logprobs=logprobs, stop=stop)
        if loop == "vanilla":
            out = m.vanilla_generate(ids, pl, **kw)[0]
        elif loop == "chain":
            out = m.spec_generate(ids, pl, gamma=4, **kw)[0]
        elif loop == "magicdec":
            out = m.magicdec_generate(ids, pl, gamma=3, **kw)[0]
        else:
            out = m.tree_spec_generate(ids, pl, tree_shape=run["tree_shape"], **kw)[0]
    finally:
        m.ops = saved
    events = spy.events if spy is not None else []
    rounds = [int(e[2][0]) for e in events if e[0] == "tree"] if loop == "tree" else \
        [int(e[1][0]) for e in events if e[0] == "chain"] if loop != "vanilla" else [1] * (GEN - 1)
    ls = m.last_stop
    triple = None if ls is None else (int(ls.length[0]), int(ls.which[0]), int(ls.match_start[0]))
    lp = m.last_logprobs
    if lp is not None:
        lp = SimpleNamespace(token=lp.token.clone().cpu(), top=lp.top.clone().cpu(), top_ids=lp.top_ids.clone().cpu())
    n = 1 + sum(rounds) if spy is not None else int((~torch.isnan(lp.token[0])).sum()) if lp is not None else None
    return SimpleNamespace(out=out[0].tolist(), lp=lp, stop=triple, rounds=rounds, n=n,
                           names=spy.names if spy is not None else None)


def derive_stops(plain, loop):
    """The stops of test 1 from a speculative loop's plain run: {kind: (Stop, column it must match at)}.  A candidate counts
    only when the oracle says it matches first at the intended column."""
    text = plain.out[:plain.n]
    starts, c0 = [], 1
    for acc in plain.rounds:
        starts.append((c0, acc))
        c0 += acc
    wide = [(c, acc) for c, acc in starts if acc >= 2]
    assert wide, f"{loop}: no round accepted two tokens or more"
    found = {}

    def take(kind, stop, c):
        if kind not in found and c <= LAST_COL and so.scan(text, stop)[0] == c + 1:
            found[kind] = (stop, c)

    for c, acc in wide:
        take("id-inside-a-round", Stop(token_ids=[text[c]]), c)                          # the cut falls strictly inside
        take("bigram-inside-a-round", Stop(sequences=[text[c:c + 2]]), c + 1)
    for c, acc in starts[1:]:
        take("bigram-across-rounds", Stop(sequences=[text[c - 1:c + 1]]), c)
    found["column-0"] = (Stop(token_ids=[text[0]]), 0)
    return found


_plain, _models = {}, {}


def model_of(key):
    if key not in _models:
        family, name, sampling, pen_kw = hl.CONFIGS[key]
        run = get_run(family, name)
        _models[key] = (run, sampling, build(run))
    return _models[key]


def plain_runs(key, **kw):
    """{loop: plain run} of a configuration, computed once."""
    if key not in _plain:
        run, sampling, m = model_of(key)
        _plain[key] = {loop: run_loop(m, loop, run, sampling, None, **kw) for loop in loops_of(run)}
    return _plain[key]


def check_cut(got, plain, stop, fill, loop, what):
    """``got`` (a run with ``stop``) is the oracle's cut of ``plain`` (the same loop without)."""
    length, which, start = so.scan(plain.out[:plain.n], stop)
    assert length > 0, (what, loop, "the stop does not match the plain text")
    assert got.stop == (length, which, start), (what, loop, got.stop)
    assert got.out == plain.out[:length] + [fill] * (len(plain.out) - length), (what, loop, got.out, plain.out)
    assert so.cut(plain.out, plain.n, stop, fill)[0][:plain.n] == got.out[:plain.n], (what, loop)
    if plain.lp is not None:
        for name in ("token", "top", "top_ids"):
            g, p = getattr(got.lp, name)[0], getattr(plain.lp, name)[0]
            assert torch.equal(hl.bits(g[:length].contiguous()), hl.bits(p[:length].contiguous())), (what, loop, name)
        assert torch.isnan(got.lp.token[0, length:]).all() and (got.lp.top_ids[0, length:] == -1).all(), (what, loop)
        assert (got.lp.top[0, length:] == float("-inf")).all(), (what, loop)


@pytest.mark.parametrize("key", KEYS)
def test_every_loop_returns_the_oracles_cut_of_its_plain_text(key):
    run, sampling, m = model_of(key)
    plain = plain_runs(key)
    for eos in (run["eos_id"], getattr(run["cfg"], "eos_token_id", None)):
        assert all(eos not in p.out[:p.n] for p in plain.values()), "the built-in stop id occurs in a text"
    assert all(p.n > LAST_COL and p.stop is None for p in plain.values())
    stops = {}
    for loop, p in plain.items():
        if loop == "vanilla":
            continue
        if (key, loop) in NO_WIDE_ROUND:
            assert max(p.rounds) == 1, f"{key} {loop}: the exemption is out of date"
            continue
        assert max(p.rounds) >= 2, f"{loop}: no round accepted two tokens or more"
        found = derive_stops(p, loop)
        assert set(found) == {"id-inside-a-round", "bigram-inside-a-round", "bigram-across-rounds", "column-0"}, (loop, sorted(found))
        for kind, (stop, c) in found.items():
            stops.setdefault(stop, f"{kind} of {loop} at column {c}")
    for stop, what in stops.items():
        res = {loop: run_loop(m, loop, run, sampling, stop) for loop in plain}
        for loop, got in res.items():
            check_cut(got, plain[loop], stop, fill_of(m, run, loop), loop, what)
        length = res["vanilla"].stop[0]
        for loop, got in res.items():                               # ... and the four loops agree with each other
            assert got.stop == res["vanilla"].stop and got.out[:length] == res["vanilla"].out[:length], (what, loop)


def test_a_stopped_state_is_final_and_counts_are_not_rolled_back():
    run, sampling, m = model_of("greedy-mixed")
    p = plain_runs("greedy-mixed")["tree"]
    stop, c = derive_stops(p, "tree")["id-inside-a-round"]
    states = []
    for what in ("begin_tree_decode", "begin_chain_decode"):
        orig = getattr(m, what)
        setattr(m, what, lambda *a, _o=orig, **k: states.append(_o(*a, **k)) or states[-1])
    try:
        run_loop(m, "tree", run, sampling, stop)
        run_loop(m, "chain", run, sampling, stop)
    finally:
        del m.begin_tree_decode, m.begin_chain_decode
    tree, chain = states
    assert tree.stopped and chain.stopped and tree.emitted > c + 1          # the overshoot stays counted
    spy = CallSpy(so.ops)
    m.ops = spy
    try:
        assert m.tree_round(tree) is False and m.chain_round(chain) is False
    finally:
        m.ops = so.ops
    assert spy.names == [], "a round on a stopped state did device work"


def test_batched_vanilla_rows_stop_on_their_own_and_keep_their_tails_erased():
    """Two rows that stop at different steps (and one that never stops): every row is the cut of its own plain text, the row
    that stopped first stays erased while the batch decodes on, and the loop's timing ends with the last row's stop."""
    run, sampling, m = model_of("greedy-mixed")
    ids = torch.cat([run["prompt"], run["prompt"].roll(3, 1)], 0)
    pl = torch.tensor([run["prompt_len"]] * 2)
    kw = dict(max_gen_len=GEN, eos_id=run["eos_id"], logprobs=Logprobs(1))
    plain = m.vanilla_generate(ids, pl, **kw)[0].tolist()
    plain_lp = m.last_logprobs
    assert not set(plain[0]) & set(plain[1])
    for stop in (Stop(token_ids=[plain[1][9], plain[0][3]]), Stop(token_ids=[plain[0][3]]), Stop(sequences=[plain[1][4:6]], token_ids=[plain[0][12]])):
        out, num, elapsed = m.vanilla_generate(ids, pl, stop=stop, **kw)
        ls, lp = m.last_stop, m.last_logprobs
        assert num == 2 * (GEN - 1)                                  # the steps that ran: not rolled back
        for z in range(2):
            want, triple = so.cut(plain[z], GEN, stop, 0)
            assert out[z].tolist() == want and (int(ls.length[z]), int(ls.which[z]), int(ls.match_start[z])) == triple, (stop, z)
            n = triple[0] if triple[0] > 0 else GEN
            assert torch.equal(hl.bits(lp.token[z, :n].contiguous()), hl.bits(plain_lp.token[z, :n].contiguous())), (stop, z)
            assert torch.isnan(lp.token[z, n:]).all() and (lp.top_ids[z, n:] == -1).all(), (stop, z)
        assert elapsed > 0


# ---- min_tokens: (config, column of the plain text whose token becomes the stop id, min_tokens) -- pairs where every row of the
# banned vanilla run keeps the project's near-tie bound between its two best entries (asserted below: a condition on the
# inputs, as in the penalised host tests).  Found by trying columns 0..5 x three minima per run: no pair of the bf16 run keeps
# its bound of 0.25 (the penalised tests met the same and steer with a bias); the ban itself is exact in bf16 in
# tests/test_gpu_stop_ban_rows.py.  `greedy-long`, column 4: the banned id comes back at column 9 >= min_tokens and stops the run.
BANNED = [("greedy-mixed", 3, 7), ("greedy-long", 4, 8), ("greedy-long", 1, 9)]


class BanSpy:
    """Keeps every row ``stop_ban_rows`` returned (vanilla: one per token)."""

    def __init__(self, base):
        self._base = base
        self.rows = []

    def __getattr__(self, name):
        return getattr(self._base, name)

    def stop_ban_rows(self, logits, table, **kw):
        raw = logits.detach().clone()
        out = self._base.stop_ban_rows(logits, table, **kw)
        self.rows.append((raw.reshape(-1, raw.shape[-1]), out.detach().clone().reshape(-1, raw.shape[-1])))
        return out


@pytest.mark.parametrize("key,col,min_tokens", BANNED)
def test_min_tokens_is_banned_decoding_in_every_loop(key, col, min_tokens):
    run, sampling, m = model_of(key)
    text = plain_runs(key)["vanilla"].out
    stop = Stop(token_ids=[text[col]], min_tokens=min_tokens)
    assert col < min_tokens and so.scan(text, stop)[0] != col + 1
    spy = BanSpy(so.ops)
    m.ops = spy
    try:
        out = m.vanilla_generate(run["prompt"], torch.tensor([run["prompt_len"]]), max_gen_len=GEN, eos_id=run["eos_id"],
                                 sampling=sampling, stop=stop)[0][0].tolist()
        triple = tuple(int(t[0]) for t in (m.last_stop.length, m.last_stop.which, m.last_stop.match_start))
    finally:
        m.ops = so.ops
    assert len(spy.rows) == GEN                                              # the first token's row and one per step
    n = triple[0] if triple[0] > 0 else GEN
    rows = torch.cat([r[1] for r in spy.rows])[:n]
    for c, (raw, banned) in enumerate(spy.rows[:n]):
        want = raw.clone()
        if c < min_tokens:
            want[:, text[col]] = float("-inf")
        assert torch.equal(hl.bits(banned.float()), hl.bits(want.float())), f"column {c}"
    assert rows.float().argmax(dim=-1).tolist() == out[:n], "a token is not the arg-max of its banned row"
    assert text[col] not in out[:min_tokens] and out[:col] == text[:col] and out[col] != text[col]
    margin = top2_margin(rows)
    print(f"{key}: smallest top-2 margin of a banned run's row {margin:.4f}, bound {sr.TOL[run['dtype']]}")
    assert margin >= sr.TOL[run["dtype"]], "choose another (run, stop) pair: a row of the banned run is a near-tie"
    assert triple == so.scan(out[:n], stop) and out[n:] == [0] * (GEN - n)
    for loop in loops_of(run):
        got = run_loop(m, loop, run, sampling, stop)
        k = min(n, got.n) if triple[0] < 0 else n
        assert got.stop == triple and got.out[:k] == out[:k], (loop, got.out, out)
        assert k > min_tokens, loop


def test_a_banned_row_never_emits_a_banned_id_and_its_logprob_is_finite():
    family, name, sampling, pen_kw = hl.CONFIGS["sampled-penalised-mixed"]
    run = get_run(family, name)
    m = build(run)
    pen = Penalties(**pen_kw)
    plain = run_loop(m, "vanilla", run, sampling, None, pen=pen)
    banned = sorted(set(plain.out[:8]))
    stop = Stop(token_ids=banned, min_tokens=GEN)
    for loop in loops_of(run):
        got = run_loop(m, loop, run, sampling, stop, pen=pen)
        assert got.stop == (-1, -1, -1) and got.n > LAST_COL, loop
        assert not set(banned) & set(got.out[:got.n]), (loop, got.out)
        assert torch.isfinite(got.lp.token[0, :got.n]).all(), loop
        for c in range(got.n):                                  # the log-probs are those of the banned distribution
            listed = got.lp.top_ids[0, c].tolist()
            assert not set(banned) & set(listed), (loop, c, listed)


def test_refusals():
    run = get_run("llama", "mixed")
    m = build(run)
    pl = torch.tensor([run["prompt_len"]])
    stop = Stop(token_ids=[3])
    real = m.model.forward
    m.model.forward = lambda *a, **k: (_ for _ in ()).throw(AssertionError("prefill before the refusal"))
    try:
        for call in (lambda: m.tree_spec_generate(run["prompt"], pl, tree_shape=run["tree_shape"], max_gen_len=16, temperature=0.5, stop=stop),
                     lambda: m.spec_generate(run["prompt"], pl, max_gen_len=16, temperature=0.5, stop=stop),
                     lambda: m.magicdec_generate(run["prompt"], pl, max_gen_len=16, temperature=0.5, stop=stop)):
            with pytest.raises(ValueError, match="temperature"):
                call()
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.tree_spec_generate(run["prompt"], pl, max_gen_len=16, shard=SimpleNamespace(vocab_parallel=True),
                                 stop=Stop(token_ids=[3], min_tokens=1))
        with pytest.raises(TypeError):
            m.vanilla_generate(run["prompt"], pl, max_gen_len=16, stop=[3])
        with pytest.raises(ValueError, match="vocabulary"):
            m.vanilla_generate(run["prompt"], pl, max_gen_len=16, stop=Stop(token_ids=[run["cfg"].vocab_size]))
    finally:
        m.model.forward = real
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    with pytest.raises(ValueError, match="temperature"):
        m.begin_tree_decode(first, lens, run["prompt_len"], temperature=0.5, stop=stop)
    with pytest.raises(ValueError, match="temperature"):
        m.begin_chain_decode(first, lens, lens, run["prompt_len"], temperature=0.5, stop=stop)
    m.model.layers[-1].self_attn.shard = SimpleNamespace(vocab_parallel=True)
    try:
        banned = Stop(token_ids=[3], min_tokens=2)
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_tree_decode(first, lens, run["prompt_len"], stop=banned)
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_chain_decode(first, lens, lens, run["prompt_len"], stop=banned)
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_vanilla_decode(torch.zeros((1, 8), dtype=torch.int64), lens.clone(), lens, run["prompt_len"], stop=banned)
        st = m.begin_tree_decode(first, lens, run["prompt_len"], stop=stop)            # without min_tokens the shard is fine
        assert st.last_stop.length.tolist() == [1] and st.stop_state.dtype == torch.int32
    finally:
        m.model.layers[-1].self_attn.shard = None


def test_environment_default(monkeypatch):
    from longspec_amd.stop import STOP_ENV
    run = get_run("llama", "mixed")
    m = build(run)
    pl = torch.tensor([run["prompt_len"]])
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    monkeypatch.delenv(STOP_ENV, raising=False)
    st = m.begin_tree_decode(first, lens, run["prompt_len"])
    assert st.stop is None and st.last_stop is None and st.stop_state is None
    plain = m.vanilla_generate(run["prompt"], pl, max_gen_len=12, eos_id=run["eos_id"])[0][0].tolist()
    assert m.last_stop is None
    monkeypatch.setenv(STOP_ENV, f"ids={plain[4]},seq={plain[2]}+{plain[3]}|7,min=1")
    want = Stop([plain[4]], [[plain[2], plain[3]], [7]], 1)
    assert m.begin_tree_decode(first, lens, run["prompt_len"]).stop.cfg == want
    assert m.begin_tree_decode(first, lens, run["prompt_len"], temperature=0.5).stop is None
    assert m.begin_tree_decode(first, lens, run["prompt_len"], stop=Stop([5])).stop.cfg == Stop([5])        # the argument wins
    assert m.begin_chain_decode(first, lens, lens, run["prompt_len"]).stop.cfg == want
    out = torch.zeros((1, 8), dtype=torch.int64)
    assert m.begin_vanilla_decode(out, lens.clone(), lens, run["prompt_len"]).stop.cfg == want
    cut = m.vanilla_generate(run["prompt"], pl, max_gen_len=12, eos_id=run["eos_id"])[0][0].tolist()
    length, which, start = so.scan(plain, want)
    assert (int(m.last_stop.length[0]), int(m.last_stop.which[0]), int(m.last_stop.match_start[0])) == (length, which, start)
    assert length == 4 and which == 1 and cut == plain[:length] + [0] * (12 - length)
    monkeypatch.delenv(STOP_ENV)
    m.vanilla_generate(run["prompt"], pl, max_gen_len=12, eos_id=run["eos_id"])
    assert m.last_stop is None


@pytest.mark.parametrize("key", ["greedy-mixed", "greedy-long"])
def test_without_the_keyword_neither_new_operator_is_called(key):
    run, sampling, m = model_of(key)
    never = Stop(token_ids=[run["cfg"].vocab_size - 1], sequences=[[run["cfg"].vocab_size - 1] * 3])
    new = {"stop_scan", "stop_ban_rows"}
    for loop in loops_of(run):
        plain = run_loop(m, loop, run, sampling, None, logprobs=None)
        assert not new & set(plain.names), loop
        with_stop = run_loop(m, loop, run, sampling, never, logprobs=None)
        assert with_stop.stop == (-1, -1, -1) and with_stop.out == plain.out
        assert "stop_scan" in with_stop.names and "stop_ban_rows" not in with_stop.names        # no ban without min_tokens
        # every other operator is called as before, in the same order: the plain run is the run with stop= minus its scans
        assert [n for n in with_stop.names if n not in new] == plain.names, loop
        assert with_stop.names.count("stop_scan") == 1 + len(plain.rounds), loop                 # column 0, then one per round
