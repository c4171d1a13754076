"""Log-probabilities of the emitted tokens (``logprobs=``) through the host loops on the CPU oracle (tests/logprob_oracle.py):
the keyword changes no token, every emitted column holds -- bit for bit -- the values of the verification row on the accepted
path and every other column the fill, the first alternative of a greedy row is the emitted token, the four loops agree on the
log-probs of a common text, and the keyword's checks."""
from types import SimpleNamespace

import pytest
import torch

import logprob_oracle as lo
import sampled_runs as sr
from longspec_amd import Logprobs, Penalties, Sampling
from test_host_generate_penalized import QWQ, SAMPLED
from test_host_generate_sampled import FP16, BF16, build as _build, get_run

# (family, run, sampling, penalties): greedy, sampled, and sampled with penalties; `name@1030` also runs MagicDec, so the
# fourth loop runs under each of the three
_S16 = lambda seed: Sampling(FP16["temperature"], FP16["top_k"], FP16["top_p"], seed)
_SP = lambda seed: Sampling(SAMPLED["temperature"], SAMPLED["top_k"], SAMPLED["top_p"], seed)
CONFIGS = {
    "greedy-mixed": ("llama", "mixed", None, None),
    "greedy-gqa-penalised": ("llama", "gqa_mixed", None, QWQ),
    "greedy-bf16": ("qwen2_bf16", "qwen_bf16_g5", None, None),
    "greedy-long": ("llama", "mixed@1030", None, None),
    "sampled-forced": ("llama", "forced", _S16(384), None),
    "sampled-long": ("llama", "mixed@1030", _S16(328), None),
    "sampled-bf16": ("qwen2_bf16", "qwen_bf16_g7", Sampling(BF16["temperature"], seed=488), None),
    "sampled-penalised-mixed": ("llama", "mixed", _SP(854), QWQ),
    "sampled-penalised-long": ("llama", "mixed@1030", _SP(287), QWQ),
}
GEN = 16
TOP_N = 3


def build(run):
    return _build(run, ops=lo.ops)


def bits(t):
    """Bit patterns: NaN fills compare equal to themselves."""
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class Spy:
    """An operator namespace that forwards to `base` and keeps, in call order, the rows every ``token_logprobs`` call returned
    and what the round's own operators said was accepted (``tree_collapse``: index_mapping and acc_num; ``chain_commit``:
    correct_len)."""

    def __init__(self, base):
        self._base = base
        self.events = []

    def __getattr__(self, name):
        return getattr(self._base, name)

    def token_logprobs(self, logits, ids, temperature=1.0, n=0):
        rows = self._base.token_logprobs(logits, ids, temperature, n)
        self.events.append(("rows", tuple(t.clone() for t in rows), ids.clone().reshape(rows[0].shape), float(temperature)))
        return rows

    def tree_collapse(self, *a, **k):
        out = self._base.tree_collapse(*a, **k)
        self.events.append(("tree", out[3].clone(), out[1].clone()))
        return out

    def chain_commit(self, *a, **k):
        state = self._base.chain_commit(*a, **k)
        self.events.append(("chain", state[:, 0].clone()))
        return state


def run_loop(m, loop, run, sampling, pen, logprobs, spy_on=lo.ops, device=None):
    """(output_ids, count, num, last_logprobs, events) of one loop; ``spy_on``: the operators to spy on (None: the model's own,
    unspied -- a device run, which may replay graphs)."""
    spy = Spy(spy_on) if spy_on is not None else None
    saved = m.ops
    if spy is not None:
        m.ops = spy
    try:
        ids, pl = run["prompt"].to(device or "cpu"), torch.tensor([run["prompt_len"]], device=device)
        kw = dict(max_gen_len=GEN, eos_id=run["eos_id"], sampling=sampling, penalties=pen, logprobs=logprobs)
        if loop == "vanilla":
            out, num, _ = m.vanilla_generate(ids, pl, **kw)
            count = 0
        elif loop == "chain":
            out, count, num, _, _ = m.spec_generate(ids, pl, gamma=4, **kw)
        elif loop == "magicdec":
            out, count, num, _, _ = m.magicdec_generate(ids, pl, gamma=3, **kw)
        else:
            out, count, num, _, _ = m.tree_spec_generate(ids, pl, tree_shape=run["tree_shape"], **kw)
    finally:
        m.ops = saved
    return out.clone(), int(count), int(num), m.last_logprobs, spy.events if spy is not None else None


def expected_buffers(loop, events, width, n):
    """The three buffers rebuilt from the spied rows alone, and the number of columns emitted."""
    from longspec_amd.logprobs import new_buffers
    want = new_buffers(1, width, n, "cpu")

    def put(col, rows, src):
        want.token[0, col], want.top[0, col], want.top_ids[0, col] = rows[0][0, src], rows[1][0, src], rows[2][0, src]

    rows_events = [e for e in events if e[0] == "rows"]
    put(0, rows_events[0][1], 0)                                  # the first token: one row, column 0
    emitted = 1
    if loop == "vanilla":
        for e in rows_events[1:]:
            put(emitted, e[1], 0)
            emitted += 1
        return want, emitted
    rows = accepted = None               # a round's rows and what its own operators accepted, in either call order
    for e in events[events.index(rows_events[0]) + 1:]:
        if e[0] == "rows":
            rows = e[1]
        elif e[0] == "tree" and loop == "tree":
            accepted = [int(e[1][0, j]) for j in range(int(e[2][0]))]           # index_mapping[:acc_num]
        elif e[0] == "chain" and loop != "tree":
            accepted = list(range(int(e[1][0])))                                # the first correct_len rows
        if rows is not None and accepted is not None:
            for j, src in enumerate(accepted):
                put(emitted + j, rows, src)
            emitted += len(accepted)
            rows = accepted = None
    return want, emitted


_cache = {}


def runs_of(key):
    """{loop: result of `run_loop`} with and without ``logprobs=`` for one configuration."""
    if key not in _cache:
        family, name, sampling, pen_kw = CONFIGS[key]
        run = get_run(family, name)
        pen = Penalties(**pen_kw) if pen_kw else None
        m = build(run)
        loops = ["vanilla", "chain", "tree"] + (["magicdec"] if run["prompt_len"] >= 1024 else [])
        _cache[key] = (run, sampling, {loop: (run_loop(m, loop, run, sampling, pen, Logprobs(TOP_N)),
                                              run_loop(m, loop, run, sampling, pen, None)) for loop in loops})
    return _cache[key]


@pytest.mark.parametrize("key", list(CONFIGS))
def test_the_keyword_changes_no_token(key):
    run, sampling, res = runs_of(key)
    assert ("magicdec" in res) == (run["prompt_len"] >= 1024)
    for loop, (with_lp, without) in res.items():
        assert torch.equal(with_lp[0], without[0]) and with_lp[1:3] == without[1:3], loop
        assert without[3] is None and not [e for e in without[4] if e[0] == "rows"], f"{loop}: log-prob work without the keyword"
        assert with_lp[3] is not None


@pytest.mark.parametrize("key", list(CONFIGS))
def test_every_emitted_column_holds_the_accepted_rows_values_and_the_rest_the_fill(key):
    run, sampling, res = runs_of(key)
    T = sampling.temperature if sampling is not None else 1.0
    for loop, ((out, count, num, lp, events), _) in res.items():
        assert lp.token.shape == out.shape and lp.top.shape == (*out.shape, TOP_N) == lp.top_ids.shape, loop
        assert all(e[3] == T for e in events if e[0] == "rows"), f"{loop}: the sampler's temperature"
        want, emitted = expected_buffers(loop, events, out.size(1), TOP_N)
        eos = m_eos(run)
        if loop == "vanilla" and eos in out[0].tolist():                # the cut of output_ids, on the same columns
            stop = max(out[0].tolist().index(eos), 1)
            want.token[:, stop + 1:], want.top[:, stop + 1:], want.top_ids[:, stop + 1:] = float("nan"), float("-inf"), -1
            emitted = min(emitted, stop + 1)
        assert emitted >= 8, (loop, emitted)
        for name in ("token", "top", "top_ids"):
            assert torch.equal(bits(getattr(lp, name)), bits(getattr(want, name))), f"{loop}: {name}"
        assert not torch.isnan(lp.token[0, :emitted]).any() and torch.isnan(lp.token[0, emitted:]).all(), loop
        assert (lp.top_ids[0, emitted:] == -1).all() and (lp.top[0, emitted:] == float("-inf")).all(), loop
        first = next(e for e in events if e[0] == "rows")               # the rows were taken for the emitted tokens themselves
        assert int(first[2][0, 0]) == int(out[0, 0]), loop


def m_eos(run):
    return getattr(run["cfg"], "eos_token_id", None) if run["family"] != "qwen2" else run["eos_id"]


@pytest.mark.parametrize("key", [k for k in CONFIGS if k.startswith("greedy")])
def test_the_first_alternative_of_a_greedy_row_is_the_emitted_token(key):
    run, sampling, res = runs_of(key)
    for loop, ((out, count, num, lp, events), _) in res.items():
        emitted = int((~torch.isnan(lp.token[0])).sum())
        assert emitted >= 8
        assert torch.equal(lp.top_ids[0, :emitted, 0], out[0, :emitted]), loop
        assert torch.equal(bits(lp.top[0, :emitted, 0].contiguous()), bits(lp.token[0, :emitted].contiguous())), loop
        assert (lp.top[0, :emitted, :-1] >= lp.top[0, :emitted, 1:]).all(), loop


@pytest.mark.parametrize("key", list(CONFIGS))
def test_the_loops_agree_on_the_logprobs_of_a_common_text(key):
    """Bound 2 tol / T: the project's near-tie bound on a 16-bit logit between passes (sampled_runs.TOL) can move the chosen
    logit and the log-sum-exp by tol each."""
    run, sampling, res = runs_of(key)
    T = sampling.temperature if sampling is not None else 1.0
    bound = 2 * sr.TOL[run["dtype"]] / T
    v_out, _, _, v_lp, _ = res["vanilla"][0]
    for loop, ((out, count, num, lp, events), _) in res.items():
        if loop == "vanilla":
            continue
        n = min(int((~torch.isnan(lp.token[0])).sum()), int((~torch.isnan(v_lp.token[0])).sum()))
        same = (out[0, :n] == v_out[0, :n]).long().cumprod(0).sum().item()
        assert same >= 8, f"{loop}: only {same} common tokens"
        err = (lp.token[0, :same].double() - v_lp.token[0, :same].double()).abs().max().item()
        print(f"{key} {loop}: {same} common tokens, largest log-prob difference {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (loop, err, bound)


def test_the_vanilla_cut_after_eos_is_applied_to_the_logprobs():
    run = get_run("qwen2_bf16", "qwen_bf16_g5")
    m = build(run)
    pl = torch.tensor([run["prompt_len"]])
    full, _, _ = m.vanilla_generate(run["prompt"], pl, max_gen_len=GEN, eos_id=None, logprobs=Logprobs(2))
    full, full_lp = full.clone(), m.last_logprobs
    text = full[0].tolist()
    eos = next(t for t in text[3:] if t != 0)
    stop = max(text.index(eos), 1)
    cut, _, _ = m.vanilla_generate(run["prompt"], pl, max_gen_len=GEN, eos_id=eos, logprobs=Logprobs(2))
    lp = m.last_logprobs
    assert cut[0, :stop + 1].tolist() == text[:stop + 1] and not cut[0, stop + 1:].any()
    assert torch.equal(bits(lp.token[:, :stop + 1].contiguous()), bits(full_lp.token[:, :stop + 1].contiguous()))
    assert torch.equal(lp.top_ids[:, :stop + 1], full_lp.top_ids[:, :stop + 1])
    assert torch.isnan(lp.token[:, stop + 1:]).all() and (lp.top_ids[:, stop + 1:] == -1).all()
    assert (lp.top[:, stop + 1:] == float("-inf")).all()


def test_refusals_and_validation():
    run = get_run("llama", "mixed")
    m = build(run)
    pl = torch.tensor([run["prompt_len"]])
    lp = Logprobs(2)
    real = m.model.forward
    m.model.forward = lambda *a, **k: (_ for _ in ()).throw(AssertionError("prefill before the refusal"))
    try:
        for call in (lambda: m.tree_spec_generate(run["prompt"], pl, tree_shape=run["tree_shape"], max_gen_len=16, temperature=0.5, logprobs=lp),
                     lambda: m.spec_generate(run["prompt"], pl, max_gen_len=16, temperature=0.5, logprobs=lp),
                     lambda: m.magicdec_generate(run["prompt"], pl, max_gen_len=16, temperature=0.5, logprobs=lp)):
            with pytest.raises(ValueError, match="temperature"):
                call()
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.tree_spec_generate(run["prompt"], pl, max_gen_len=16, shard=SimpleNamespace(vocab_parallel=True), logprobs=lp)
        with pytest.raises(TypeError):
            m.vanilla_generate(run["prompt"], pl, max_gen_len=16, logprobs=5)
    finally:
        m.model.forward = real
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    with pytest.raises(ValueError, match="temperature"):
        m.begin_tree_decode(first, lens, run["prompt_len"], temperature=0.5, logprobs=lp)
    with pytest.raises(ValueError, match="temperature"):
        m.begin_chain_decode(first, lens, lens, run["prompt_len"], temperature=0.5, logprobs=lp)
    m.model.layers[-1].self_attn.shard = SimpleNamespace(vocab_parallel=True)
    try:
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_tree_decode(first, lens, run["prompt_len"], logprobs=lp)
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_chain_decode(first, lens, lens, run["prompt_len"], logprobs=lp)
        with pytest.raises(ValueError, match="vocabulary-parallel"):
            m.begin_vanilla_decode(torch.zeros((1, 8), dtype=torch.int64), lens.clone(), lens, run["prompt_len"], logprobs=lp)
    finally:
        m.model.layers[-1].self_attn.shard = None
    assert Logprobs().top_n == 0 and Logprobs(20).top_n == 20 and Logprobs(5) == Logprobs(top_n=5) != Logprobs(4)
    for bad in (-1, 21, 1.5, True, "3", None):
        with pytest.raises(ValueError):
            Logprobs(bad)


def test_environment_default(monkeypatch):
    from longspec_amd.logprobs import LOGPROBS_ENV, env_logprobs
    monkeypatch.delenv(LOGPROBS_ENV, raising=False)
    assert env_logprobs() is None
    monkeypatch.setenv(LOGPROBS_ENV, "n=5")
    assert env_logprobs() == Logprobs(5) == Logprobs.parse(" n=5 ")
    for bad in ("5", "n", "n=abc", "k=3", "n=21", "n=-1", "n=1.5"):
        monkeypatch.setenv(LOGPROBS_ENV, bad)
        with pytest.raises(ValueError):
            env_logprobs()
    run = get_run("llama", "mixed")
    m = build(run)
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    monkeypatch.setenv(LOGPROBS_ENV, "n=2")
    st = m.begin_tree_decode(first, lens, run["prompt_len"], max_gen_len=32)
    assert st.logprobs.top_n == 2 and st.logprobs.top.shape == (1, 32, 2) and torch.isnan(st.logprobs.token).all()
    assert m.begin_tree_decode(first, lens, run["prompt_len"], temperature=0.5).logprobs is None
    assert m.begin_tree_decode(first, lens, run["prompt_len"], logprobs=Logprobs(4)).logprobs.top_n == 4      # the argument wins
    assert m.begin_chain_decode(first, lens, lens, run["prompt_len"], gamma=4, max_gen_len=32).logprobs.token.shape == (1, 36)
    out = torch.zeros((1, 8), dtype=torch.int64)
    assert m.begin_vanilla_decode(out, lens.clone(), lens, run["prompt_len"]).logprobs.top_ids.shape == (1, 8, 2)
    pl = torch.tensor([run["prompt_len"]])
    m.vanilla_generate(run["prompt"], pl, max_gen_len=12, eos_id=run["eos_id"])
    env_lp = m.last_logprobs
    monkeypatch.delenv(LOGPROBS_ENV)
    assert m.begin_tree_decode(first, lens, run["prompt_len"]).logprobs is None
    m.vanilla_generate(run["prompt"], pl, max_gen_len=12, eos_id=run["eos_id"], logprobs=Logprobs(2))
    assert torch.equal(bits(env_lp.token), bits(m.last_logprobs.token)) and torch.equal(env_lp.top_ids, m.last_logprobs.top_ids)
    m.vanilla_generate(run["prompt"], pl, max_gen_len=12, eos_id=run["eos_id"])
    assert m.last_logprobs is None
