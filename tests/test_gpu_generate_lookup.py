"""``lookup_generate`` end to end on the HIP kernels: the toy runs of tests/test_host_generate_lookup.py on the device.  The
expectation is the DEVICE's own vanilla text, recorded launch by launch under a spy that keeps the arg-max rows -- exact where
the run keeps the near-tie bound, else explained by it --, and the rounds replayed from HIP graphs give the bits of the
launch-by-launch rounds."""
from types import SimpleNamespace

import pytest
import torch

import sampled_runs as sr
import stop_oracle as so
import test_host_generate_logprobs as hl
import test_host_generate_penalized as hp
from longspec_amd import Logprobs, Penalties, Sampling, Stop
from test_host_generate_sampled import FP16, build as _build, get_run

pytestmark = pytest.mark.gpu
GEN, G, MX, MN = 64, 4, 3, 1
_models, _vanilla = {}, {}


def model_of(family, name):
    if (family, name) not in _models:
        run = get_run(family, name)
        m = _build(run, device="cuda")
        m.GRAPH_AFTER = 0
        _models[family, name] = (run, m)
    return _models[family, name]


class Spy:
    """The device's operator module with the arg-max rows, the rounds' accepted counts and the matched lengths kept (one host
    read per call: for launch-by-launch runs only)."""

    def __init__(self):
        from longspec_amd import ops
        self._base, self.rows, self.rounds, self.matched = ops, [], [], []

    def __getattr__(self, name):
        return getattr(self._base, name)

    def argmax_rows(self, logits):
        self.rows.append(logits.reshape(-1, logits.shape[-1]).float().cpu())
        return self._base.argmax_rows(logits)

    def chain_commit(self, *a, **k):
        state = self._base.chain_commit(*a, **k)
        self.rounds.append(int(state[0, 0]))
        return state

    def ngram_draft(self, *a, **k):
        info = self._base.ngram_draft(*a, **k)
        self.matched.append(int(info[0, 0]))
        return info


def vanilla(family, name, gen=GEN):
    """(text, the arg-max row of every column >= 1) of the device's launch-by-launch vanilla run."""
    if (family, name, gen) not in _vanilla:
        run, m = model_of(family, name)
        spy = Spy()
        m.ops, m.GRAPH_ROUNDS = spy, False
        try:
            out = m.vanilla_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"), max_gen_len=gen,
                                     eos_id=run["eos_id"])[0][0].tolist()
        finally:
            m.ops, m.GRAPH_ROUNDS = spy._base, True
        rows = torch.cat(spy.rows)
        assert rows.shape[0] == gen - 1 and rows.argmax(dim=-1).tolist() == out[1:]
        for eos in (run["eos_id"], getattr(run["cfg"], "eos_token_id", None)):
            assert eos not in out, "the runs were chosen so that no loop stops early"
        _vanilla[family, name, gen] = (out, rows)
    return _vanilla[family, name, gen]


def lookup(family, name, graphs, spy=False, gen=GEN, m=None, **kw):
    run, m0 = model_of(family, name)
    m = m or m0
    states = []
    orig = m.begin_lookup_decode
    m.begin_lookup_decode = lambda *a, **k: states.append(orig(*a, **k)) or states[-1]
    s = Spy() if spy else None
    if s is not None:
        assert not graphs
        m.ops = s
    m.GRAPH_ROUNDS = graphs
    try:
        out, count, num, _, _ = m.lookup_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"), gamma=G,
                                                  max_ngram=MX, min_ngram=MN, max_gen_len=gen, eos_id=run["eos_id"], **kw)
    finally:
        del m.begin_lookup_decode
        m.GRAPH_ROUNDS = True
        if s is not None:
            m.ops = s._base
    st, ls, lp = states[0], m.last_stop, m.last_logprobs
    assert (st.replayer.captures > 0 and not st.replayer.disabled) == bool(graphs), "replayed / eager as asked"
    return SimpleNamespace(out=out[0].tolist(), n=1 + int(count) + int(num), num=int(num), st=st, hist=m.last_lookup.hist.cpu().tolist(),
                           rounds=s.rounds if s else None, matched=s.matched if s else None,
                           stop=None if ls is None else (int(ls.length[0]), int(ls.which[0]), int(ls.match_start[0])),
                           lp=None if lp is None else [t.clone().cpu() for t in (lp.token, lp.top, lp.top_ids)])


def same_bits(a, b, what):
    assert a.out == b.out and a.stop == b.stop and a.hist == b.hist and a.n == b.n, what
    assert (a.lp is None) == (b.lp is None)
    for x, y in zip(a.lp or (), b.lp or ()):
        assert torch.equal(hl.bits(x), hl.bits(y)), what


def margin(rows):
    best = rows.topk(2, dim=-1).values
    return float((best[:, 0] - best[:, 1]).min())


def test_forced_is_the_devices_vanilla_text_and_accepts_whole_drafts():
    run, m = model_of("llama", "forced")
    text, rows = vanilla("llama", "forced")
    tol = sr.TOL[run["dtype"]]
    print(f"forced: smallest top-2 margin of the device's vanilla run {margin(rows):.4f}, bound {tol}")
    assert margin(rows) >= tol, "choose another run: a row of the device's vanilla run is a near-tie"
    eager = lookup("llama", "forced", graphs=False, spy=True)
    n = min(eager.n, GEN)
    assert n >= GEN - G - 1 and eager.out[:n] == text[:n]
    full = sum(a == G + 1 for a in eager.rounds)
    print(f"forced: {len(eager.rounds)} rounds, {full} full, {eager.matched.count(0)} without a match")
    assert full >= 10 and eager.matched.count(0) >= 1
    assert sum(eager.hist[0]) == len(eager.rounds) and eager.hist[0][0] == eager.matched.count(0)
    replayed = lookup("llama", "forced", graphs=True)
    same_bits(replayed, lookup("llama", "forced", graphs=False), "forced")
    assert replayed.out == eager.out


@pytest.mark.parametrize("family,name", [("llama", "mixed"), ("qwen2_bf16", "qwen_bf16_g5")])
def test_the_text_is_the_devices_vanilla_text_up_to_an_explained_near_tie(family, name):
    run, m = model_of(family, name)
    text, rows = vanilla(family, name)
    tol = sr.TOL[run["dtype"]]
    eager = lookup(family, name, graphs=False, spy=True)
    n = min(eager.n, GEN)
    diff = [c for c in range(n) if eager.out[c] != text[c]]
    upto = diff[0] if diff else n
    if diff:
        c = diff[0]
        assert c >= 1, "the first token comes from the same prefill"
        best = rows[c - 1].topk(2)
        print(f"{name}: parts at column {c}: took {eager.out[c]}, vanilla {text[c]}, gap {float(best.values[0] - best.values[1]):.4f}")
        assert eager.out[c] == int(best.indices[1]) and float(best.values[0] - best.values[1]) < tol
    starts, c = [], 1
    for acc in eager.rounds:
        starts.append((c, acc))
        c += acc
    assert any(acc >= 2 and c0 + acc <= upto for c0, acc in starts), "no round in front of that column accepted a draft token"
    replayed = lookup(family, name, graphs=True, logprobs=Logprobs(2))
    same_bits(replayed, lookup(family, name, graphs=False, logprobs=Logprobs(2)), name)
    assert replayed.out == eager.out


def test_a_generation_that_outgrows_its_tier_captures_the_next():
    run, m = model_of("llama", "forced")
    text, rows = vanilla("llama", "forced", gen=96)
    assert margin(rows) >= sr.TOL[run["dtype"]], "choose another run: a row of the device's vanilla run is a near-tie"
    m.GRAPH_TIER = 32
    try:
        got = lookup("llama", "forced", graphs=True, gen=96)
    finally:
        del m.GRAPH_TIER
    assert got.st.graph_tiers >= 2 and got.st.graph_captures >= 2
    n = min(got.n, 96)
    assert n >= 96 - G - 1 and got.out[:n] == text[:n]


def test_sampling_penalties_and_stop_replay_the_bits_of_the_eager_rounds():
    name, seed = FP16["pairs"][0]
    assert name == "forced"
    s = Sampling(FP16["temperature"], FP16["top_k"], FP16["top_p"], seed)
    a = lookup("llama", name, graphs=True, sampling=s, logprobs=Logprobs(2))
    same_bits(a, lookup("llama", name, graphs=False, sampling=s, logprobs=Logprobs(2)), "sampled")
    assert a.out != lookup("llama", name, graphs=False).out
    pen = Penalties(**hp.QWQ)
    b = lookup("llama", "mixed", graphs=True, penalties=pen, logprobs=Logprobs(2))
    same_bits(b, lookup("llama", "mixed", graphs=False, penalties=pen, logprobs=Logprobs(2)), "penalised")
    plain = lookup("llama", "mixed", graphs=False, spy=True)
    assert b.out != plain.out, "the penalty does not bite"
    # stop=: the oracle's cut of the device's own plain lookup text, inside a round that accepted drafts
    text = plain.out[:plain.n]
    starts, c = [], 1
    for acc in plain.rounds:
        starts.append((c, acc))
        c += acc
    stop = None
    for j, k in ((j, k) for c0, acc in starts for j in range(c0, c0 + acc - 1) for k in range(1, 17)):
        seq = text[max(j - k + 1, 0):j + 1]
        if stop is None and so.scan(text, Stop(sequences=[seq]))[0] == j + 1:
            stop = Stop(sequences=[seq])
    assert stop is not None, "no stop ends strictly inside a round"
    want, triple = so.cut(plain.out, plain.n, stop, 0)
    for graphs in (True, False):
        got = lookup("llama", "mixed", graphs=graphs, stop=stop)
        assert got.stop == triple and got.out[:plain.n] == want[:plain.n] and not any(got.out[triple[0]:]), graphs
        assert got.st.stopped


def test_nan_glide_weights_change_nothing():
    run = get_run("llama", "mixed")
    m = _build(run, device="cuda")
    m.GRAPH_AFTER = 0
    with torch.no_grad():
        for p in m.glide.parameters():
            p.fill_(float("nan"))
    assert lookup("llama", "mixed", graphs=True, m=m).out == lookup("llama", "mixed", graphs=True).out
