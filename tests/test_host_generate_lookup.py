"""Prompt-lookup speculation (``lookup_generate``) through the host loop on the CPU oracle (tests/lookup_oracle.py): the text is
the vanilla text for every parameter set and for ANY draft, the rounds really accept drafts, the glide layer is not used, the
loop composes with ``sampling=`` / ``penalties=`` / ``logprobs=`` / ``stop=``, and the keyword's checks."""
from types import SimpleNamespace

import pytest
import torch

import logprob_oracle
import lookup_oracle as lo
import sampled_runs as sr
import stop_oracle as so
import test_host_generate_logprobs as hl
import test_host_generate_penalized as hp
from longspec_amd import Logprobs, Sampling, Stop
from test_host_generate_sampled import FP16, build as _build, get_run

GEN = 64
RUNS = [("llama", "forced"), ("llama", "mixed"), ("llama", "rand"), ("qwen2_bf16", "qwen_bf16_g5")]
PARAMS = [(4, 3, 1), (7, 2, 1), (1, 1, 1), (15, 8, 2)]
G, MX, MN = 4, 3, 1                    # the parameters of the round-count tests
_models, _vanilla = {}, {}


def model_of(family, name):
    if (family, name) not in _models:
        run = get_run(family, name)
        _models[family, name] = (run, _build(run, ops=lo.ops))
    return _models[family, name]


def vanilla_text(family, name, gen=GEN, **kw):
    key = (family, name, gen, tuple(sorted(kw)))
    if key not in _vanilla or kw:
        run, m = model_of(family, name)
        out = m.vanilla_generate(run["prompt"], torch.tensor([run["prompt_len"]]), max_gen_len=gen, eos_id=run["eos_id"], **kw)[0]
        if kw:
            return out[0].tolist()
        _vanilla[key] = out[0].tolist()
        for eos in (run["eos_id"], getattr(run["cfg"], "eos_token_id", None)):
            assert eos not in _vanilla[key], "the runs were chosen so that no loop stops early"
    return _vanilla[key]


class Spy(hl.Spy):
    """``hl.Spy`` (the rows of ``token_logprobs``, the correct_len of ``chain_commit``) that also keeps what every
    ``ngram_draft`` call said it matched, and may replace the draft: ``override(call number, text, gamma) -> gamma ids``."""

    def __init__(self, base, override=None):
        super().__init__(base)
        self.matched, self.texts, self.override = [], [], override

    def ngram_draft(self, prompt_ids, input_len, output_ids, cache_lens, len_bound, gamma, max_ngram, min_ngram, spec_buffer,
                    info=None, hist=None):
        info = self._base.ngram_draft(prompt_ids, input_len, output_ids, cache_lens, len_bound, gamma, max_ngram, min_ngram,
                                      spec_buffer, info=info, hist=hist)
        text = lo.text_of(prompt_ids, input_len, output_ids, cache_lens, 0)
        assert len(text) <= len_bound
        if self.override is not None:
            spec_buffer[0, 1:] = torch.tensor(self.override(len(self.matched), text, gamma), dtype=torch.int64)
        self.matched.append(int(info[0, 0]))
        self.texts.append(text)
        return info


def lookup(family, name, g=G, mx=MX, mn=MN, gen=GEN, override=None, m=None, **kw):
    """One ``lookup_generate`` under the spy: out (a list), n text columns, the rounds' accepted counts and matched lengths."""
    run, m0 = model_of(family, name)
    m = m or m0
    spy = Spy(lo.ops, override)
    saved, m.ops = m.ops, spy
    try:
        out, count, num, elapsed, mask = m.lookup_generate(run["prompt"], torch.tensor([run["prompt_len"]]), gamma=g, max_ngram=mx,
                                                           min_ngram=mn, max_gen_len=gen, eos_id=run["eos_id"], **kw)
    finally:
        m.ops = saved
    rounds = [int(e[1][0]) for e in spy.events if e[0] == "chain"]
    assert (int(count), int(num)) == (sum(rounds) - len(rounds), len(rounds)) and out.shape == (1, gen + g) == mask.shape
    ls = m.last_stop
    return SimpleNamespace(out=out[0].tolist(), n=1 + sum(rounds), rounds=rounds, matched=spy.matched, texts=spy.texts,
                           hist=m.last_lookup.hist.clone(), events=spy.events, lp=m.last_logprobs, m=m,
                           stop=None if ls is None else (int(ls.length[0]), int(ls.which[0]), int(ls.match_start[0])))


def assert_is_vanilla(got, text, what):
    n = min(got.n, len(text))
    assert n >= len(text) - 16, (what, n)                              # the loop ran to the end of its buffer
    assert got.out[:n] == text[:n], f"{what}: parts from the vanilla text"


@pytest.mark.parametrize("family,name", RUNS)
@pytest.mark.parametrize("g,mx,mn", PARAMS)
def test_the_lookup_text_is_the_vanilla_text(family, name, g, mx, mn):
    got = lookup(family, name, g, mx, mn)
    assert_is_vanilla(got, vanilla_text(family, name), (name, g, mx, mn))
    # every round drafted what the oracle drafts from the text as it stood, and the histogram is the oracle's
    hist = [0] * (mx + 1)
    for text, n in zip(got.texts, got.matched):
        assert lo.match(text, mx, mn)[0] == n
        hist[n] += 1
    assert got.hist.tolist() == [hist] and sum(hist) == len(got.rounds)
    text = got.out[:got.n]                                             # the texts the drafter saw are prefixes of the result
    run = get_run(family, name)
    prompt = run["prompt"][0, :run["prompt_len"]].tolist()
    w = 1
    for seen, acc in zip(got.texts, got.rounds):
        assert seen == prompt + text[:w]
        w += acc


def test_rounds_of_the_forced_run_accept_whole_drafts():
    got = lookup("llama", "forced")
    full = sum(a == G + 1 for a in got.rounds)
    print(f"forced: {len(got.rounds)} rounds, {full} full, {got.matched.count(0)} without a match")
    assert full >= 10 and got.matched.count(0) >= 1


def test_rounds_of_the_mixed_run_accept_all_part_and_nothing():
    got = lookup("llama", "mixed")
    full = sum(a == G + 1 for a in got.rounds)
    part = sum(2 <= a <= G for a in got.rounds)
    print(f"mixed: {len(got.rounds)} rounds, {full} full, {part} partial, {got.matched.count(0)} without a match")
    assert full >= 5 and part >= 1 and got.matched.count(0) >= 10


@pytest.mark.parametrize("family,name", [("llama", "mixed"), ("qwen2_bf16", "qwen_bf16_g5")])
def test_the_loop_is_lossless_for_any_draft(family, name):
    text = vanilla_text(family, name)
    run = get_run(family, name)
    P = run["prompt_len"]
    V = run["cfg"].vocab_size
    gen = torch.Generator().manual_seed(5)

    def truth(i, seen, gamma):
        w = len(seen) - P
        return (text[w:w + gamma] + [0] * gamma)[:gamma]

    def noise(i, seen, gamma):
        w = len(seen) - P
        d = torch.randint(0, V, (gamma,), generator=gen).tolist()
        d[0] = (text[w] + 1) % V if w < len(text) else d[0]            # never the true next token
        return d

    a = lookup(family, name, override=truth)
    assert_is_vanilla(a, text, "true drafts")
    assert all(acc == G + 1 for acc in a.rounds[:-1]) and len(a.rounds) >= 12
    b = lookup(family, name, override=noise)
    assert_is_vanilla(b, text, "random drafts")
    assert all(acc == 1 for acc in b.rounds) and len(b.rounds) == GEN - 1
    c = lookup(family, name, override=lambda i, seen, gamma: (truth if i % 2 == 0 else noise)(i, seen, gamma))
    assert_is_vanilla(c, text, "alternating drafts")
    assert set(c.rounds[:-1]) == {1, G + 1}


def test_the_glide_layer_is_not_used():
    run = get_run("llama", "mixed")
    m = _build(run, ops=lo.ops)
    with torch.no_grad():
        for p in m.glide.parameters():
            p.fill_(float("nan"))
    called = []
    m.glide.register_forward_pre_hook(lambda *a: called.append(1))
    got = lookup("llama", "mixed", m=m)
    assert not called and got.out == lookup("llama", "mixed").out
    assert_is_vanilla(got, vanilla_text("llama", "mixed"), "NaN glide")


@pytest.mark.parametrize("name,seed", FP16["pairs"][:2])
def test_sampling_gives_the_sampled_vanilla_text(name, seed):
    s = Sampling(FP16["temperature"], FP16["top_k"], FP16["top_p"], seed)
    text = vanilla_text("llama", name, sampling=s)
    got = lookup("llama", name, sampling=s)
    assert_is_vanilla(got, text, ("sampled", name, seed))
    assert text != vanilla_text("llama", name)


def test_penalties_give_the_penalised_vanilla_text():
    kind, (name, kw) = "fp16", hp.PAIRS["fp16"]["pairs"][0]
    run, m = model_of("llama", name)
    run, m, pen, gen, text = hp.checked_vanilla(kind, name, kw, m=m)   # (asserts the pair's near-tie margin)
    got = lookup("llama", name, gen=gen, penalties=pen)
    assert got.n >= gen - G - 1 and got.out[:min(got.n, gen)] == text.tolist()[:min(got.n, gen)]
    assert text.tolist() != vanilla_text("llama", name, gen=gen)[:gen], "the penalty does not bite"


@pytest.mark.parametrize("family,name", [("llama", "mixed"), ("qwen2_bf16", "qwen_bf16_g5")])
def test_logprobs_hold_the_accepted_rows_values(family, name):
    """The comparison tests/test_host_generate_logprobs.py applies to the chain loop: every emitted column holds the bits of
    the verification row that produced it, the rest the fill; and the values agree with the vanilla loop's within 2 tol."""
    top_n = 3
    got = lookup(family, name, logprobs=Logprobs(top_n))
    plain = lookup(family, name)
    assert got.out == plain.out and plain.lp is None and not [e for e in plain.events if e[0] == "rows"]
    want, emitted = hl.expected_buffers("chain", got.events, GEN + G, top_n)
    assert emitted == got.n
    for f in ("token", "top", "top_ids"):
        assert torch.equal(hl.bits(getattr(got.lp, f)), hl.bits(getattr(want, f))), f
    assert not torch.isnan(got.lp.token[0, :emitted]).any() and torch.isnan(got.lp.token[0, emitted:]).all()
    assert torch.equal(got.lp.top_ids[0, :emitted, 0], torch.tensor(got.out[:emitted]))
    run, m = model_of(family, name)
    m.vanilla_generate(run["prompt"], torch.tensor([run["prompt_len"]]), max_gen_len=GEN, eos_id=run["eos_id"], logprobs=Logprobs(top_n))
    v_lp = m.last_logprobs
    n = min(emitted, GEN)
    err = (got.lp.token[0, :n].double() - v_lp.token[0, :n].double()).abs().max().item()
    bound = 2 * sr.TOL[run["dtype"]]
    print(f"{name}: {n} common tokens, largest log-prob difference {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_stop_cuts_the_loops_own_plain_text():
    plain = lookup("llama", "mixed", logprobs=Logprobs(2))
    text = plain.out[:plain.n]
    starts, c = [], 1
    for acc in plain.rounds:
        starts.append((c, acc))
        c += acc
    stops = {"column-0": Stop(token_ids=[text[0]])}
    # a stop that ends strictly inside a round: wide rounds repeat earlier text, so it takes a sequence long enough to be new
    for j, k in ((j, k) for c, acc in starts for j in range(c, c + acc - 1) for k in range(1, 17)):
        seq = text[max(j - k + 1, 0):j + 1]
        if "inside" not in stops and so.scan(text, Stop(sequences=[seq]))[0] == j + 1:
            stops["inside"] = Stop(sequences=[seq])
    assert set(stops) == {"column-0", "inside"}
    for what, stop in stops.items():
        got = lookup("llama", "mixed", logprobs=Logprobs(2), stop=stop)
        want, triple = so.cut(plain.out, plain.n, stop, 0)
        assert triple[0] > 0 and got.stop == triple, what
        assert got.out[:plain.n] == want[:plain.n] and got.out[triple[0]:] == [0] * (len(got.out) - triple[0]), what
        assert torch.isnan(got.lp.token[0, triple[0]:]).all(), what
        assert torch.equal(hl.bits(got.lp.token[0, :triple[0]].contiguous()), hl.bits(plain.lp.token[0, :triple[0]].contiguous()))
        assert len(got.rounds) == (1 if what == "column-0" else len([s for s in starts if s[0] < triple[0]])), what
    st_rounds = []
    run, m = model_of("llama", "mixed")
    orig = m.begin_lookup_decode
    m.begin_lookup_decode = lambda *a, **k: st_rounds.append(orig(*a, **k)) or st_rounds[-1]
    try:
        lookup("llama", "mixed", stop=stops["inside"])
    finally:
        del m.begin_lookup_decode
    assert st_rounds[0].stopped and m.lookup_round(st_rounds[0]) is False   # a stopped state is final


def test_bad_parameters_are_refused_before_the_model_is_touched():
    run, m = model_of("llama", "mixed")
    pl = torch.tensor([run["prompt_len"]])
    real = m.model.forward
    m.model.forward = lambda *a, **k: (_ for _ in ()).throw(AssertionError("prefill before the refusal"))
    try:
        for bad in (dict(gamma=0), dict(gamma=16), dict(max_ngram=0), dict(max_ngram=9), dict(max_ngram=2, min_ngram=3),
                    dict(min_ngram=0), dict(gamma=2.0)):
            with pytest.raises(ValueError, match="lookup"):
                m.lookup_generate(run["prompt"], pl, max_gen_len=16, **bad)
            with pytest.raises(ValueError, match="lookup"):
                m.begin_lookup_decode(torch.tensor([3]), torch.tensor([8], dtype=torch.int32), pl, 8, run["prompt"], **bad)
        with pytest.raises(TypeError):
            m.lookup_generate(run["prompt"], pl, max_gen_len=16, temperature=0.5)
    finally:
        m.model.forward = real


def test_the_oracle_namespace_is_layered_on_the_stop_oracle():
    assert lo.ops.stop_scan is so.ops.stop_scan and lo.ops.token_logprobs is logprob_oracle.ops.token_logprobs
    assert not hasattr(so.ops, "ngram_draft")
