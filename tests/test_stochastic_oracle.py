"""The word-stream oracle of ``ls_tree_verify_stochastic`` (tests/stochastic_oracle.py), checked without a GPU: it replays
Python's ``random`` word for word, it reproduces the reference's 24 golden walks, every case of the GPU case table meets
the margin condition that makes exact comparison legitimate, and the table tells every listed wrong walk from the right one."""
import random

import numpy as np
import pytest
import torch

import cases
import stochastic_oracle as so


def _next_words(n):
    """The next n raw Mersenne-Twister words of Python's generator, which is left where it was."""
    state = random.getstate()
    words = [random.getrandbits(32) for _ in range(n)]
    random.setstate(state)
    return words


def _advance(n):
    for _ in range(n):
        random.getrandbits(32)


@pytest.mark.parametrize("seed", [0, 1, 20240607])
def test_word_draws_replay_pythons_random(seed):
    """The claim of the kernel's header comment: random.choice(seq) is seq[getrandbits(k)] rejection-sampled, one word per
    attempt; random.random() is two words.  Same values, same number of words."""
    random.seed(seed)
    draws = so.WordDraws(_next_words(4000), None)
    order = random.Random(seed + 1)              # which call comes next: a generator of its own
    got, want = [], []
    for _ in range(600):
        n = order.choice([1, 2, 3, 5, 16, 17, 64])
        if order.random() < 0.6:
            got.append(draws.choice(range(n)))
            want.append(random.choice(range(n)))
        else:
            got.append(draws.random())
            want.append(random.random())
    assert got == want
    after = random.getstate()
    random.seed(seed)
    _advance(draws.used)
    assert random.getstate() == after


def test_word_draws_run_out():
    d = so.WordDraws([0xFFFFFFFF] * 3, None)     # getrandbits(2) = 3 >= 3: redrawn until the words end
    with pytest.raises(so.WordsExhausted):
        d.choice([7, 8, 9])
    assert d.used == 3
    d = so.WordDraws([0, 5], None)
    assert d.choice([7, 8, 9]) == 7
    with pytest.raises(so.WordsExhausted):       # random() needs two words
        d.random()


@pytest.mark.parametrize("c", list(cases.stochastic_cases()), ids=lambda c: c["name"])
def test_walk_reproduces_the_reference_goldens(c):
    random.seed(5000 + c["ci"])
    torch.manual_seed(6000 + c["ci"])
    state = random.getstate()
    words = _next_words(512)
    noise = torch.empty(c["logits"].shape[-1], dtype=c["logits"].dtype).exponential_(1)    # what torch.multinomial draws
    ids, num, used, margins = so.walk(c["spec"][0], c["mask"][0], c["logits"][0], c["spec_logp"][0], c["T"], words, noise)
    assert num == int(c["acc_num"][0])
    assert torch.equal(ids, c["acc_ids"][0])
    random.setstate(state)
    _advance(used)
    assert random.random() == c["after_random"]
    assert len(margins) >= 1 and margins[-1]["kind"] == "final"


@pytest.mark.parametrize("c", so.CASES, ids=lambda c: c["name"])
def test_case_meets_the_margin_condition(c):
    """Every acceptance decision |r - ratio| / ratio and the final draw's (top1 - top2) / top1 are at least
    4 * (n_res + 1) ulp of the activation type away from going the other way (stochastic_oracle.margin_bound)."""
    rows = so.expected(c)
    assert all(m["kind"] == "final" for r in rows for m in r[3][-1:])
    assert all(len(r[3]) >= 2 for r in rows), "a case whose walk takes no acceptance decision tests nothing"
    assert so.violations(c) == []


def test_case_table_covers_what_it_claims():
    by = so.BY_NAME
    # the forced cases walk as designed
    for n in (1, 2, 3, 5, 16, 17, 64):
        for name in (f"reject_all_{n}", f"reject_all_{n}_2"):
            (ids, num, used, margins), = so.expected(by[name])
            acc = [m for m in margins if m["kind"] == "accept"]
            assert num == 2 and len(acc) == n and [m["n_res"] for m in acc] == list(range(n)) and margins[-1]["n_res"] == n
            assert used >= 3 * n
    for n in (3, 5, 17):                          # a non-power-of-two child count redraws some word
        assert so.expected(by[f"reject_all_{n}"])[0][2] > 3 * n or so.expected(by[f"reject_all_{n}_2"])[0][2] > 3 * n
    (ids, num, used, margins), = so.expected(by["chain13"])
    assert num == 15 and torch.equal(ids[:14], so.build(by["chain13"])["spec"][0])
    (ids, num, used, margins), = so.expected(by["accept_all_2x5"])
    assert num == len(margins) + 1 and all(m["r"] <= m["ratio"] for m in margins[:-1])
    for name in ("tie_5_1029_3000", "tie_70_1029_2053_3000"):
        (ids, num, used, margins), = so.expected(by[name])
        assert margins[-1]["margin"] == 0.0 and int(ids[num - 1]) == min(by[name]["ties"])
    x = so.build(by["strided_f16"])
    assert x["logp"].shape[1] < x["spec"].shape[1] and not x["logits"].is_contiguous() and not x["logp"].is_contiguous()
    assert {c["V"] for c in so.CASES} >= {1023, 1024, 1025, 2047, 4099, 33001, 128256, 152064}


def _same(a, b):
    return a[1] == b[1] and a[2] == b[2] and torch.equal(a[0], b[0])


@pytest.mark.parametrize("name", list(so.MUTANTS))
def test_mutant_changes_some_case(name):
    """The case table has teeth: a kernel that implemented this wrong walk would return something else for a listed case."""
    for c in so.CASES:
        try:
            rows = so.expected(c, **so.MUTANTS[name])
        except (so.WordsExhausted, so.ZeroDistribution):
            return
        if not all(_same(a, b) for a, b in zip(rows, so.expected(c))):
            return
    raise AssertionError(f"no case of the table tells '{name}' from the right walk")


def test_zero_residual_raises_like_torch_multinomial():
    x = so.zero_residual_inputs()
    with pytest.raises(so.ZeroDistribution) as e:
        so.walk(x["spec"][0], x["mask"][0], x["logits"][0], x["logp"][0], x["T"], x["words"][0], x["noise"][0])
    assert len(e.value.margins) == 3 and all(m["ratio"] == 0.0 and m["r"] > 0 for m in e.value.margins)
    assert e.value.words_used >= 9
    with pytest.raises(RuntimeError):            # the reference's own draw on the row the walk leaves behind
        torch.multinomial(torch.zeros(x["logits"].shape[-1], dtype=torch.float16), num_samples=1)


def test_word_budget_is_exact():
    """With exactly the words the walk uses it completes; with one fewer it runs out."""
    c = so.BY_NAME["reject_all_3"]
    x = so.build(c)
    (ids, num, used, _), = so.expected(c)
    args = (x["spec"][0], x["mask"][0], x["logits"][0], x["logp"][0], x["T"])
    got = so.walk(*args, x["words"][0, :used], x["noise"][0])
    assert got[2] == used and torch.equal(got[0], ids)
    with pytest.raises(so.WordsExhausted):
        so.walk(*args, x["words"][0, :used - 1], x["noise"][0])
    assert np.asarray(x["words"]).dtype == np.uint32
