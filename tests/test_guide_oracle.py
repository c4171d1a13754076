"""``longspec_amd.Guide`` and its oracle (tests/guide_oracle.py) without a GPU: the oracle against a brute-force simulation of
the language as a set of strings, the constructor's checks, the table's layout word for word, the dead-end check, ``choice``,
``from_byte_dfa``, ``save`` / ``load`` / ``LONGSPEC_GUIDE`` and ``resolve``."""
import itertools
import time

import numpy as np
import pytest
import torch

import guide_oracle as go
from longspec_amd import Guide
from longspec_amd import guide as guide_mod


def language(g, vocab, n):
    """Every string of length <= n over [0, vocab) the guide accepts as a text (every prefix live), by enumeration."""
    out = set()
    for k in range(n + 1):
        for s in itertools.product(range(vocab), repeat=k):
            st, ok = g.start, True
            for t in s:
                c = int(g.token_class[t]) if t < g.token_class.size else -1
                st = int(g.next[st, c]) if c >= 0 else -1
                if st < 0:
                    ok = False
                    break
            if ok:
                out.add(s)
    return out


SMALL = [Guide([[1, -1], [-1, 0]]),                                                   # 0 1 0 1 ...
         Guide([[1, 2, -1], [1, -1, 2], [2, 2, 2]], token_class=[0, 1, 2, 1, -1]),     # classes shared, id 4 forbidden
         Guide([[0, 1], [1, 0]], token_class=[1, 0, 1], start=1)]                     # ids 3, 4 beyond token_class


@pytest.mark.parametrize("g", SMALL, ids=lambda g: repr(g))
def test_the_oracle_is_the_language(g):
    V, n = 5, 4
    table = g.table(V, "cpu")
    p = go.parse(table)
    lang = language(g, V, n)
    assert len(lang) > 3
    for s in itertools.product(range(V), repeat=n - 1):
        for k in range(n):
            text = s[:k]
            st = go.walk(p, p.start, text)
            assert st == g.walk(text, vocab=V)
            assert (st >= 0) == (text in lang), text
            if st >= 0:
                ok = go.allowed(p, st, V)
                assert [v for v in range(V) if ok[v]] == [v for v in range(V) if text + (v,) in lang], text
    # the operators: rows that follow 0, 1, 2 extras, live and dead, and the advance
    x = torch.arange(3 * V, dtype=torch.float32).view(1, 3, V).to(torch.float16)
    ids = torch.tensor([[1, 0]])
    mask = torch.tensor([[0, 0], [1, 0], [1, 1]])
    state = torch.tensor([g.start], dtype=torch.int32)
    got = go.guide_rows(x, table, state, ids, mask)
    for r, text in enumerate([(), (1,), (1, 0)]):
        if text in lang:
            want = [float(x[0, r, v]) if text + (v,) in lang else float("-inf") for v in range(V)]
        else:
            want = x[0, r].tolist()
        assert got[0, r].tolist() == want, text
    go.guide_advance(state, table, torch.tensor([[1, 0, 3]]), num=torch.tensor([2]))
    assert int(state[0]) == g.walk((1, 0))
    dead = torch.tensor([-1], dtype=torch.int32)
    go.guide_advance(dead, table, torch.tensor([[0]]))
    assert int(dead[0]) == -1 and torch.equal(go.guide_rows(x, table, dead), x)


def test_constructor_checks():
    with pytest.raises(TypeError, match="Guide: next must be an integer array"):
        Guide([[0.5]])
    with pytest.raises(TypeError, match="Guide: next must be an integer array"):
        Guide([[True]])
    with pytest.raises(ValueError, match="Guide: next must have 2 dimensions"):
        Guide([0, 1])
    with pytest.raises(ValueError, match="at least one state"):
        Guide(np.zeros((0, 3), dtype=np.int64))
    with pytest.raises(ValueError, match=f"1..{guide_mod.MAX_CLASSES} classes"):
        Guide(np.zeros((1, 0), dtype=np.int64))
    with pytest.raises(ValueError, match=f"1..{guide_mod.MAX_CLASSES} classes"):
        Guide(np.zeros((1, guide_mod.MAX_CLASSES + 1), dtype=np.int64))
    with pytest.raises(ValueError, match=f"at most {guide_mod.MAX_CELLS} entries"):
        Guide(np.zeros((1025, 16384), dtype=np.int8))
    Guide(np.zeros((1024, 16384), dtype=np.int8))                              # the limits themselves are legal
    with pytest.raises(ValueError, match="entries of next are -1"):
        Guide([[2, 0], [0, 0]])
    with pytest.raises(ValueError, match="entries of next are -1"):
        Guide([[-2]])
    with pytest.raises(TypeError, match="token_class must be an integer array"):
        Guide([[0]], token_class=[0.0])
    with pytest.raises(ValueError, match="token_class must have 1 dimension"):
        Guide([[0]], token_class=[[0]])
    with pytest.raises(ValueError, match="entries of token_class are -1"):
        Guide([[0]], token_class=[0, 1])
    with pytest.raises(ValueError, match="entries of token_class are -1"):
        Guide([[0]], token_class=[-2])
    with pytest.raises(TypeError, match="start must be an integer"):
        Guide([[0]], start=0.0)
    with pytest.raises(TypeError, match="start must be an integer"):
        Guide([[0]], start=True)
    with pytest.raises(ValueError, match="start must be a state 0..0"):
        Guide([[0]], start=1)
    assert (guide_mod.MAX_CLASSES, guide_mod.MAX_CELLS, guide_mod.HEADER_WORDS, guide_mod.NO_CLASS) == (16384, 1 << 24, 8, 0xFFFF)
    a, b = Guide([[0, -1]], [0, 1, -1]), Guide(torch.tensor([[0, -1]]), np.array([0, 1, -1], dtype=np.int32))
    assert a == b and hash(a) == hash(b) and a != Guide([[0, -1]], [0, 1]) and a != Guide([[0, 0]], [0, 1, -1])
    assert a != "x" and "states=1" in repr(a) and "classes=2" in repr(a)
    assert Guide([[0, 0, 0]]).token_class.tolist() == [0, 1, 2]                # None: the identity
    with pytest.raises(ValueError):
        a.next[0, 0] = 5                                                       # the arrays are frozen: the hash stays valid


@pytest.mark.parametrize("vocab", [5, 6, 7, 8, 9, 16, 17])
def test_the_table_layout_word_for_word(vocab):
    g = Guide([[1, -1, 0], [0, 1, -1]], token_class=[2, 0, -1, 1, 0, 1], start=1)
    t = g.table(vocab, "cpu")
    assert t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous()
    w = t.tolist()
    K = (((vocab + 1) // 2) + 3) // 4 * 4
    assert w[:8] == [2, 3, 1, vocab, 8 + K + 6, 0, 0, 0] and len(w) == 8 + K + 6
    cls = [2, 0, 0xFFFF, 1, 0, 1][:vocab] + [0xFFFF] * (2 * K - min(vocab, 6))    # ids beyond token_class and the padding
    for i in range(K):
        assert w[8 + i] & 0xFFFFFFFF == cls[2 * i] | (cls[2 * i + 1] << 16), i      # the even id in the low half
    assert (8 + K) % 4 == 0                                                       # the transition area: 16-byte aligned
    assert w[8 + K:] == [1, -1, 0, 0, 1, -1]
    assert guide_mod.class_words(vocab) == K
    p = go.parse(t)
    assert (p.S, p.C, p.start, p.vocab) == (2, 3, 1, vocab) and p.cls.tolist() == ([2, 0, -1, 1, 0, 1] + [-1] * 16)[:vocab]
    for bad in (0, -1, 2 ** 30, 1.5, True):
        with pytest.raises(ValueError, match="vocab"):
            g.table(bad, "cpu")


def test_the_dead_end_check():
    # state 2 allows nothing; it is reachable through class 1 of state 1
    nx = [[1, -1], [-1, 2], [-1, -1], [-1, -1]]
    with pytest.raises(ValueError, match="state 2 is reachable"):
        Guide(nx).table(2, "cpu")
    Guide([[1, -1], [0, -1], [-1, -1], [-1, -1]]).table(2, "cpu")              # states 2 and 3 are unreachable
    # reachable only through a class no token below vocab has: not reachable
    Guide([[0, 2], [-1, -1], [-1, -1]], token_class=[0, 0, 1]).table(2, "cpu")
    with pytest.raises(ValueError, match="state 2 is reachable"):
        Guide([[0, 2], [-1, -1], [-1, -1]], token_class=[0, 0, 1]).table(3, "cpu")
    with pytest.raises(ValueError, match="state 1 is reachable"):              # ... and state 1 then allows nothing below vocab
        Guide([[1, -1], [-1, 0]], token_class=[0, 0, 1]).table(2, "cpu")
    with pytest.raises(ValueError, match="state 0 is reachable"):
        Guide([[-1]]).table(4, "cpu")
    with pytest.raises(ValueError, match="state 0 is reachable"):
        Guide([[0]], token_class=[-1, -1, 0]).table(2, "cpu")


def test_choice():
    eos = 9
    seqs = [[3, 4, 5], [3, 4], [7], [3, 6, 6]]
    g = Guide.choice(seqs, eos)
    assert g.classes == len({3, 4, 5, 6, 7, 9}) and g.start == 0 and g.token_class.size == 10
    V, n = 10, 5
    lang = language(g, V, n)
    complete = {s for s in lang if len(s) >= 2 and s[-1] == eos and s[-2] != eos}
    assert complete == {tuple(s) + (eos,) for s in seqs}
    for s in lang:                                                            # a text is a prefix of a choice + eos + eos ...
        assert any(s == (tuple(c) + (eos,) * n)[:len(s)] for c in seqs), s
    g.table(V, "cpu")                                                         # no reachable dead end
    with pytest.raises(ValueError, match="no sequences"):
        Guide.choice([], eos)
    with pytest.raises(ValueError, match="at least one token"):
        Guide.choice([[]], eos)
    with pytest.raises(TypeError, match="not an integer token id"):
        Guide.choice([[1.5]], eos)
    with pytest.raises(ValueError, match="not a token id"):
        Guide.choice([[-1]], eos)
    with pytest.raises(TypeError, match="token id lists"):
        Guide.choice("ab", eos)
    with pytest.raises(ValueError, match="eos_id"):
        Guide.choice([[1]], -1)


def digits_dfa():
    """[+-]?[0-9]+ : state 0 start, 1 behind a sign, 2 behind a digit."""
    bn = np.full((3, 256), -1, dtype=np.int64)
    bn[0, ord("+")] = bn[0, ord("-")] = 1
    for s in range(3):
        bn[s, ord("0"):ord("9") + 1] = 2
    return bn


def test_from_byte_dfa():
    bn = digits_dfa()
    rng = np.random.default_rng(7)
    alphabet = np.frombuffer(b"0123456789+-ab", dtype=np.uint8)
    toks = [b""] + [bytes(rng.choice(alphabet, size=int(rng.integers(1, 7)), p=[0.085] * 10 + [0.05, 0.05, 0.025, 0.025]))
                    for _ in range(1999)]
    toks[5], toks[6], toks[7], toks[8], toks[9] = b"+", b"-12", b"007", b"+x", b"-"
    g = Guide.from_byte_dfa(bn, toks)
    assert g.states == 3 and g.token_class.size == 2000

    def run(s, t):
        for byte in t:
            if s < 0:
                break
            s = int(bn[s, byte])
        return s

    for i, t in enumerate(toks):
        vec = [run(s, t) if t else -1 for s in range(3)]
        c = int(g.token_class[i])
        if all(v < 0 for v in vec):
            assert c == -1, (i, t)
        else:
            assert c >= 0 and g.next[:, c].tolist() == vec, (i, t)
    # behaviours: a sign alone (0 -> 1), sign + digits (0 -> 2), digits (every state -> 2); everything else is dead everywhere
    assert g.classes == 3 and g.token_class[0] == -1 and g.token_class[8] == -1
    assert len({int(g.token_class[i]) for i in (5, 6, 7)}) == 3 and g.token_class[5] == g.token_class[toks.index(b"-")]
    assert sorted(map(tuple, g.next.T.tolist())) == sorted([(1, -1, -1), (2, -1, -1), (2, 2, 2)])
    assert int((g.token_class >= 0).sum()) == sum(1 for t in toks if t and any(run(s, t) >= 0 for s in range(3)))
    g.table(2000, "cpu")
    with pytest.raises(ValueError, match=r"\[S, 256\]"):
        Guide.from_byte_dfa(bn[:, :255], toks)
    with pytest.raises(TypeError, match="bytes"):
        Guide.from_byte_dfa(bn, ["ab"])
    # more behaviours than classes: under a random 32-state DFA nearly every two-byte token is its own behaviour
    rnd = rng.integers(0, 32, size=(32, 256))
    with pytest.raises(ValueError, match="distinct behaviours"):
        Guide.from_byte_dfa(rnd, [bytes((i >> 8, i & 255)) for i in range(65536)])


def test_from_byte_dfa_takes_seconds_at_128k_tokens_and_100_states():
    rng = np.random.default_rng(3)
    bn = rng.integers(-1, 100, size=(100, 256))
    lens = rng.integers(1, 12, size=128 * 1024)
    blob = rng.integers(97, 101, size=int(lens.sum()), dtype=np.uint8).tobytes()       # four letters: many shared behaviours
    offs = np.concatenate(([0], np.cumsum(lens)))
    toks = [blob[offs[i]:offs[i + 1]] for i in range(lens.size)]
    t0 = time.time()
    try:
        g = Guide.from_byte_dfa(bn, toks)
    except ValueError as e:
        assert "distinct behaviours" in str(e)
        g = None
    took = time.time() - t0
    print(f"from_byte_dfa, 128k tokens x 100 states: {took:.2f} s")
    assert took < 30, "seconds, not minutes"
    if g is not None:
        for i in (0, 1, 77, 131071):
            s = 5
            for byte in toks[i]:
                s = int(bn[s, byte]) if s >= 0 else -1
            c = int(g.token_class[i])
            assert (int(g.next[5, c]) if c >= 0 else -1) == s


def test_save_load_and_the_environment_default(tmp_path, monkeypatch):
    g = Guide([[1, -1, 0], [0, 1, -1]], token_class=[2, 0, -1, 1], start=1)
    path = str(tmp_path / "g.npz")
    g.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["next", "start", "token_class"]
    back = Guide.load(path)
    assert back == g and back.start == 1 and hash(back) == hash(g)
    monkeypatch.delenv(guide_mod.GUIDE_ENV, raising=False)
    assert guide_mod.env_guide() is None and guide_mod.resolve(None, None, use_env=True) is None
    monkeypatch.setenv(guide_mod.GUIDE_ENV, path)
    assert guide_mod.env_guide() == g and guide_mod.resolve(None, None, use_env=True) == g
    assert guide_mod.resolve(None, 0.0, use_env=True) == g
    assert guide_mod.resolve(None, None, use_env=False) is None
    assert guide_mod.resolve(None, 0.5, use_env=True) is None                  # the default stays out of the T > 0 path
    other = Guide([[0]])
    assert guide_mod.resolve(other, None, use_env=True) is other               # the argument wins
    np.savez(str(tmp_path / "bad.npz"), next=g.next)
    with pytest.raises(ValueError, match="token_class"):
        Guide.load(str(tmp_path / "bad.npz"))


def test_resolve_refuses():
    g = Guide([[0]])
    with pytest.raises(TypeError, match="longspec_amd.Guide"):
        guide_mod.resolve([[0]], None, use_env=False)
    with pytest.raises(ValueError, match="temperature"):
        guide_mod.resolve(g, 0.5, use_env=True)
    assert guide_mod.resolve(g, 0.0, use_env=False) is g and guide_mod.resolve(g, None, use_env=False) is g
