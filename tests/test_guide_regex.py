"""``longspec_amd.regex`` (pattern -> minimal byte DFA) against ``re.fullmatch(p, s, re.ASCII)`` over UTF-8 text, the shape of
its result, its refusals, ``Guide.from_regex`` on a toy vocabulary and the byte-level vocabulary helper.  No GPU."""
import itertools
import re

import numpy as np
import pytest

from longspec_amd import Guide, regex

PATTERNS = ["a", "(ab|a)*c?", "[a-c]{2,3}x+", r"\d+(\.\d+)?", "[^ab]b", ".a", r"-?(0|[1-9]\d*)(\.\d+)?([eE][+-]?\d+)?",
            "(yes|no|maybe)", r"\w+@\w+\.(com|org)", "[é€a]+", r"\s*\{\"a\": (true|false)\}", "a{0,3}b{2}", "(a|b)*abb", r"[\D]x",
            "é*€?"]
ALWAYS = "é€\n"


def alphabet(p):
    """At most 14 characters: the pattern's own literal characters (11 at the most) and é, € and the line feed."""
    own = sorted({c for c in p if c.isalnum() or c in '@.{}": -+'})[:11]
    return sorted(set(own) | set(ALWAYS))


@pytest.mark.parametrize("p", PATTERNS)
def test_the_language_is_that_of_re_fullmatch(p):
    dfa = regex.compile(p)
    want = re.compile(p, re.ASCII)
    chars = alphabet(p)
    assert len(chars) <= 14 and all(c in chars for c in ALWAYS)
    wrong = [s for n in range(5) for s in map("".join, itertools.product(chars, repeat=n))
             if regex.matches(dfa, s.encode("utf-8")) != (want.fullmatch(s) is not None)]
    assert not wrong, (p, wrong[:5])


@pytest.mark.parametrize("p", [".", "[^a]"])
def test_ill_formed_bytes_never_match(p):
    one, two = regex.compile(p), regex.compile(p + "a")
    for bad in (b"\xff", b"\xc3", b"\xc0\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80"):
        assert not regex.matches(one, bad) and not regex.matches(two, bad + b"a"), (p, bad)
        assert not regex.matches(regex.compile(f"({p})*"), bad), (p, bad)
    for good in ("\u00e9", "\u20ac", "\U0001F600", "\ufffd", "\u0800", "\U0010FFFF", "\ud7ff", "\ue000", "x"):
        assert regex.matches(one, good.encode("utf-8")), (p, good)


def test_the_shape_is_minimal_and_canonical():
    d = regex.compile("(a|b)*abb")
    assert d.next.shape == (4, 256) and d.next.dtype == np.int64 and d.accepting.dtype == bool and d.start == 0
    assert regex.compile("a").next.shape == (2, 256)
    e = regex.compile("(b|a)*abb")
    assert (d.next == e.next).all() and (d.accepting == e.accepting).all()
    f = regex.compile("(?:a|b)*ab{2}")
    assert (d.next == f.next).all() and (d.accepting == f.accepting).all()
    for p in PATTERNS:
        d = regex.compile(p)
        S = d.next.shape[0]
        assert d.start == 0 and d.accepting.shape == (S,) and d.next.min() >= -1 and d.next.max() < S
        reach = d.accepting.copy()                                # every state reaches an accepting one
        for _ in range(S):
            reach |= np.where(d.next >= 0, reach[np.maximum(d.next, 0)], False).any(axis=1)
        assert reach.all(), p
        seen, front = {0}, [0]                                    # ... is reachable, and numbered breadth-first in byte order
        for s in front:
            for t in d.next[s]:
                if t >= 0 and int(t) not in seen:
                    assert int(t) == len(seen), p
                    seen.add(int(t))
                    front.append(int(t))
        assert len(seen) == S, p


REFUSED = [("^a", 0), ("a$", 1), (r"a\b", 1), (r"\Ba", 0), (r"\Aa", 0), (r"a\Z", 1), (r"(a)\1", 3), ("(?P=n)", 0), ("(?=a)", 0),
           ("a(?!b)", 1), ("(?<=a)b", 0), ("(?<!a)b", 0), ("(?P<n>a)", 0), ("(?i)a", 0), ("a*?", 1), ("a+?", 1), ("a??", 1),
           ("a{2}?", 1), ("a*+", 1), ("a++", 1), ("[^é]", 2), ("[^aé]", 3), ("[a-é]", 3), ("[é-€]", 1), ("a{3,2}", 1), ("(a", 0),
           ("a(b(c)", 1), ("[a", 0), ("ab[^c", 2), ("a)", 1), ("*a", 0), (r"\pL", 0)]


@pytest.mark.parametrize("p,offset", REFUSED)
def test_everything_else_is_refused_with_its_offset(p, offset):
    with pytest.raises(ValueError, match=f"offset {offset} of"):
        regex.compile(p)


def test_the_state_bound_and_the_empty_language():
    with pytest.raises(ValueError, match="states"):
        regex.compile("(a|b)*a(a|b){12}")
    assert regex.compile("(a|b)*a(a|b){12}", max_states=16384).next.shape[0] == 8192
    with pytest.raises(ValueError, match="states"):
        regex.compile("(a|b)*a(a|b){12}", max_states=8191)
    with pytest.raises(ValueError, match="states"):
        regex.compile("abcdef", max_states=6)
    assert regex.compile("abcdef", max_states=7).next.shape[0] == 7
    with pytest.raises(ValueError, match="empty"):
        regex.compile(r"a[^\d\D]")


# ---- Guide.from_regex on a toy vocabulary ----------------------------------------------------------------------------
def toy_vocab():
    """About 300 tokens of 1-6 bytes: every printable ASCII byte, é and € whole and in pieces, words, numbers, duplicates, an
    empty token; the last id is the end-of-sequence token, whose bytes look like text."""
    rng = np.random.default_rng(7)
    toks = [bytes([b]) for b in range(0x20, 0x7F)] + [b"\n", "é".encode(), "€".encode(), b"\xc3", b"\xa9", b"\xe2\x82", b"\xac",
                                                      b"\xe2", b"\x82\xac", b""]
    toks += [w.encode() for w in ("yes", "no", "maybe", "may", "be", "true", "false", "tr", "ue", ".com", ".org", "com", "org", "@",
                                  '{"a"', '": ', '{"a": ', "tru", "e}", "abb", "ab", "ba", "aab", "bb", "0.", ".5", "1e", "e+", "-1")]
    digits, letters = b"0123456789", b"abcxyz_@.e"
    while len(toks) < 290:
        src = digits if rng.random() < 0.5 else letters + digits
        toks.append(bytes(rng.choice(list(src), size=int(rng.integers(2, 7))).tolist()))
    toks += toks[100:109]                                          # duplicates
    toks.append(b"<eos>")
    return toks, len(toks) - 1


@pytest.mark.parametrize("p", [r"-?(0|[1-9]\d*)(\.\d+)?([eE][+-]?\d+)?", r"\w+@\w+\.(com|org)", r"\s*\{\"a\": (true|false)\}", "(a|b)*abb",
                               "[é€a]+", "(yes|no|maybe)"])
def test_from_regex_on_a_toy_vocabulary(p):
    toks, eos = toy_vocab()
    g = Guide.from_regex(p, toks, eos)
    want = re.compile(p, re.ASCII)
    dfa = regex.compile(p)
    assert g.start == 0 and g.token_class[eos] == g.classes - 1 and g.token_class[toks.index(b"")] == -1
    F = g.states - 1
    rng = np.random.default_rng(len(p))
    usable = [t for t in range(len(toks)) if t != eos]
    hits = 0
    for trial in range(400):
        if trial % 2:                                              # a walk along the guide: mostly inside the language
            seq, s = [], g.start
            for _ in range(12):
                ok = [t for t in usable if g.step(s, t) >= 0]
                if not ok or (g.step(s, eos) >= 0 and rng.random() < 0.5):
                    break
                seq.append(int(rng.choice(ok)))
                s = g.step(s, seq[-1])
        else:
            seq = rng.choice(usable, size=int(rng.integers(0, 5))).tolist()
        data = b"".join(toks[t] for t in seq)
        try:
            full = all(toks[t] for t in seq) and want.fullmatch(data.decode("utf-8")) is not None
        except UnicodeDecodeError:
            full = False
        assert (g.walk(seq + [eos]) >= 0) == full == (all(toks[t] for t in seq) and regex.matches(dfa, data)), (p, seq)
        hits += full
        if full:                                                   # behind the end only the end is legal
            assert g.walk(seq + [eos]) == F
            assert [t for t in range(len(toks)) if g.step(F, t) >= 0] == [eos]
    assert hits >= 20, (p, hits)
    # from every reachable state the final state is reachable, over tokens the vocabulary has
    tc = g.token_class
    used = np.zeros(g.classes, dtype=bool)
    used[tc[tc >= 0]] = True
    live = np.where(used[None, :], g.next, -1)
    seen, front = {0}, [0]
    for s in front:
        for t in np.unique(live[s][live[s] >= 0]).tolist():
            if t not in seen:
                seen.add(t)
                front.append(t)
    good = np.zeros(g.states, dtype=bool)
    good[F] = True
    for _ in range(g.states):
        good |= np.where(live >= 0, good[np.maximum(live, 0)], False).any(axis=1)
    assert F in seen and all(good[s] for s in seen), p
    table = g.table(len(toks), "cpu")
    assert table[0] == g.states and table[1] == g.classes


def test_a_vocabulary_that_cannot_spell_the_language():
    toks, eos = toy_vocab()
    with pytest.raises(ValueError, match="cannot spell"):
        Guide.from_regex("(yes|no)\t", toks, eos)                  # no token holds a tab
    g = Guide.from_regex("(yes\t|no)", toks, eos)                  # one branch cannot end: it is cut off at its first token
    assert g.walk([toks.index(b"no"), eos]) >= 0
    assert g.walk([toks.index(b"yes")]) < 0 and g.walk([toks.index(b"y")]) < 0 and g.walk([toks.index(b"n")]) >= 0
    assert Guide.from_regex("a*", toks, eos).walk([eos]) >= 0      # the empty text matches
    with pytest.raises(ValueError):
        Guide.from_regex("a", toks, -1)


def test_from_byte_dfa_is_unchanged_by_the_new_argument():
    toks, _ = toy_vocab()
    d = regex.compile(r"\d+(\.\d+)?")
    assert Guide.from_byte_dfa(d.next, toks) == Guide.from_byte_dfa(d.next, toks, 0, None) == Guide.from_byte_dfa(d.next, toks, device="cpu")


# ---- the byte-level vocabulary helper --------------------------------------------------------------------------------
def byte_to_unicode():
    """The published GPT-2 table, written out independently of the module's."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, map(chr, cs)))


def test_the_byte_level_vocabulary_helper():
    enc = byte_to_unicode()
    assert enc[ord(" ")] == "Ġ" and enc[ord("\n")] == "Ċ" and enc[ord("a")] == "a"
    vocab = {enc[b]: b for b in range(256)}
    vocab["ĠHello"] = 256
    vocab["Ã©"] = 257                                             # the two bytes of é
    vocab["<|endoftext|>"] = 259                                   # (258 is a hole)
    vocab["<|weird|>ḁ"] = 260                                      # a character outside the table
    got = regex.token_bytes_of_byte_level_vocab(vocab)
    assert len(got) == 261 and got[:256] == [bytes([b]) for b in range(256)]
    assert got[256] == b" Hello" and got[257] == "é".encode("utf-8") and got[258] == b"" and got[260] == b""
    assert got[259] == b"<|endoftext|>"                            # plain ASCII: the caller names its end-of-sequence id
    assert regex.token_bytes_of_byte_level_vocab(vocab, size=300)[261:] == [b""] * 39
    assert regex.token_bytes_of_byte_level_vocab(vocab, size=100) == got[:100]
    assert regex.token_bytes_of_byte_level_vocab({}) == []
