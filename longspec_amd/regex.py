"""A regular expression as a minimal byte-level DFA (the front door of ``guide=``: ``Guide.from_regex``).

``compile(pattern)`` gives the DFA whose language is that of ``re.fullmatch(pattern, text, re.ASCII)`` over UTF-8 encoded text,
for this subset:

    literals (a non-ASCII character stands for its UTF-8 bytes), ``\\n \\t \\r \\f \\v \\0 \\xHH``, a backslash in front of any
    non-alphanumeric character; ``\\d \\w \\s \\D \\W \\S`` with ASCII semantics; ``.`` (any character but ``\\n``);
    ``[...]`` with ranges (ASCII end points), escapes and non-ASCII members, ``[^...]`` with ASCII members only;
    ``( )``, ``(?: )``, ``|``; ``* + ? {m} {m,} {m,n}``, greedy only.

``.``, ``[^...]``, ``\\D \\W \\S`` and a positive class that holds one of ``\\D \\W \\S`` also match every WELL-FORMED multi-byte
UTF-8 sequence (the 2-, 3- and 4-byte rows of the Unicode standard's table: no surrogates, no overlong forms, nothing above
U+10FFFF) and never a stray byte >= 0x80.  Everything else -- anchors, ``\\b \\B \\A \\Z``, back-references, look-around, named
groups, flags, lazy and possessive quantifiers, a non-ASCII member of a negated class, a non-ASCII range end, ``{m,n}`` with
n < m, an unbalanced ``(`` or ``[`` -- raises ValueError naming the construct and its offset in the pattern.

Pipeline: parse -> epsilon-NFA -> subset construction over byte classes -> drop the states that reach no accepting state ->
Moore minimisation -> renumber breadth-first from the start in byte order.  The renumbering makes the arrays a function of the
language: two patterns with the same language give identical arrays.  Host only, pure Python / numpy.
"""
from __future__ import annotations

import re as _re
from collections import namedtuple

import numpy as np

ByteDFA = namedtuple("ByteDFA", ["next", "accepting", "start"])     # int64 [S, 256] (-1 = dead), bool [S], 0

_MAX_NFA = 1 << 18           # epsilon-NFA states: a bounded repeat beyond this cannot stay within any max_states
_ASCII = (1 << 128) - 1


def _mask(chars) -> int:
    m = 0
    for c in chars:
        m |= 1 << (c if isinstance(c, int) else ord(c))
    return m


def _span(lo: int, hi: int) -> int:
    return ((1 << (hi + 1)) - 1) & ~((1 << lo) - 1)


_DIGIT = _span(0x30, 0x39)
_WORD = _DIGIT | _span(0x41, 0x5A) | _span(0x61, 0x7A) | _mask("_")
_SPACE = _mask(" \t\n\r\f\v")
_SHORT = {"d": _DIGIT, "w": _WORD, "s": _SPACE}
_CONT = _span(0x80, 0xBF)
# the well-formed multi-byte sequences (Unicode standard, table 3-7): the byte sets of each position
_UTF8_ROWS = (
    (_span(0xC2, 0xDF), _CONT),
    (_span(0xE0, 0xE0), _span(0xA0, 0xBF), _CONT),
    (_span(0xE1, 0xEC), _CONT, _CONT),
    (_span(0xED, 0xED), _span(0x80, 0x9F), _CONT),
    (_span(0xEE, 0xEF), _CONT, _CONT),
    (_span(0xF0, 0xF0), _span(0x90, 0xBF), _CONT, _CONT),
    (_span(0xF1, 0xF3), _CONT, _CONT, _CONT),
    (_span(0xF4, 0xF4), _span(0x80, 0x8F), _CONT, _CONT),
)
_BRACE = _re.compile(r"\{(\d*)(?:(,)(\d*))?\}")
_ESC_CHAR = {"n": "\n", "t": "\t", "r": "\r", "f": "\f", "v": "\v"}

# ---- the syntax tree: ("set", mask of bytes) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, lo, hi or None) | ("none",)
_MULTIBYTE = ("alt", [("cat", [("set", m) for m in row]) for row in _UTF8_ROWS])


def _char_node(ch: str):
    return ("cat", [("set", 1 << b) for b in ch.encode("utf-8")])


def _class_node(ascii_mask: int, multibyte: bool, members):
    alts = []
    if ascii_mask:
        alts.append(("set", ascii_mask))
    if multibyte:
        alts.append(_MULTIBYTE)
    else:
        alts.extend(_char_node(ch) for ch in sorted(members))
    if not alts:
        return ("none",)
    return alts[0] if len(alts) == 1 else ("alt", alts)


class _Parser:
    def __init__(self, pattern: str):
        self.p, self.i = pattern, 0

    def fail(self, what: str, at: int):
        raise ValueError(f"regex: {what} at offset {at} of {self.p!r}: outside the supported subset (longspec_amd/regex.py)")

    def peek(self, k: int = 0) -> str:
        return self.p[self.i + k] if self.i + k < len(self.p) else ""

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("an unbalanced ')'", self.i)
        return node

    def alt(self):
        branches = [self.seq()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.seq())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def seq(self):
        items = []
        while self.i < len(self.p) and self.p[self.i] not in "|)":
            items.append(self.quantified(self.atom()))
        return ("cat", items)

    def brace(self):
        """The match of a ``{...}`` quantifier at the cursor, as ``re`` reads it (``{}`` and anything else is a literal)."""
        m = _BRACE.match(self.p, self.i)
        return m if m and m.group(0) != "{}" else None

    def atom(self):
        at, c = self.i, self.p[self.i]
        if c == "(":
            self.i += 1
            if self.peek() == "?":
                kind = self.p[at + 2:at + 4]
                if kind[:1] == ":":
                    self.i += 2
                elif kind[:1] in ("=", "!") or kind in ("<=", "<!"):
                    self.fail("look-around", at)
                elif kind == "P=":
                    self.fail("a back-reference", at)
                elif kind[:1] in ("P", "<"):
                    self.fail("a named group", at)
                else:
                    self.fail("a flag or extension group '(?...'", at)
            node = self.alt()
            if self.peek() != ")":
                self.fail("an unbalanced '('", at)
            self.i += 1
            return node
        if c == "[":
            return self.char_class()
        if c == ".":
            self.i += 1
            return _class_node(_ASCII & ~_mask("\n"), True, ())
        if c in "^$":
            self.fail(f"the anchor {c!r}", at)
        if c in "*+?" or (c == "{" and self.brace()):
            self.fail("a quantifier with nothing to repeat", at)
        if c == "\\":
            kind, v = self.escape()
            if kind == "c":
                return _char_node(v)
            if v.islower():
                return ("set", _SHORT[v])
            return _class_node(_ASCII & ~_SHORT[v.lower()], True, ())
        self.i += 1
        return _char_node(c)

    def quantified(self, node):
        at, c = self.i, self.peek()
        if c == "*":
            lo, hi, n = 0, None, 1
        elif c == "+":
            lo, hi, n = 1, None, 1
        elif c == "?":
            lo, hi, n = 0, 1, 1
        elif c == "{" and self.brace():
            m = self.brace()
            if m.group(1) == "":
                self.fail("a repeat without a lower bound '{,n}'", at)
            lo = int(m.group(1))
            hi = lo if m.group(2) is None else (int(m.group(3)) if m.group(3) else None)
            if hi is not None and hi < lo:
                self.fail(f"the repeat {m.group(0)} with n < m", at)
            n = len(m.group(0))
        else:
            return node
        self.i += n
        c = self.peek()
        if c == "?":
            self.fail("a lazy quantifier", at)
        if c == "+":
            self.fail("a possessive quantifier", at)
        if c == "*" or (c == "{" and self.brace()):
            self.fail("a quantifier behind a quantifier", self.i)
        return ("rep", node, lo, hi)

    def escape(self):
        """The escape at the cursor: ("c", the character) or ("s", one of dwsDWS)."""
        at, e = self.i, self.peek(1)
        if e == "":
            self.fail("a backslash at the end", at)
        self.i += 2
        if e in "dwsDWS":
            return "s", e
        if e in _ESC_CHAR:
            return "c", _ESC_CHAR[e]
        if e == "0":
            if self.peek() and self.peek() in "01234567":
                self.fail("an octal escape", at)
            return "c", "\0"
        if e == "x":
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or any(ch not in "0123456789abcdefABCDEF" for ch in h):
                self.fail("an incomplete \\xHH escape", at)
            self.i += 2
            return "c", chr(int(h, 16))
        if e in "123456789":
            self.fail("a back-reference", at)
        if e in "bBAZ":
            self.fail(f"the anchor \\{e}", at)
        if e.isalnum():
            self.fail(f"the escape \\{e}", at)
        return "c", e

    def char_class(self):
        at = self.i
        self.i += 1
        negated = self.peek() == "^"
        if negated:
            self.i += 1
        mask, members, wide, first = 0, {}, False, True          # members: non-ASCII character -> its offset

        def element():
            if self.i >= len(self.p):
                self.fail("an unbalanced '['", at)
            if self.p[self.i] == "\\":
                return self.escape()
            self.i += 1
            return "c", self.p[self.i - 1]

        while True:
            if self.i >= len(self.p):
                self.fail("an unbalanced '['", at)
            if self.p[self.i] == "]" and not first:
                self.i += 1
                break
            first = False
            e_at = self.i
            kind, v = element()
            if self.peek() == "-" and self.peek(1) not in ("", "]"):
                self.i += 1
                h_at = self.i
                kind2, w = element()
                if kind != "c" or kind2 != "c":
                    self.fail("a class shorthand as the end of a range", e_at)
                if ord(v) > 127 or ord(w) > 127:
                    self.fail("a non-ASCII range end", e_at if ord(v) > 127 else h_at)
                if ord(w) < ord(v):
                    self.fail(f"the reversed range {v}-{w}", e_at)
                mask |= _span(ord(v), ord(w))
            elif kind == "s":
                if v.islower():
                    mask |= _SHORT[v]
                else:
                    mask |= _ASCII & ~_SHORT[v.lower()]
                    wide = True
            elif ord(v) > 127:
                members.setdefault(v, e_at)
            else:
                mask |= 1 << ord(v)
        if negated:
            if members:
                self.fail("a non-ASCII member in a negated class", min(members.values()))
            return _class_node(_ASCII & ~mask, not wide, ())
        return _class_node(mask, wide, members)


class _NFA:
    def __init__(self):
        self.eps, self.tr = [], []                                 # per state: epsilon targets; (byte mask, target)

    def new(self) -> int:
        if len(self.eps) >= _MAX_NFA:
            raise ValueError(f"regex: the pattern needs more than {_MAX_NFA} NFA states")
        self.eps.append([])
        self.tr.append([])
        return len(self.eps) - 1

    def build(self, node):
        """(first, last) of a fresh fragment for `node`."""
        kind = node[0]
        if kind == "set":
            s, e = self.new(), self.new()
            self.tr[s].append((node[1], e))
            return s, e
        if kind == "none":
            return self.new(), self.new()
        if kind == "cat":
            s = cur = self.new()
            for it in node[1]:
                a, b = self.build(it)
                self.eps[cur].append(a)
                cur = b
            return s, cur
        if kind == "alt":
            s, e = self.new(), self.new()
            for it in node[1]:
                a, b = self.build(it)
                self.eps[s].append(a)
                self.eps[b].append(e)
            return s, e
        _, sub, lo, hi = node
        s = cur = self.new()
        e = self.new()
        for _ in range(lo):
            a, b = self.build(sub)
            self.eps[cur].append(a)
            cur = b
        if hi is None:
            a, b = self.build(sub)
            loop = self.new()
            self.eps[cur].append(loop)
            self.eps[loop] += [a, e]
            self.eps[b].append(loop)
        else:
            for _ in range(hi - lo):
                self.eps[cur].append(e)
                a, b = self.build(sub)
                self.eps[cur].append(a)
                cur = b
            self.eps[cur].append(e)
        return s, e


def _byte_classes(masks):
    """The coarsest partition of 0..255 that every mask is a union of: (class of every byte, int [256]; number of classes),
    the classes numbered by their smallest byte."""
    blocks = [(1 << 256) - 1]
    for m in masks:
        nxt = []
        for b in blocks:
            inside, outside = b & m, b & ~m
            if inside:
                nxt.append(inside)
            if outside:
                nxt.append(outside)
        blocks = nxt
    blocks.sort(key=lambda b: (b & -b).bit_length())
    of = np.zeros(256, dtype=np.int64)
    for k, b in enumerate(blocks):
        for byte in range(256):
            if (b >> byte) & 1:
                of[byte] = k
    return of, blocks


def _subset(nfa: _NFA, first: int, last: int, blocks, max_states: int):
    """Subset construction over the byte classes: (table int64 [n, K], -1 = none; accepting bool [n])."""
    n, K = len(nfa.eps), len(blocks)
    closure = [None] * n
    for s in range(n):
        seen, stack = {s}, [s]
        while stack:
            for t in nfa.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        closure[s] = frozenset(seen)
    moves = [[([k for k in range(K) if blocks[k] & m], t) for m, t in nfa.tr[s]] for s in range(n)]
    start = closure[first]
    index, order, rows = {start: 0}, [start], []
    at = 0
    while at < len(order):
        cur, at = order[at], at + 1
        to = [None] * K
        for s in cur:
            for ks, t in moves[s]:
                for k in ks:
                    if to[k] is None:
                        to[k] = set()
                    to[k] |= closure[t]
        row = [-1] * K
        for k in range(K):
            if to[k]:
                key = frozenset(to[k])
                j = index.get(key)
                if j is None:
                    if len(order) >= max_states:
                        raise ValueError(f"regex: the subset construction needs more than max_states = {max_states} states")
                    j = index[key] = len(order)
                    order.append(key)
                row[k] = j
        rows.append(row)
    table = np.array(rows, dtype=np.int64).reshape(len(order), K)
    return table, np.array([last in s for s in order], dtype=bool)


def _trim(table, accepting):
    """Keep the states that reach an accepting state (transitions into the others become -1); None: the language is empty."""
    n = table.shape[0]
    live = accepting.copy()
    while True:
        reach = np.where(table >= 0, live[np.maximum(table, 0)], False).any(axis=1) | live
        if (reach == live).all():
            break
        live = reach
    if not live[0]:
        return None
    new = np.cumsum(live) - 1
    t = table[live]
    t = np.where((t >= 0) & live[np.maximum(t, 0)], new[np.maximum(t, 0)], -1)
    return t, accepting[live]


def _minimise(table, accepting):
    """Moore: refine (accepting?) by the labels of the successors until nothing splits.  Every state is live, 0 is the start."""
    n, K = table.shape
    label = accepting.astype(np.int64)
    count = len(np.unique(label))
    while True:
        succ = np.where(table >= 0, label[np.maximum(table, 0)], -1)
        _, new = np.unique(np.concatenate([label[:, None], succ], axis=1), axis=0, return_inverse=True)
        new = np.asarray(new).reshape(-1)
        c = int(new.max()) + 1
        label = new
        if c == count:
            break
        count = c
    rep = np.full(count, -1, dtype=np.int64)
    rep[label[::-1]] = np.arange(n)[::-1]                          # the first state of every block
    t = table[rep]
    t = np.where(t >= 0, label[np.maximum(t, 0)], -1)
    return t, accepting[rep], int(label[0])


def _renumber(table, accepting, start):
    """Breadth-first from `start`, classes in the order of their smallest byte (= byte order 0..255)."""
    n = table.shape[0]
    new = np.full(n, -1, dtype=np.int64)
    new[start] = 0
    order = [start]
    for s in order:
        for t in table[s]:
            if t >= 0 and new[t] < 0:
                new[t] = len(order)
                order.append(int(t))
    order = np.array(order)                                        # (every state is reachable: subset construction)
    t = table[order]
    return np.where(t >= 0, new[np.maximum(t, 0)], -1), accepting[order]


def compile(pattern: str, max_states: int = 4096) -> ByteDFA:
    """The minimal byte DFA of `pattern` (the module's docstring: the subset, the semantics, the errors).  ValueError with the
    word "states" where the subset construction or the result needs more than `max_states`; ValueError where the language is
    empty."""
    if not isinstance(pattern, str):
        raise TypeError(f"regex: pattern must be a str, got {type(pattern).__name__}")
    if isinstance(max_states, bool) or not isinstance(max_states, int) or max_states < 1:
        raise ValueError(f"regex: max_states must be a positive integer, got {max_states!r}")
    tree = _Parser(pattern).parse()
    nfa = _NFA()
    first, last = nfa.build(tree)
    of, blocks = _byte_classes(sorted({m for row in nfa.tr for m, _ in row}))
    table, accepting = _subset(nfa, first, last, blocks, max_states)
    trimmed = _trim(table, accepting)
    if trimmed is None:
        raise ValueError(f"regex: the language of {pattern!r} is empty")
    table, accepting, start = _minimise(*trimmed)
    table, accepting = _renumber(table, accepting, start)
    if table.shape[0] > max_states:
        raise ValueError(f"regex: the minimal DFA has {table.shape[0]} states, more than max_states = {max_states}")
    nxt = np.ascontiguousarray(table[:, of])
    nxt.setflags(write=False)
    accepting = np.ascontiguousarray(accepting)
    accepting.setflags(write=False)
    return ByteDFA(nxt, accepting, 0)


def matches(dfa: ByteDFA, data: bytes) -> bool:
    """Whether the DFA accepts `data` as a whole."""
    s = dfa.start
    for b in data:
        s = int(dfa.next[s, b])
        if s < 0:
            return False
    return bool(dfa.accepting[s])


def _byte_level_table():
    """The GPT-2 byte-to-unicode table (also Llama-3's and Qwen2's): printable bytes stand for themselves, the others for
    U+0100 onwards in byte order.  Returns character -> byte."""
    keep = list(range(0x21, 0x7F)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    table, n = {}, 0
    for b in range(256):
        if b in keep:
            table[chr(b)] = b
        else:
            table[chr(256 + n)] = b
            n += 1
    return table


def token_bytes_of_byte_level_vocab(vocab, size=None):
    """The byte string of every id of a byte-level BPE vocabulary (``vocab``: token string -> id, as a GPT-2 / Llama-3 / Qwen2
    tokenizer's ``get_vocab()`` gives it): a list of ``size`` (None: the largest id + 1) bytes objects.  An id whose string holds
    a character outside the byte table (a special token) and an id the dict does not have get ``b""``, which ``Guide`` forbids."""
    table = _byte_level_table()
    ids = list(vocab.values())
    for v in ids:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError(f"regex: {v!r} is not a token id")
    n = (max(ids) + 1 if ids else 0) if size is None else int(size)
    out = [b""] * n
    for text, v in vocab.items():
        if v < n and text and all(ch in table for ch in text):
            out[int(v)] = bytes(table[ch] for ch in text)
    return out
