"""Guided decoding: a deterministic automaton over token ids on the TARGET's logits (``guide=`` of the generate loops and the
``begin_*_decode`` entry points).

With ``guide`` set, the generated text must be a walk of a DFA whose alphabet is the token ids: in each state only the tokens
with a transition are legal, the entries of every other token of the TARGET's logits become ``-inf`` -- behind the penalties,
next to the bans of ``stop=`` and ``ban=``, in front of the arg-max or draw and of the log-probs.  The text is then exactly
guided decoding of the target, whichever loop produced it; draft passes are untouched, a draft that leaves the language is
rejected.

The alphabet is compressed: ``token_class`` maps a token id to a class in ``[0, C)`` (``-1``: forbidden in every state; ids
beyond the array: forbidden in every state) and ``next`` is ``[S, C]`` with entries in ``[-1, S)`` (``-1``: no transition).
``walk(s, id) = next[s, token_class[id]]``, or ``-1`` where ``s < 0``, the id lies outside ``[0, vocab)`` or its class is
forbidden; ``-1`` is the dead state and stays dead.

For a row of target logits the row's text is the generated columns (column 0 being the prefill's token; the prompt is NOT part
of it: the automaton is in ``start`` in front of column 0, as ``stop=`` and ``ban=`` start at column 0) followed, in a
verification pass, by the draft tokens the row follows -- ``extra_ids[z, c]`` with ``extra_mask[z, r, c] != 0``, in increasing
``c``, which is path order for the chain and for both level-major trees.  The state of the committed text is kept per batch row
(``state`` int32 [b], advanced behind every commit by ``ops.guide_advance``); the row's state ``s`` is that state walked along
its path.  ``s < 0``: the row is dead and keeps its bits -- its parent's logits forbid the token that killed it, so it is never
accepted.  Otherwise every ``v`` in ``[0, V)`` with ``walk(s, v) < 0`` gets the type's ``-inf`` pattern; every other element
keeps its bits.  A live row in which everything is forbidden is the caller's error (``table`` refuses the reachable ones).

Where guides come from: the constructor (any table), ``Guide.choice`` (one of these answers, then EOS), ``Guide.from_byte_dfa``
(a byte-level DFA lifted to the tokens of a vocabulary, on the host or -- ``device=`` -- by ``ops.guide_lift``) and
``Guide.from_regex`` (``longspec_amd/regex.py`` compiles the pattern to the byte DFA; then the lift, then EOS).

The device side (``ops.guide_rows`` / ``ops.guide_advance``) reads one int32 table, built once per decode state:

    [0] S   [1] C   [2] start   [3] vocab   [4] the word count   [5 : 8] reserved (0)
    [8 : 8 + K]          the classes of ids 0 .. vocab - 1 as 16-bit values, two per word (the even id in the low half),
                         0xFFFF = forbidden; K = ceil(vocab / 2) rounded up to a multiple of 4 words, the padding 0xFFFF,
                         so that the transition area starts 16-byte aligned
    [8 + K : 8 + K + S * C]   ``next`` as int32 [S, C], row-major
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .keyword import resolve_keyword

GUIDE_ENV = "LONGSPEC_GUIDE"     # path of a Guide.save() file: the process-wide default
MAX_CLASSES = 16384              # C (LS_GUIDE_MAX_CLASSES): a state's allow bits are at most 2 KB
MAX_CELLS = 1 << 24              # S * C (LS_GUIDE_MAX_CELLS): the transition area is at most 64 MB
HEADER_WORDS = 8                 # (LS_GUIDE_HEADER_WORDS)
NO_CLASS = 0xFFFF                # the 16-bit class of a forbidden id (LS_GUIDE_NO_CLASS)
LIFT_MAX_STATES = 16384          # byte-DFA states the device lifts (LS_GUIDE_LIFT_MAX_STATES)


def _int_array(v, what, ndim):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    try:
        a = np.asarray(v)
    except Exception:
        raise TypeError(f"Guide: {what} must be an integer array, got {type(v).__name__}") from None
    if a.dtype == object or a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"Guide: {what} must be an integer array, got dtype {a.dtype}")
    if a.ndim != ndim:
        raise ValueError(f"Guide: {what} must have {ndim} dimension{'s' if ndim > 1 else ''}, got shape {tuple(a.shape)}")
    return np.ascontiguousarray(a.astype(np.int64))


def class_words(vocab: int) -> int:
    """Words of the class area of a table for ``vocab`` ids (K of the module's docstring)."""
    return ((vocab + 1) // 2 + 3) // 4 * 4


class Guide:
    """``Guide(next, token_class=None, start=0)``: a DFA over token ids.  ``next`` int [S, C], entries in [-1, S) (-1: no
    transition); ``token_class`` int [n], entries in [-1, C) (-1 and ids >= n: forbidden in every state; None: the identity,
    C ids); ``start`` in [0, S).  1 <= S, 1 <= C <= 16384, S * C <= 2^24."""

    __slots__ = ("next", "token_class", "start", "_hash")

    def __init__(self, next, token_class=None, start=0):
        nx = _int_array(next, "next", 2)
        S, C = nx.shape
        if S < 1:
            raise ValueError(f"Guide: next needs at least one state, got shape {tuple(nx.shape)}")
        if not (1 <= C <= MAX_CLASSES):
            raise ValueError(f"Guide: next has 1..{MAX_CLASSES} classes (columns), got {C}")
        if S * C > MAX_CELLS:
            raise ValueError(f"Guide: next holds at most {MAX_CELLS} entries, got {S} x {C}")
        if nx.min() < -1 or nx.max() >= S:
            raise ValueError(f"Guide: the entries of next are -1 (no transition) or a state 0..{S - 1}")
        if token_class is None:
            tc = np.arange(C, dtype=np.int64)
        else:
            tc = _int_array(token_class, "token_class", 1)
            if tc.size and (tc.min() < -1 or tc.max() >= C):
                raise ValueError(f"Guide: the entries of token_class are -1 (forbidden) or a class 0..{C - 1}")
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)):
            raise TypeError(f"Guide: start must be an integer, got {start!r}")
        if not (0 <= start < S):
            raise ValueError(f"Guide: start must be a state 0..{S - 1}, got {start!r}")
        nx.setflags(write=False)
        tc.setflags(write=False)
        self.next, self.token_class, self.start = nx, tc, int(start)
        self._hash = None

    @property
    def states(self):
        return self.next.shape[0]

    @property
    def classes(self):
        return self.next.shape[1]

    def __repr__(self):
        return f"Guide(states={self.states}, classes={self.classes}, tokens={self.token_class.size}, start={self.start})"

    def _key(self):
        return (self.next.shape, self.start, self.next.tobytes(), self.token_class.tobytes())

    def __eq__(self, other):
        return isinstance(other, Guide) and self._key() == other._key()

    def __hash__(self):
        if self._hash is None:
            self._hash = hash(("Guide",) + self._key())
        return self._hash

    # --------------------------------------------------------------------------------------------------------------------
    def step(self, state: int, token: int, vocab=None) -> int:
        """``walk(state, token)`` of the module's docstring (``vocab``: None = no bound beyond ``token_class``)."""
        if state < 0 or token < 0 or token >= self.token_class.size or (vocab is not None and token >= vocab):
            return -1
        c = int(self.token_class[token])
        return -1 if c < 0 else int(self.next[state, c])

    def walk(self, tokens, state=None, vocab=None) -> int:
        """The state behind ``tokens``, from ``state`` (None: ``start``); -1 once dead."""
        s = self.start if state is None else int(state)
        for t in tokens:
            s = self.step(s, int(t), vocab)
        return s

    def _classes_of(self, vocab: int):
        """int64 [vocab]: the class of every id below ``vocab``, -1 where forbidden."""
        tc = np.full(vocab, -1, dtype=np.int64)
        n = min(vocab, self.token_class.size)
        tc[:n] = self.token_class[:n]
        return tc

    def table(self, vocab: int, device):
        """A new int32 table of this object for a vocabulary of ``vocab`` ids on `device` (layout: the module's docstring).  The
        object keeps no tensor: a decode state holds the table of its generation.  Raises ValueError, naming the state, where a
        state reachable from ``start`` allows no token below ``vocab``."""
        if isinstance(vocab, bool) or not isinstance(vocab, int) or not (1 <= vocab < 2 ** 30):
            raise ValueError(f"Guide: vocab must be an integer 1 .. 2^30 - 1, got {vocab!r}")
        S, C = self.next.shape
        tc = self._classes_of(vocab)
        used = np.zeros(C, dtype=bool)
        used[tc[tc >= 0]] = True
        live = np.where(used[None, :], self.next, -1)                         # transitions a token below vocab can take
        seen = np.zeros(S, dtype=bool)
        seen[self.start] = True
        front = np.array([self.start])
        while front.size:
            rows = live[front]
            dead = front[(rows < 0).all(axis=1)]
            if dead.size:
                raise ValueError(f"Guide: state {int(dead.min())} is reachable from start = {self.start} and allows no token "
                                 f"below vocab = {vocab}")
            nxt = np.unique(rows[rows >= 0])
            front = nxt[~seen[nxt]]
            seen[front] = True
        K = class_words(vocab)
        words = HEADER_WORDS + K + S * C
        out = np.zeros(words, dtype=np.int32)
        out[:5] = (S, C, self.start, vocab, words)
        cls = np.full(2 * K, NO_CLASS, dtype=np.uint16)
        cls[:vocab] = np.where(tc >= 0, tc, NO_CLASS).astype(np.uint16)
        out[HEADER_WORDS:HEADER_WORDS + K] = cls.astype("<u2").view("<i4")
        out[HEADER_WORDS + K:] = self.next.reshape(-1).astype(np.int32)
        return torch.from_numpy(out).to(device)

    # --------------------------------------------------------------------------------------------------------------------
    @classmethod
    def choice(cls, sequences, eos_id: int) -> "Guide":
        """The text is exactly one of ``sequences`` (each 1 or more token ids) followed by ``eos_id``: the trie of the
        sequences, every end of a sequence going to a final state on ``eos_id``, which loops on ``eos_id``.  The classes are
        the distinct ids used."""
        if isinstance(eos_id, bool) or not isinstance(eos_id, int) or not (0 <= eos_id < 2 ** 31):
            raise ValueError(f"Guide: eos_id {eos_id!r} is not a token id (0 .. 2^31 - 1)")
        if isinstance(sequences, (str, bytes)) or not hasattr(sequences, "__iter__"):
            raise TypeError(f"Guide: sequences must be a list of token id lists, got {sequences!r}")
        seqs = []
        for s in sequences:
            if isinstance(s, (str, bytes)) or not hasattr(s, "__iter__"):
                raise TypeError(f"Guide: a choice must be a sequence of token ids, got {s!r}")
            s = tuple(s)
            for v in s:
                if isinstance(v, bool) or not isinstance(v, int):
                    raise TypeError(f"Guide: choice token {v!r} is not an integer token id")
                if not (0 <= v < 2 ** 31):
                    raise ValueError(f"Guide: choice token {v!r} is not a token id (0 .. 2^31 - 1)")
            if not s:
                raise ValueError("Guide: a choice holds at least one token id")
            seqs.append(s)
        if not seqs:
            raise ValueError("Guide: no sequences to choose from")
        ids = sorted({v for s in seqs for v in s} | {eos_id})
        col = {v: i for i, v in enumerate(ids)}
        rows, ends = [{}], set()                                              # state 0 is the root
        for s in seqs:
            at = 0
            for v in s:
                if col[v] not in rows[at]:
                    rows.append({})
                    rows[at][col[v]] = len(rows) - 1
                at = rows[at][col[v]]
            ends.add(at)
        final = len(rows)
        nx = np.full((final + 1, len(ids)), -1, dtype=np.int64)
        for s, row in enumerate(rows):
            for c, t in row.items():
                nx[s, c] = t
        for s in ends:
            nx[s, col[eos_id]] = final
        nx[final, col[eos_id]] = final
        tc = np.full(ids[-1] + 1, -1, dtype=np.int64)
        tc[ids] = np.arange(len(ids))
        return cls(nx, tc, 0)

    @classmethod
    def from_byte_dfa(cls, byte_next, token_bytes, start=0, device=None) -> "Guide":
        """Lift a byte-level DFA (``byte_next`` int [S, 256], -1 = dead) to the tokens of a vocabulary (``token_bytes``: the byte
        string of every id; an empty one: the token is forbidden).  A token's behaviour is the vector state -> state of running
        its bytes; tokens with the same vector share a class, tokens that are dead from every state are forbidden.  ``device``:
        None walks every token from every state on the host; a GPU device runs the lift there (``ops.guide_lift``: hashes of the
        vectors, exact vectors of one token per hash group, every token verified) and gives an equal object; a DFA beyond
        ``LIFT_MAX_STATES`` states is lifted on the host."""
        bn = _int_array(byte_next, "byte_next", 2)
        S = bn.shape[0]
        if bn.shape[1] != 256 or S < 1:
            raise ValueError(f"Guide: byte_next must be [S, 256] with S >= 1, got shape {tuple(bn.shape)}")
        if bn.min() < -1 or bn.max() >= S:
            raise ValueError(f"Guide: the entries of byte_next are -1 (dead) or a state 0..{S - 1}")
        if isinstance(token_bytes, (str, bytes)) or not hasattr(token_bytes, "__len__"):
            raise TypeError("Guide: token_bytes must be a list of bytes objects")
        for t in token_bytes:
            if not isinstance(t, (bytes, bytearray)):
                raise TypeError(f"Guide: token_bytes holds bytes objects, got {t!r}")
        T = len(token_bytes)
        lens = np.fromiter((len(t) for t in token_bytes), dtype=np.int64, count=T)
        flat = np.frombuffer(b"".join(bytes(t) for t in token_bytes), dtype=np.uint8)
        if device is not None and torch.device(device).type == "cuda" and T >= 1 and S <= LIFT_MAX_STATES and flat.size < 2 ** 31:
            return cls._lifted_on_device(bn, lens, flat, start, torch.device(device))
        offs = np.concatenate(([0], np.cumsum(lens)))[:-1]
        step = np.vstack([bn, np.full((1, 256), S, dtype=np.int64)])          # row S: the dead state, as an index
        step[step < 0] = S
        step = step.astype(np.int32)
        cur = np.broadcast_to(np.arange(S, dtype=np.int32), (T, S)).copy()
        order = np.argsort(-lens, kind="stable")                              # longest first: position p's tokens are a front slice
        sorted_lens = lens[order]
        for p in range(int(lens.max()) if T else 0):
            k = int(np.searchsorted(-sorted_lens, -p, side="left"))           # tokens with len > p
            act = order[:k]
            b = flat[offs[act] + p]
            cur[act] = step[cur[act], b[:, None]]
        cur[cur == S] = -1
        alive = (lens > 0) & (cur >= 0).any(axis=1)
        tc = np.full(T, -1, dtype=np.int64)
        if alive.any():
            vecs, inverse = np.unique(cur[alive], axis=0, return_inverse=True)
            if vecs.shape[0] > MAX_CLASSES:
                raise ValueError(f"Guide: the vocabulary has {vecs.shape[0]} distinct behaviours under this DFA, more than "
                                 f"{MAX_CLASSES} classes")
            tc[alive] = np.asarray(inverse).reshape(-1)
            nx = vecs.T.astype(np.int64)
        else:
            nx = np.full((S, 1), -1, dtype=np.int64)
        return cls(nx, tc, start)

    @classmethod
    def _lifted_on_device(cls, bn, lens, flat, start, device) -> "Guide":
        """``from_byte_dfa`` through ``ops.guide_lift``: the step table byte-major with the dead state as column S."""
        from . import ops
        S = bn.shape[0]
        step = np.full((256, S + 1), S, dtype=np.int16)
        step[:, :S] = np.where(bn < 0, S, bn).T
        offsets = np.zeros(lens.size + 1, dtype=np.int32)
        np.cumsum(lens, out=offsets[1:])
        with torch.cuda.device(device):
            tc, vecs = ops.guide_lift(torch.from_numpy(step).to(device), torch.from_numpy(flat.copy()).to(device),
                                      torch.from_numpy(offsets).to(device))
        nx = vecs.T if vecs.shape[0] else np.full((S, 1), -1, dtype=np.int64)
        return cls(nx, tc, start)

    @classmethod
    def from_regex(cls, pattern, token_bytes, eos_id: int, device=None, max_states: int = 4096) -> "Guide":
        """The text, as the bytes of its tokens, must match ``pattern`` as a whole and is then ended by ``eos_id``: the pattern
        compiled to a byte DFA (``longspec_amd.regex.compile``: the subset and its errors), lifted to the vocabulary
        (``from_byte_dfa``, on ``device`` where given) and ended as ``choice`` ends its sequences -- one more class for
        ``eos_id`` (whatever its bytes are) and one more state F, ``next[s, eos] = F`` in every accepting s, F looping on
        ``eos_id``.  Every transition into a state from which F cannot be reached over the tokens of this vocabulary is cleared,
        so no text gets stuck: a finished text always matches.  ValueError where the start is such a state."""
        from . import regex
        if isinstance(eos_id, bool) or not isinstance(eos_id, (int, np.integer)) or not (0 <= eos_id < 2 ** 31):
            raise ValueError(f"Guide: eos_id {eos_id!r} is not a token id (0 .. 2^31 - 1)")
        dfa = regex.compile(pattern, max_states=max_states)
        g = cls.from_byte_dfa(dfa.next, token_bytes, 0, device=device)
        S, C = g.next.shape
        nx = np.full((S + 1, C + 1), -1, dtype=np.int64)
        nx[:S, :C] = g.next
        nx[:S, C][dfa.accepting] = S
        nx[S, C] = S
        tc = np.full(max(g.token_class.size, int(eos_id) + 1), -1, dtype=np.int64)
        tc[:g.token_class.size] = g.token_class
        tc[eos_id] = C
        used = np.zeros(C + 1, dtype=bool)
        used[tc[tc >= 0]] = True
        live = np.where(used[None, :], nx, -1)                                # transitions some token takes
        good = np.zeros(S + 1, dtype=bool)
        good[S] = True
        while True:
            more = good | np.where(live >= 0, good[np.maximum(live, 0)], False).any(axis=1)
            if (more == good).all():
                break
            good = more
        if not good[0]:
            raise ValueError(f"Guide: the vocabulary cannot spell the language of {pattern!r}: no sequence of its tokens "
                             f"followed by eos_id = {eos_id} matches")
        nx[(nx >= 0) & ~good[np.maximum(nx, 0)]] = -1
        return cls(nx, tc, 0)

    # --------------------------------------------------------------------------------------------------------------------
    def save(self, path):
        """One ``.npz`` file holding ``next``, ``token_class`` and ``start`` (``load`` reads it; LONGSPEC_GUIDE names one)."""
        with open(path, "wb") as f:
            np.savez(f, next=self.next, token_class=self.token_class, start=np.int64(self.start))

    @classmethod
    def load(cls, path) -> "Guide":
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in ("next", "token_class", "start") if k not in z.files]
            if missing:
                raise ValueError(f"Guide: {path!r} holds no {' / '.join(missing)} (a Guide.save file has next, token_class, start)")
            return cls(z["next"], z["token_class"], int(z["start"]))


_env_cache = {}


def env_guide():
    """The process-wide default (LONGSPEC_GUIDE = the path of a ``Guide.save`` file), or None.  The file is read once per
    (path, modification time)."""
    path = os.environ.get(GUIDE_ENV, "")
    if not path:
        return None
    key = (path, os.stat(path).st_mtime_ns)
    if key not in _env_cache:
        _env_cache.clear()
        _env_cache[key] = Guide.load(path)
    return _env_cache[key]


def resolve(guide, temperature, use_env: bool):
    """The ``Guide`` a loop runs with: the argument; else, where `use_env` and no temperature is given, the default."""
    return resolve_keyword(guide, Guide, "guide", env_guide,
                           "is not available with temperature > 0, the reference's own T > 0 path; sampled decoding "
                           "under a guide is sampling= with guide=",
                           temperature, use_env)
