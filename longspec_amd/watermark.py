"""Watermarked decoding (``watermark=`` of the generate loops and the ``begin_*_decode`` entry points) and its detector.

With ``watermark`` set, every position's vocabulary is split by a keyed hash of the ``context`` tokens in front of it into a
green part (a fraction ``gamma``) and a red part, and every green id gains ``delta`` of its TARGET logit -- behind
``penalties=`` and ``dry=``, in front of the bans of ``stop=`` / ``ban=`` / ``guide=``, of the arg-max or draw and of the
log-probs.  A text decoded that way holds more green tokens than chance allows, which whoever has the key can count
(``Watermark.detect``).  The text is exactly watermarked decoding of the target, whichever loop produced it; the draft passes
are unmarked, so the mark costs acceptance length, never text.

**Definition** (a public contract: a text marked today verifies with a later build).  All arithmetic is on unsigned 64-bit
words, modulo 2^64, with ``M1 = 0x9E3779B97F4A7C15``, ``M2 = 0xBF58476D1CE4E5B9``, ``M3 = 0x94D049BB133111EB``:

* ``fin(z)``: ``z = (z ^ (z >> 30)) * M2``; ``z = (z ^ (z >> 27)) * M3``; ``z ^ (z >> 31)`` -- the SplitMix64 finaliser.
* The state of the ``h`` tokens ``c_1 .. c_h``, oldest first (int64 ids reinterpreted as uint64; ids outside the vocabulary
  take part as they are): ``s = fin(key + M1)``, then for each ``c_i``: ``s = fin((s ^ c_i) + M1)``.
* ``u(s, v) = fin(s + (v + 1) * M1)``: output ``v`` of a SplitMix64 stream seeded ``s``.
* ``v`` is green after that context iff ``(u >> 32) < T``, ``T = floor(gamma * 2^32)``.  Each id is green independently; the
  detector's null rate is ``p = T / 2^32``, not ``gamma``.

**Generation.**  For a row of target logits let ``t[0 .. m-1]`` be the row's text, exactly as for ``ban=`` and ``dry=``: the
generated columns, then the draft tokens the row follows in path order; the prompt is never part of it.  With ``m < h`` the
row keeps its bits (the prefill's token and the first ``h - 1`` steps are unmarked and never scored).  Otherwise ``s`` is the
state of ``t[m-h .. m-1]`` and every green ``v`` in ``[0, vocab)`` becomes ``dtype(float(logit[v]) + delta)``: one fp32 add,
rounded to nearest even into the 16-bit type; a NaN keeps its bits, ``-inf`` stays ``-inf``; every element that is not green
keeps its bits.  ``delta`` is in logit units, in front of ``sampling=``'s temperature.

**Detection.**  For ids ``x[0 .. n-1]`` position ``c`` is scored iff ``h <= c < n``; it is green iff ``x[c]`` is green after
``x[c-h .. c-1]``.  ``N`` scored and ``G`` green positions give ``z = (G - p N) / sqrt(p (1 - p) N)`` in float64 (NaN with
``N = 0``).  With ``unique=True`` positions with equal ``u`` count once in ``N`` and in ``G``: a loop in the text cannot
inflate ``z``.

What this is not: no fixed-size green list (the green count of a position is binomial), no self-hash scheme (the token
itself is not part of its context), not robust to paraphrase (a rewritten token breaks the ``h + 1`` positions that see it),
and the draft is unmarked.

The device side (``ops.watermark_rows`` / ``ops.watermark_score``) reads one int32 table, built once per decode state:

    [0] h   [1] T as bits   [2] delta as fp32 bits   [3] TABLE_WORDS   [4] key, low word   [5] key, high word   [6] [7] zero
"""
from __future__ import annotations

import math
import os
import struct
from types import SimpleNamespace

import numpy as np
import torch

from .keyword import resolve_keyword

WATERMARK_ENV = "LONGSPEC_WATERMARK"      # "key=81985529216486895,gamma=0.25,delta=2.0,ctx=1": the process-wide default
MAX_CONTEXT = 8                           # LS_WATERMARK_MAX_CONTEXT
TABLE_WORDS = 8                           # LS_WATERMARK_TABLE_WORDS
M1, M2, M3 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_MASK = 2 ** 64 - 1


def _i32(word: int) -> int:
    """A 32-bit pattern as the int32 that holds it."""
    return word - 2 ** 32 if word >= 2 ** 31 else word


def _fin(z):
    """``fin`` on a numpy uint64 array (array arithmetic wraps modulo 2^64)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(M2)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(M3)
    return z ^ (z >> np.uint64(31))


class Watermark:
    """``Watermark(key, gamma=0.25, delta=2.0, context=1)``: ``key`` an int in 0 .. 2^64-1; ``gamma`` the green fraction, with
    ``T = floor(gamma * 2^32)`` in 1 .. 2^32-1; ``delta`` finite and > 0, what a green id gains in logit units; ``context``
    (``h``) in 1..8, the tokens in front of a position that key its green list."""

    __slots__ = ("key", "gamma", "delta", "context")

    def __init__(self, key, gamma=0.25, delta=2.0, context=1):
        if isinstance(key, bool) or not isinstance(key, int):
            raise TypeError(f"Watermark: key must be an integer, got {key!r}")
        if not (0 <= key <= _MASK):
            raise ValueError(f"Watermark: key must be in 0 .. 2^64-1, got {key!r}")
        for v, what in ((gamma, "gamma"), (delta, "delta")):
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise TypeError(f"Watermark: {what} must be a number, got {v!r}")
        gamma, delta = float(gamma), float(delta)
        if not math.isfinite(gamma) or not (1 <= math.floor(gamma * 2 ** 32) <= 2 ** 32 - 1):
            raise ValueError(f"Watermark: gamma must give 1 <= floor(gamma * 2^32) <= 2^32-1, got {gamma!r}")
        if not math.isfinite(delta) or not delta > 0:
            raise ValueError(f"Watermark: delta must be finite and > 0, got {delta!r}")
        try:
            struct.pack("<f", delta)
        except OverflowError:
            raise ValueError(f"Watermark: delta must be an fp32 value, got {delta!r}") from None
        if isinstance(context, bool) or not isinstance(context, int):
            raise TypeError(f"Watermark: context must be an integer, got {context!r}")
        if not (1 <= context <= MAX_CONTEXT):
            raise ValueError(f"Watermark: context must be 1..{MAX_CONTEXT}, got {context!r}")
        self.key, self.gamma, self.delta, self.context = key, gamma, delta, context

    def __repr__(self):
        return f"Watermark(key={self.key:#x}, gamma={self.gamma}, delta={self.delta}, context={self.context})"

    def _key(self):
        return (self.key, self.gamma, self.delta, self.context)

    def __eq__(self, other):
        return isinstance(other, Watermark) and self._key() == other._key()

    def __hash__(self):
        return hash(("Watermark",) + self._key())

    @property
    def threshold(self) -> int:
        """``T = floor(gamma * 2^32)``."""
        return math.floor(self.gamma * 2 ** 32)

    @property
    def rate(self) -> float:
        """The detector's null rate ``p = T / 2^32``."""
        return self.threshold / 2 ** 32

    def table(self, vocab: int, device):
        """A new int32 [TABLE_WORDS] table of this object on `device` (layout: the module's docstring).  The object keeps no
        tensor: a decode state holds the table of its generation.  ``vocab`` takes no part: ids are hashed as they are."""
        delta_bits = struct.unpack("<I", struct.pack("<f", self.delta))[0]
        words = [self.context, _i32(self.threshold), _i32(delta_bits), TABLE_WORDS, _i32(self.key & 0xffffffff), _i32(self.key >> 32),
                 0, 0]
        assert len(words) == TABLE_WORDS
        return torch.tensor(words, dtype=torch.int32).to(device)

    def _score_cpu(self, x, lengths):
        """(flags int8 [b, n], hashes uint64 [b, n] as numpy arrays) of int64 [b, n] ids on the CPU: the definition, vectorised
        over the positions."""
        b, n = x.shape
        h = self.context
        ids = x.numpy().astype(np.int64).view(np.uint64).reshape(b, n)
        flags = np.full((b, n), -1, dtype=np.int8)
        hashes = np.zeros((b, n), dtype=np.uint64)
        if n > h:
            s0 = (self.key + M1) & _MASK
            s = _fin(np.full((b, n - h), s0, dtype=np.uint64))
            for i in range(h, 0, -1):                                      # position c folds ids[c - h], ..., ids[c - 1]
                s = _fin((s ^ ids[:, h - i:n - i]) + np.uint64(M1))
            u = _fin(s + (ids[:, h:] + np.uint64(1)) * np.uint64(M1))
            live = np.arange(h, n)[None, :] < lengths[:, None]
            flags[:, h:] = np.where(live, ((u >> np.uint64(32)) < np.uint64(self.threshold)).astype(np.int8), np.int8(-1))
            hashes[:, h:] = np.where(live, u, np.uint64(0))
        return flags, hashes

    def detect(self, ids, lengths=None, unique=False):
        """Score token ids against this watermark: ``ids`` int64 [n] or [b, n] (``[n]`` is one row), ``lengths`` int [b] or None
        (row z is ``ids[z, :lengths[z]]``, clamped to 0..n).  Returns a namespace of ``scored`` and ``green`` (int32 [b]),
        ``z`` (float64 [b]; NaN where nothing is scored) and ``flags`` (int8 [b, n]: -1 not scored, 0 red, 1 green), on the
        device of ``ids``.  With ``unique`` positions with equal ``u`` count once in ``scored`` and ``green``.  A GPU tensor is
        scored by one launch (``ops.watermark_score``), a CPU tensor by a vectorised restatement of the definition."""
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.dim() not in (1, 2):
            raise TypeError("Watermark.detect: ids must be an int64 [n] or [b, n] tensor")
        x = ids if ids.dim() == 2 else ids.unsqueeze(0)
        b, n = x.shape
        if lengths is not None:
            lengths = torch.as_tensor(lengths)
            if lengths.dtype not in (torch.int32, torch.int64) or lengths.numel() != b or lengths.dim() > 1:
                raise TypeError("Watermark.detect: lengths must be b integers")
            lengths = lengths.reshape(b).clamp(0, n).to(device=x.device, dtype=torch.int32)
        if x.is_cuda:
            from . import ops
            got = ops.watermark_score(x, self.table(0, x.device), lengths, want_flags=True, want_hashes=unique)
            scored, green, flags = got.counts[:, 0].contiguous(), got.counts[:, 1].contiguous(), got.flags
            hashes = got.hashes.view(torch.int64) if unique else None      # (a bijection: equal stays equal)
        else:
            lens = np.full((b,), n, dtype=np.int64) if lengths is None else lengths.numpy().astype(np.int64)
            f, hs = self._score_cpu(x.contiguous(), lens)
            flags = torch.from_numpy(f)
            hashes = torch.from_numpy(hs.view(np.int64)) if unique else None
            scored, green = (flags >= 0).sum(dim=1).to(torch.int32), (flags == 1).sum(dim=1).to(torch.int32)
        if unique:
            count = lambda z, sel: int(torch.unique(hashes[z][sel[z]]).numel())
            scored = torch.tensor([count(z, flags >= 0) for z in range(b)], dtype=torch.int32, device=x.device)
            green = torch.tensor([count(z, flags == 1) for z in range(b)], dtype=torch.int32, device=x.device)
        p = self.rate
        N, G = scored.to(torch.float64), green.to(torch.float64)
        z = (G - p * N) / torch.sqrt(p * (1.0 - p) * N)                    # N = 0: 0 / 0 = NaN
        return SimpleNamespace(scored=scored, green=green, z=z, flags=flags)

    @classmethod
    def parse(cls, text: str) -> "Watermark":
        """``"key=<int>,gamma=0.25,delta=2.0,ctx=1"`` (``key`` required -- decimal or 0x.. --, the others optional, any order)."""
        form = f"{WATERMARK_ENV}={text!r}: expected key=<int>[,gamma=<float>][,delta=<float>][,ctx=<int>]"
        names = {"key": ("key", lambda v: int(v, 0)), "gamma": ("gamma", float), "delta": ("delta", float), "ctx": ("context", int)}
        kw = {}
        for part in text.split(","):
            key, sep, val = part.strip().partition("=")
            key = key.strip()
            if not sep or key not in names or names[key][0] in kw:
                raise ValueError(form)
            name, conv = names[key]
            try:
                kw[name] = conv(val.strip())
            except ValueError:
                raise ValueError(f"{form}; {val!r} does not read as the value of {key}") from None
        if "key" not in kw:
            raise ValueError(form)
        return cls(**kw)


def env_watermark():
    """The process-wide default (LONGSPEC_WATERMARK), or None."""
    text = os.environ.get(WATERMARK_ENV, "")
    return Watermark.parse(text) if text else None


def resolve(watermark, temperature, use_env: bool):
    """The ``Watermark`` a loop runs with: the argument; else, where `use_env` and no temperature is given, the default."""
    return resolve_keyword(watermark, Watermark, "watermark", env_watermark,
                           "is not available with temperature > 0, the reference's own T > 0 path; sampled decoding "
                           "with a watermark is sampling= with watermark=",
                           temperature, use_env)
