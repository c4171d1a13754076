"""The DRY oracle (tests/dry_oracle.py) against hand-worked texts, ``Dry``'s refusals, the environment form and the table's
layout against the header's constants.  No GPU."""
import math
import os
import re
import struct

import pytest
import torch

import dry_oracle as do
from longspec_amd import Dry
from longspec_amd import dry as dry_mod

A, B, C, D, X = 10, 11, 12, 13, 99
V = 128


def penalised(text, dry, dtype=torch.float16, fill=1.0, **kw):
    """{v: the fp32 amount row 0 lost at v} for a one-row call with the committed text ``text``."""
    x = torch.full((1, V), fill, dtype=dtype)
    out = torch.tensor([list(text) + [0, 0]], dtype=torch.int64)
    got = do.dry_rows(x, dry.table(V, "cpu"), out, base=torch.tensor([len(text)], dtype=torch.int32), **kw)
    assert got is x
    return {v: fill - float(x[0, v]) for v in range(V) if float(x[0, v]) != fill}


def test_a_b_c_a_b_penalises_c_by_the_multiplier():
    dry = Dry(0.5)                                                        # allowed_length 2: a match of 2 costs multiplier * base^0
    assert do.match_lengths([A, B, C, A, B]) == {C: 2}
    assert penalised([A, B, C, A, B], dry) == {C: 0.5}
    assert penalised([A, B, C, A], dry) == {}                             # a match of 1 is below allowed_length
    assert penalised([A, B, C, A], Dry(0.5, allowed_length=1)) == {B: 0.5}
    assert penalised([A, B, C, D, A, B, C], Dry(0.5, base=2.0)) == {D: 1.0}
    assert penalised([], dry) == {} and penalised([A], dry) == {} and penalised([A, A], Dry(0.5, allowed_length=1)) == {A: 0.5}


def test_a_a_a_a():
    # j = 0, 1, 2 match to depth 1, 2, 3 (j - k >= 0 stops them) and all have the candidate a: the maximum counts
    assert do.match_lengths([A, A, A, A]) == {A: 3}
    assert penalised([A, A, A, A], Dry(0.25, base=2.0)) == {A: 0.5}
    assert penalised([A, A, A, A], Dry(0.25, base=2.0, allowed_length=4)) == {}


def test_the_maximum_over_positions_and_two_candidates():
    t = [B, A, C, 98, X, B, A, D, X, B, A]                                 # "b a" -> c (depth 2), "x b a" -> d (depth 3)
    assert do.match_lengths(t) == {C: 2, D: 3}
    assert penalised(t, Dry(1.0, base=2.0)) == {C: 1.0, D: 2.0}
    t = [A, B, C, X, A, B, C, X, A, B]                                    # c at depth 2 (j = 1) and at depth 6 (j = 5): the maximum counts
    assert do.match_lengths(t) == {C: 6} and penalised(t, Dry(1.0, base=2.0), fill=32.0) == {C: 16.0}


def test_a_breaker_inside_a_match():
    t = [A, X, B, C, A, X, B]                                             # without breakers: depth 3 -> c
    assert do.match_lengths(t) == {C: 3}
    assert do.match_lengths(t, breakers={X}) == {C: 1}                    # the match stops in front of the breaker
    assert penalised(t, Dry(1.0, base=2.0, breakers=[X])) == {}
    assert penalised(t, Dry(1.0, base=2.0, breakers=[X], allowed_length=1)) == {C: 1.0}
    assert do.match_lengths([A, B, X, A, B, X], breakers={X}) == {}       # the last token is a breaker: nothing
    assert do.match_lengths([A, B, X, A, B, X]) == {A: 3}


def test_last_n_cuts_a_match():
    t = [A, B, C, D, A, B, C]
    assert do.match_lengths(t) == {D: 3}
    assert do.match_lengths(t, last_n=6) == {D: 2}                        # lo = 1: the match may not reach column 0
    assert do.match_lengths(t, last_n=5) == {D: 1}
    assert do.match_lengths(t, last_n=4) == {} and do.match_lengths(t, last_n=1) == {}
    assert penalised(t, Dry(1.0, base=2.0, last_n=6)) == {D: 1.0} and penalised(t, Dry(1.0, base=2.0)) == {D: 2.0}


def test_saturation_at_32():
    assert do.match_lengths([A] * 33) == {A: 32} and do.match_lengths([A] * 200) == {A: 32}
    unit = list(range(40))
    assert do.match_lengths(unit + [X] + unit[:39]) == {39: 32}
    dry = Dry(1.0, base=1.0625, allowed_length=2)
    want = struct.unpack("<f", struct.pack("<f", 1.0625 ** 30))[0]
    got = penalised([A] * 200, dry, dtype=torch.bfloat16, fill=64.0)
    assert got == {A: 64.0 - float((torch.tensor(64.0) - torch.tensor(want)).to(torch.bfloat16))}
    assert dry.penalties()[32] == want and dry.penalties()[2] == 1.0
    # the default base: far beyond any 16-bit logit
    assert Dry(0.8).penalties()[32] > 1e7 * 0.8
    x = torch.full((1, V), 3.0, dtype=torch.float16)
    do.dry_rows(x, Dry(0.8).table(V, "cpu"), torch.tensor([[A] * 40]), base=torch.tensor([40], dtype=torch.int32))
    assert x[0, A] == -math.inf and int((x != 3.0).sum()) == 1


def test_ids_outside_the_vocabulary_match_and_are_never_penalised_and_infinities_stay():
    t = [V + 3, -1, 5, V + 3, -1]
    assert do.match_lengths(t) == {5: 2}
    assert penalised(t, Dry(1.0)) == {5: 1.0}
    assert penalised([5, V, 5], Dry(1.0, allowed_length=1)) == {}         # the candidate is outside: nothing
    x = torch.tensor([[-math.inf, math.inf, math.nan, 1.0]], dtype=torch.float16)
    bits = x.view(torch.int16).clone()
    do.dry_rows(x, Dry(1.0, allowed_length=1).table(4, "cpu"), torch.tensor([[0, 0, 1, 0, 2, 0, 3, 0]]),
                base=torch.tensor([8], dtype=torch.int32))
    assert x.view(torch.int16)[0, :3].tolist() == bits[0, :3].tolist() and float(x[0, 3]) == 0.0


def test_paths_follow_the_text_in_column_order():
    dry = Dry(1.0, base=2.0)
    x = torch.zeros((1, 3, V), dtype=torch.float16)
    out = torch.tensor([[A, B, C, A, 0, 0]])
    ids = torch.tensor([[B, C]])
    mask = torch.tensor([[0, 0], [1, 0], [1, 1]])
    do.dry_rows(x, dry.table(V, "cpu"), out, base=torch.tensor([4], dtype=torch.int32), extra_ids=ids, extra_mask=mask)
    assert x[0, 0].abs().sum() == 0                                       # "a b c a": depth 1
    assert x[0, 1].nonzero().view(-1).tolist() == [C] and float(x[0, 1, C]) == -1.0           # "a b c a b" -> c
    assert x[0, 2].nonzero().view(-1).tolist() == [A] and float(x[0, 2, A]) == -2.0           # "a b c a b c" -> a, depth 3


def test_refusals():
    for bad in (dict(multiplier=0.0), dict(multiplier=-1.0), dict(multiplier=math.inf), dict(multiplier=math.nan),
                dict(base=0.99), dict(base=4.01), dict(base=math.nan), dict(allowed_length=0), dict(allowed_length=33),
                dict(breakers=[3, 3]), dict(breakers=[-1]), dict(breakers=[2 ** 31]), dict(breakers=list(range(65))),
                dict(last_n=-1), dict(last_n=2 ** 23 + 1)):
        kw = dict(multiplier=0.8)
        kw.update(bad)
        with pytest.raises(ValueError, match="Dry"):
            Dry(**kw)
    for bad in (dict(multiplier="0.8"), dict(multiplier=True), dict(base=None), dict(allowed_length=2.0), dict(breakers="13"),
                dict(breakers=7), dict(breakers=[1.5]), dict(last_n=1.0), dict(last_n=False)):
        kw = dict(multiplier=0.8)
        kw.update(bad)
        with pytest.raises(TypeError, match="Dry"):
            Dry(**kw)
    ok = Dry(0.8, 1.0, 32, range(64), 2 ** 23)
    assert ok == Dry(0.8, 1.0, 32, tuple(range(64)), 2 ** 23) and hash(ok) == hash(Dry(0.8, 1.0, 32, range(64), 2 ** 23))
    assert Dry(1) == Dry(1.0) and Dry(0.8) != Dry(0.8, last_n=5) and "multiplier=0.8" in repr(Dry(0.8))
    assert Dry(4, 4).base == 4.0 and dry_mod.MAX_MATCH == 32


def test_the_environment_form(monkeypatch):
    from longspec_amd.dry import DRY_ENV, env_dry, resolve
    monkeypatch.delenv(DRY_ENV, raising=False)
    assert env_dry() is None and resolve(None, None, True) is None
    monkeypatch.setenv(DRY_ENV, "mult=0.8,base=1.75,allow=2,last=0,break=13+198")
    want = Dry(0.8, 1.75, 2, (13, 198), 0)
    assert env_dry() == want and resolve(None, None, True) == want and resolve(None, 0.0, True) == want
    assert resolve(None, 0.5, True) is None and resolve(None, None, False) is None
    mine = Dry(0.3)
    assert resolve(mine, None, True) is mine
    with pytest.raises(ValueError, match="temperature"):
        resolve(mine, 0.5, True)
    with pytest.raises(TypeError, match="longspec_amd.Dry"):
        resolve("mult=0.8", None, True)
    assert Dry.parse("mult=2") == Dry(2.0) and Dry.parse(" last=7 , mult=1e-1 ") == Dry(0.1, last_n=7)
    for dry in (want, Dry(0.1, 1.0, 7, (), 100), Dry(3.0, 4.0, 32, range(64))):
        assert Dry.parse(do.spec_of(dry)) == dry
    for bad in ("", "base=2", "mult=0.8,mult=0.9", "mult=0.8,foo=1", "mult", "mult=x", "mult=0.8,allow=2.5", "mult=0.8,break=1+a",
                "mult=0.8,break="):
        with pytest.raises(ValueError, match=DRY_ENV):
            Dry.parse(bad)
    with pytest.raises(ValueError, match="Dry"):
        Dry.parse("mult=0.8,base=9")


def test_the_table_layout_and_the_header_constants():
    here = os.path.dirname(os.path.abspath(__file__))
    txt = open(os.path.join(os.path.dirname(here), "include", "longspec_hip.h")).read()
    macro = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
    assert macro("LS_DRY_MAX_MATCH") == dry_mod.MAX_MATCH == 32
    assert macro("LS_DRY_TABLE_WORDS") == dry_mod.TABLE_WORDS == 4 + 33 + 64
    dry = Dry(0.8, 1.75, 3, (13, 198, 2 ** 31 - 1), 4096)
    t = dry.table(1000, "cpu")
    assert t.dtype == torch.int32 and tuple(t.shape) == (dry_mod.TABLE_WORDS,)
    assert t[:4].tolist() == [3, 3, 4096, dry_mod.TABLE_WORDS]
    pen = t[dry_mod.PEN_OFF:dry_mod.BREAK_OFF].view(torch.float32)
    for L in range(33):                                                   # float64, then ONE rounding to fp32
        assert float(pen[L]) == float(torch.tensor(0.8 * 1.75 ** (L - 3), dtype=torch.float64).to(torch.float32)), L
    assert t[dry_mod.BREAK_OFF:dry_mod.BREAK_OFF + 3].tolist() == [13, 198, 2 ** 31 - 1] and (t[dry_mod.BREAK_OFF + 3:] == -1).all()
    p = do.params_of_table(t)
    assert (p.allowed_length, p.last_n, p.breakers) == (3, 4096, {13, 198, 2 ** 31 - 1}) and p.pen == dry.penalties()
    # beyond fp32: the largest fp32, never an infinity
    big = Dry(1e300, 4.0).table(8, "cpu")[dry_mod.PEN_OFF:dry_mod.BREAK_OFF].view(torch.float32)
    assert torch.isfinite(big).all() and float(big[32]) == dry_mod.FP32_MAX and float(big[2]) == dry_mod.FP32_MAX
    tiny = Dry(1e-300, 4.0).table(8, "cpu")[dry_mod.PEN_OFF:dry_mod.BREAK_OFF].view(torch.float32)
    assert float(tiny[0]) == 0.0 and torch.isfinite(tiny).all()
