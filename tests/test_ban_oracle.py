"""The oracle of ``ops.ban_rows`` (tests/ban_oracle.py) against a brute-force enumeration of the forbidden ids, and the ``Ban``
object: validation, ``parse``, the table and its limits.  No GPU."""
import random

import pytest
import torch

import ban_oracle as bo
from longspec_amd import Ban
from longspec_amd import ban as ban_mod


def brute(text, ban, V):
    """Try every id: v is forbidden when text + [v] ends in a listed sequence, or ends in an n-gram it already holds."""
    out = set()
    n = ban.no_repeat_ngram
    for v in range(V):
        t = list(text) + [v]
        if any(len(s) <= len(t) and t[len(t) - len(s):] == list(s) for s in ban.sequences):
            out.add(v)
        elif n >= 1 and len(t) >= n:
            last = t[len(t) - n:]
            if any(t[e - n:e] == last for e in range(n, len(t))):
                out.add(v)
    return out


def test_the_oracle_is_the_brute_force_enumeration_on_dense_small_texts():
    rng = random.Random(11)
    V, hits = 16, 0
    for m in range(0, 13):
        for n in range(0, 6):
            for trial in range(12):
                text = [rng.randrange(4 if trial % 2 else V) for _ in range(m)]
                seqs = [[rng.randrange(4) for _ in range(rng.randrange(1, 5))] for _ in range(rng.randrange(0, 4))]
                if text and trial % 3 == 0:                              # a sequence whose front is the end of the text
                    k = rng.randrange(0, min(3, m) + 1)
                    seqs.append(text[m - k:] + [rng.randrange(V)])
                if n == 0 and not seqs:
                    seqs = [[3]]
                ban = Ban(seqs, n)
                want = brute(text, ban, V)
                assert bo.forbidden(text, ban) == want, (text, ban)
                hits += bool(want)
                # ... and through the operator: a table round trip and -inf exactly there
                x = torch.zeros((1, V), dtype=torch.float16)
                out = torch.tensor([text + [0]], dtype=torch.int64)
                bo.ban_rows(x, ban.table(V, "cpu"), out, base=torch.tensor([m], dtype=torch.int32))
                assert set(torch.isinf(x[0]).nonzero().view(-1).tolist()) == want
    assert hits > 400                                                     # repeats abound


def test_the_operator_splits_a_text_between_columns_and_path_in_column_order():
    ban = Ban(no_repeat_ngram=3, sequences=[[7, 8, 9]])
    V = 12
    text = [1, 2, 3, 4, 1, 2]                                             # next 3 is forbidden; [.., 7, 8] forbids 9
    for w in range(0, len(text) + 1):
        out = torch.tensor([text[:w] + [11] * 3], dtype=torch.int64)     # (columns at and behind w are never read)
        rest = text[w:]
        C = len(rest) + 2
        ids = torch.full((1, C), 5, dtype=torch.int64)
        mask = torch.zeros((2, C), dtype=torch.int64)
        cols = sorted(random.Random(w).sample(range(C), len(rest)))
        for c, t in zip(cols, rest):
            ids[0, c], mask[0, c] = t, 1
        mask[1] = 1                                                       # row 1 follows every column: another text
        x = torch.zeros((1, 2, V), dtype=torch.bfloat16)
        bo.ban_rows(x, ban.table(V, "cpu"), out, base=torch.tensor([w + 2], dtype=torch.int32), base_add=-2, extra_ids=ids,
                    extra_mask=mask)
        assert torch.isinf(x[0, 0]).nonzero().view(-1).tolist() == [3], w
        want1 = bo.forbidden(text[:w] + ids[0].tolist(), ban)
        assert set(torch.isinf(x[0, 1]).nonzero().view(-1).tolist()) == {t for t in want1 if t < V}


def test_ids_outside_the_vocabulary_compare_and_are_never_written():
    ban = Ban(no_repeat_ngram=2, sequences=[[40, 2], [3, 99]])
    V = 8
    out = torch.tensor([[-1, 5, 40, -1, 99, 40]], dtype=torch.int64)
    x = torch.zeros((1, V), dtype=torch.float16)
    bo.ban_rows(x, ban.table(V, "cpu"), out, base=torch.tensor([6], dtype=torch.int32))
    assert bo.forbidden(out[0].tolist(), ban) == {2, -1}                   # after 40: the bigram's -1 and the sequence's 2
    assert torch.isinf(x[0]).nonzero().view(-1).tolist() == [2]


def test_validation():
    for bad in (dict(), dict(sequences=[[]]), dict(sequences=[[1] * 17]), dict(sequences=[[-1]]), dict(sequences=[[2 ** 31]]),
                dict(no_repeat_ngram=17), dict(no_repeat_ngram=-1), dict(sequences=[[1]] * 65)):
        with pytest.raises(ValueError, match="Ban"):
            Ban(**bad)
    for bad in (dict(sequences="12"), dict(sequences=[3]), dict(sequences=[[1.0]]), dict(sequences=[[True]]),
                dict(no_repeat_ngram=2.0), dict(no_repeat_ngram=True), dict(sequences=5)):
        with pytest.raises(TypeError, match="Ban"):
            Ban(**bad)
    a = Ban([[1, 2], (3,)], 4)
    assert a == Ban(((1, 2), (3,)), 4) and hash(a) == hash(Ban([[1, 2], [3]], 4)) and a != Ban([[1, 2], [3]], 3) and a != "x"
    assert repr(a) == "Ban(sequences=((1, 2), (3,)), no_repeat_ngram=4)"
    assert Ban(no_repeat_ngram=16).no_repeat_ngram == 16 and len(Ban([[1] * 16] * 64).sequences) == 64


def test_parse_round_trip_and_refusals(monkeypatch):
    for ban in (Ban([[13, 13], [198, 198, 198]], 4), Ban(no_repeat_ngram=1), Ban([[5]]), Ban([[1] * 16] * 64, 16)):
        assert Ban.parse(bo.spec_of(ban)) == ban
    assert Ban.parse("seq=13+13|198+198+198,ngram=4") == Ban([[13, 13], [198, 198, 198]], 4)
    assert Ban.parse(" ngram=2 , seq=7 ") == Ban([[7]], 2)
    for bad in ("", "ngram", "ngram=2,ngram=3", "seq=1+x", "ids=3", "ngram=1+2", "seq=", "ngram=17", "seq=1,min=2"):
        with pytest.raises(ValueError):
            Ban.parse(bad)
    monkeypatch.delenv(ban_mod.BAN_ENV, raising=False)
    assert ban_mod.env_ban() is None and ban_mod.resolve(None, None, True) is None
    monkeypatch.setenv(ban_mod.BAN_ENV, "seq=13+13,ngram=3")
    want = Ban([[13, 13]], 3)
    assert ban_mod.env_ban() == want and ban_mod.resolve(None, None, True) == want and ban_mod.resolve(None, 0.0, True) == want
    assert ban_mod.resolve(None, 0.5, True) is None and ban_mod.resolve(None, None, False) is None
    assert ban_mod.resolve(Ban([[1]]), None, True) == Ban([[1]])
    with pytest.raises(ValueError, match="temperature"):
        ban_mod.resolve(want, 0.5, True)
    with pytest.raises(TypeError, match="longspec_amd.Ban"):
        ban_mod.resolve([[1]], None, True)


def test_table_round_trip_and_limits():
    full = Ban([[q + 1] * 16 for q in range(64)], 16)
    for ban in (Ban([[13, 13], [198]], 4), Ban(no_repeat_ngram=2), full, Ban([[2 ** 31 - 1, 7]])):
        t = ban.table(8, "cpu")                                          # an id >= vocab is legal
        assert t.dtype == torch.int32 and tuple(t.shape) == (ban_mod.TABLE_WORDS,) == (1093,)
        assert int(t[0]) == len(ban.sequences) and int(t[1]) == ban.no_repeat_ngram and int(t[3]) == ban_mod.TABLE_WORDS
        assert bo.ban_of_table(t) == ban
    t = full.table(8, "cpu").tolist()
    assert t[ban_mod.OFFS_OFF:ban_mod.TOKS_OFF] == [16 * q for q in range(65)] and t[-1] == 64 and -1 not in t[ban_mod.TOKS_OFF:]
    assert Ban([[5]]).table(8, "cpu").tolist()[ban_mod.TOKS_OFF:ban_mod.TOKS_OFF + 2] == [5, -1]
