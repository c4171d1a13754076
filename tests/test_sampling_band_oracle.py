"""tests/sampling_band_oracle.py on rows small enough to work out by hand, and the ``Sampling`` object's two new fields.

The row used throughout has probabilities q = (1/2, 1/4, 1/8, 1/16, 1/64, 1/64, 1/64, 1/64) at T = 1 (x = ln q):
  surprise in bits  (1, 2, 3, 4, 6, 6, 6, 6), entropy 1/2 + 2/4 + 3/8 + 4/16 + 4 * 6/64 = 2 bits,
  distance in bits  (1, 0, 1, 2, 4, 4, 4, 4): by distance token 1 (mass 1/4), tokens 0 and 2 (7/8 with them), token 3 (15/16),
  then the four equal logits (1)."""
import math

import numpy as np
import pytest

import sampling_band_oracle as sbo
import sampling_oracle as so
from longspec_amd import Sampling

Q = np.array([1 / 2, 1 / 4, 1 / 8, 1 / 16, 1 / 64, 1 / 64, 1 / 64, 1 / 64])
X = np.log(Q)


def _kept(x, **kw):
    lo, hi = sbo.band(np.asarray(x, dtype=np.float64), kw.pop("T", 1.0), **kw)
    return [j for j in range(len(x)) if lo <= x[j] <= hi], lo, hi


def test_each_filter_on_the_hand_computed_row():
    assert _kept(X)[0] == list(range(8))
    assert _kept(X, top_k=3)[0] == [0, 1, 2]
    assert _kept(X, top_k=5)[0] == list(range(8))                    # the 5th value occurs four times: ties are kept
    assert _kept(X, top_p=0.8)[0] == [0, 1, 2]                       # 1/2, 3/4, 7/8 >= 0.8
    # min_p: w = q / q_max = (1, 1/2, 1/4, 1/8, 1/32, ...)
    assert _kept(X, min_p=0.1)[0] == [0, 1, 2, 3]
    assert _kept(X, min_p=0.2)[0] == [0, 1, 2]
    assert _kept(X, min_p=0.6)[0] == [0]
    # typical_p: see the module docstring
    kept, lo, hi = _kept(X, typical_p=0.2)
    assert kept == [1] and lo == hi == X[1]                          # the maximum is dropped
    assert _kept(X, typical_p=0.9)[0] == [0, 1, 2, 3]                # 7/8 < 0.9 <= 15/16
    assert _kept(X, typical_p=0.95)[0] == list(range(8))             # d* is the distance of a value that occurs four times


def test_the_chain_top_k_top_p_min_p_typical_p():
    # top_k = 4: {0..3}, mass 15/16.  top_p = 0.9 of it: 8/15, 12/15, 14/15 >= 0.9: {0, 1, 2}.  min_p = 0.2: w_2 = 1/4 stays.
    # typical_p = 0.5 on q = (4/7, 2/7, 1/7): s = (0.5596, 1.2528, 1.9459), H = 0.9557, d = (0.396, 0.297, 0.990):
    # token 1 (2/7 < 0.5), then token 0 (6/7): {0, 1}.
    kept, lo, hi = _kept(X, top_k=4, top_p=0.9, min_p=0.2, typical_p=0.5)
    assert kept == [0, 1] and (lo, hi) == (X[1], X[0])
    # each filter runs on what the former kept: typical_p = 0.5 on the whole row takes token 1, then a tie of 0 and 2
    s = [4 / 7, 2 / 7, 1 / 7]
    H = -sum(q * math.log(q) for q in s)
    assert [round(abs(-math.log(q) - H), 3) for q in s] == [0.396, 0.297, 0.99]
    # min_p alone after top_k: top_k = 2 leaves {0, 1}, min_p = 0.6 then only the maximum
    assert _kept(X, top_k=2, min_p=0.6)[0] == [0]


def test_a_peaked_row_can_lose_its_maximum_and_a_dominant_one_keeps_it():
    row = sbo.sample_row(X, 5, 0, 1, 1.0, typical_p=0.2)
    assert row[0] == 1 and row[1][0] == (1, -1) and row[2] == 1 and row[3] == row[4] == X[1]
    dom = np.log(np.array([0.9] + [0.1 / 7] * 7))                    # s = (0.105, 4.25 x 7), H = 0.52: the maximum is closest
    kept, lo, hi = _kept(dom, typical_p=0.5)
    assert kept == [0]
    assert _kept(dom, typical_p=0.95)[0] == list(range(8))


def test_a_flat_row_keeps_everything():
    flat = np.full(8, 1.25)
    for tp in (0.01, 0.5, 1.0):
        assert _kept(flat, typical_p=tp, T=0.7)[0] == list(range(8))
    assert _kept(flat, min_p=1.0)[0] == list(range(8))


def test_ties_at_d_star_are_all_kept():
    # the four 1/64 logits share one distance: with typical_p just above 15/16 all four come in, and the count says so
    row = sbo.sample_row(X, 0, 0, 0, 1.0, typical_p=0.94)
    assert row[2] == 8 and row[3] == X[7] and row[4] == X[0]
    x = X.copy()
    x[2] = x[1]                                                       # the closest value twice
    kept, lo, hi = _kept(x, typical_p=0.01)
    assert lo == hi and len(kept) == 2


def test_one_finite_logit_and_none():
    x = np.full(8, -np.inf)
    x[5] = 1.5
    for kw in (dict(min_p=0.3), dict(typical_p=0.4), dict(top_k=3, top_p=0.5, min_p=0.3, typical_p=0.4)):
        row = sbo.sample_row(x, 9, 2, 4, 0.8, **kw)
        assert (row[0], row[1][0], row[2], row[3], row[4]) == (5, (5, -1), 1, 1.5, 1.5)
        none = sbo.sample_row(np.full(8, -np.inf), 9, 2, 4, 0.8, **kw)
        assert (none[0], none[1][0], none[2]) == (0, (0, 1), 8) and none[3] == none[4] == -np.inf
    # a -inf logit belongs to no set while the row has a finite one
    x[1] = 0.5
    assert sbo.sample_row(x, 9, 2, 4, 0.8, typical_p=0.999)[2] == 2


@pytest.mark.parametrize("T", [0.3, 1.0, 1.7])
def test_min_p_1_keeps_exactly_the_maxima(T):
    rng = np.random.default_rng(3)
    x = np.float16(rng.standard_normal(64) * 3).astype(np.float64)
    x[[7, 40]] = x.max()
    row = sbo.sample_row(x, 1, 0, 2, T, min_p=1.0)
    assert row[2] == 3 and row[3] == row[4] == x.max()


def test_filters_off_is_the_sampling_oracle():
    rng = np.random.default_rng(11)
    for i in range(20):
        x = np.float16(rng.standard_normal(96) * 3).astype(np.float64)
        x[rng.integers(0, 96, 6)] = -np.inf
        k, p = ((0, 1.0), (10, 1.0), (0, 0.9), (20, 0.8))[i % 4]
        a = so.sample_row(x, 100 + i, i % 3, 77, 0.9, k, p)
        b = sbo.sample_row(x, 100 + i, i % 3, 77, 0.9, k, p)
        assert (b[0], b[1][0], b[1][1], b[2], b[3]) == (a[0], a[1], a[2], a[3], a[4])
        assert b[4] == x.max()


def test_typical_set_is_a_contiguous_run_with_enough_mass():
    rng = np.random.default_rng(5)
    for i in range(30):
        x = np.float16(rng.standard_normal(200) * (1 + i % 4)).astype(np.float64)
        T, tp = (0.3, 1.0, 1.7)[i % 3], (0.2, 0.5, 0.9, 0.99)[i % 4]
        lo, hi = sbo.band(x, T, typical_p=tp)
        w = np.exp((x - x.max()) / T)
        assert w[(x >= lo) & (x <= hi)].sum() / w.sum() >= tp - 1e-12
        v, n = np.unique(x, return_counts=True)
        Z, H, d = sbo.typical_distances(v, n, x.max(), T)
        inside = (v >= lo) & (v <= hi)
        assert d[inside].max() < d[~inside].min() if (~inside).any() else True


# ---- Sampling ------------------------------------------------------------------------------------------------------------------

def test_sampling_takes_and_validates_the_new_fields():
    s = Sampling(0.8, min_p=0.1)
    assert (s.min_p, s.typical_p) == (0.1, 1.0)
    s = Sampling(0.6, 40, 0.95, 1, 0.05, 0.9)
    assert (s.temperature, s.top_k, s.top_p, s.seed, s.min_p, s.typical_p) == (0.6, 40, 0.95, 1, 0.05, 0.9)
    assert Sampling(1, min_p=0, typical_p=1) == Sampling(1.0)
    assert Sampling(1, min_p=1.0).min_p == 1.0
    for bad in (dict(min_p=-0.1), dict(min_p=1.01), dict(min_p=float("nan")), dict(typical_p=0), dict(typical_p=-1),
                dict(typical_p=1.01), dict(typical_p=float("nan"))):
        with pytest.raises(ValueError):
            Sampling(1.0, **bad)
    assert "min_p=0.05" in repr(s) and "typical_p=0.9" in repr(s)
    assert set(Sampling.__slots__) == {"temperature", "top_k", "top_p", "seed", "min_p", "typical_p"}


def test_old_positional_construction_is_unchanged():
    s = Sampling(0.6, 40, 0.95, 7)
    assert (s.temperature, s.top_k, s.top_p, s.seed, s.min_p, s.typical_p) == (0.6, 40, 0.95, 7, 0.0, 1.0)


def test_equality_and_hash_see_the_new_fields():
    a, b, c = Sampling(0.7, min_p=0.05), Sampling(0.7, min_p=0.06), Sampling(0.7, typical_p=0.9)
    assert a != b and a != c and a != Sampling(0.7) and c != Sampling(0.7)
    assert a == Sampling(0.7, min_p=0.05) and hash(a) == hash(Sampling(0.7, min_p=0.05))
    assert len({a, b, c, Sampling(0.7), Sampling(0.7, min_p=0.05)}) == 4


def test_parse_round_trip(monkeypatch):
    from longspec_amd.sampling import SAMPLING_ENV, env_sampling
    assert Sampling.parse("t=0.7,m=0.05,typ=0.9,seed=3") == Sampling(0.7, seed=3, min_p=0.05, typical_p=0.9)
    assert Sampling.parse("typ=0.5, t=2, k=4, p=0.5, m=1") == Sampling(2.0, 4, 0.5, 0, 1.0, 0.5)
    monkeypatch.setenv(SAMPLING_ENV, "t=0.6,m=0.05,typ=0.9,seed=1")
    assert env_sampling() == Sampling(0.6, seed=1, min_p=0.05, typical_p=0.9)
    for bad in ("t=0.7,m=2", "t=0.7,typ=0", "t=0.7,m=x", "t=0.7,m=0.1,m=0.2", "t=0.7,min_p=0.1"):
        with pytest.raises(ValueError):
            Sampling.parse(bad)
