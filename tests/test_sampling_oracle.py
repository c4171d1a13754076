"""tests/sampling_oracle.py, the reference of ``ops.sample_rows``: Philox known answers, the distribution of the draw with
and without filters, and the filters' edge cases.  No GPU."""
import numpy as np
import pytest

import sampling_oracle as so

CHI2_999_DF15 = 37.70            # 0.999 quantile of chi-square with 15 degrees of freedom


def _hex(words):
    return [f"{int(w):08x}" for w in words]


@pytest.mark.parametrize("counter,key,expect", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, expect):
    out = so.philox4x32_10([np.array([c], dtype=np.uint64) for c in counter], key)
    assert _hex([o[0] for o in out]) == expect.split()


def test_uniforms_are_fp32_exact_and_open():
    u = so.uniforms(4096, position=(1 << 40) + 5, stream=3, seed=(7 << 32) | 9)
    assert u.min() > 0 and u.max() < 1
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    # the counter carries the column block, both halves of the position and the stream; the key both halves of the seed
    base = dict(position=(1 << 40) + 5, stream=3, seed=(7 << 32) | 9)
    for change in (dict(position=5), dict(position=(1 << 40) + 6), dict(stream=4), dict(seed=9), dict(seed=(7 << 32) | 8)):
        assert not np.array_equal(so.uniforms(64, **{**base, **change}), u[:64])
    assert np.array_equal(so.uniforms(64, **base), u[:64])          # a prefix: column j reads block j >> 2, word j & 3


ROW16 = np.array([1.5, -0.25, 0.75, 2.0, 0.0, -1.0, 1.25, 0.5, -0.5, 1.75, 0.25, -0.75, 1.0, -1.5, 2.25, -2.0])


def _draws(x, n, **kw):
    return np.array([so.sample_row(x, pos, 0, 11, 0.7, **kw)[0] for pos in range(n)])


def _chi2(draws, probs):
    n = len(draws)
    obs = np.bincount(draws, minlength=len(probs)).astype(np.float64)
    live = probs > 0
    assert obs[~live].sum() == 0                                    # dropped tokens are drawn exactly never
    return float((((obs - n * probs) ** 2)[live] / (n * probs[live])).sum())


def _softmax(x, T, keep=None):
    p = np.exp((x - x.max()) / float(np.float32(T)))
    if keep is not None:
        p = np.where(keep, p, 0.0)
    return p / p.sum()


def test_draw_follows_softmax():
    chi2 = _chi2(_draws(ROW16, 20000), _softmax(ROW16, 0.7))
    print("chi2 (no filter):", chi2)
    assert chi2 < CHI2_999_DF15


def test_draw_with_top_k_follows_the_renormalised_kept_set():
    keep = ROW16 >= np.sort(ROW16)[-5]
    assert keep.sum() == 5
    chi2 = _chi2(_draws(ROW16, 20000, top_k=5), _softmax(ROW16, 0.7, keep))
    print("chi2 (top_k = 5):", chi2)
    assert chi2 < CHI2_999_DF15                                     # (4 degrees of freedom here: the bound is the looser one)


def test_draw_with_top_p_follows_the_renormalised_kept_set():
    p = _softmax(ROW16, 0.7)
    order = np.argsort(-p)
    n_keep = int(np.argmax(np.cumsum(p[order]) >= np.float32(0.8))) + 1
    keep = np.zeros(16, dtype=bool)
    keep[order[:n_keep]] = True
    assert 1 < n_keep < 16
    assert so.threshold(ROW16, 0.7, top_p=0.8) == ROW16[keep].min()
    chi2 = _chi2(_draws(ROW16, 20000, top_p=0.8), _softmax(ROW16, 0.7, keep))
    print("chi2 (top_p = 0.8):", chi2)
    assert chi2 < CHI2_999_DF15


def test_ties_at_the_kth_value_are_all_kept():
    x = np.array([3.0, 1.0, 2.0, 2.0, 2.0, 0.0, -1.0, 2.0])
    for k in (2, 3, 4, 5):
        _, _, _, kept, thr = so.sample_row(x, 0, 0, 0, 1.0, top_k=k)
        assert (kept, thr) == (5, 2.0)
    assert so.sample_row(x, 0, 0, 0, 1.0, top_k=1)[3:] == (1, 3.0)
    assert so.sample_row(x, 0, 0, 0, 1.0, top_k=6)[3:] == (6, 1.0)
    assert so.sample_row(x, 0, 0, 0, 1.0, top_k=100)[3:] == (8, -1.0)


def test_filters_off_keep_everything():
    _, _, _, kept, thr = so.sample_row(ROW16, 0, 0, 0, 0.7, top_k=0, top_p=1.0)
    assert (kept, thr) == (16, -2.0)


def test_tiny_top_p_keeps_the_maxima_only():
    x = np.array([1.0, 4.0, 2.0, 4.0, -3.0, 4.0, 0.0, 3.5])
    seen = set()
    for pos in range(64):
        idx, top2, _, kept, thr = so.sample_row(x, pos, 0, 5, 1.0, top_p=1e-6)
        assert (kept, thr) == (3, 4.0) and idx in (1, 3, 5) and top2[1] in (1, 3, 5) and top2[1] != idx
        seen.add(idx)
    assert seen == {1, 3, 5}


def test_minus_inf_is_never_kept_beside_a_finite_entry():
    x = np.array([-np.inf, 0.5, -np.inf, -np.inf, 0.25, -np.inf, -np.inf, -np.inf])
    for kw in (dict(), dict(top_k=5), dict(top_p=0.999999), dict(top_k=8, top_p=0.5)):
        for pos in range(16):
            idx, top2, keys, kept, thr = so.sample_row(x, pos, 0, 3, 1.3, **kw)
            assert idx in (1, 4) and kept <= 2 and thr >= 0.25
            assert all(j in (1, 4, -1) for j in top2)
    one = np.array([-np.inf, -np.inf, 7.0, -np.inf, -np.inf, -np.inf, -np.inf, -np.inf])
    assert so.sample_row(one, 0, 0, 0, 1.0) == (2, (2, -1), (so.gumbel_keys(one, 0, 0, 0, 1.0)[2], -np.inf), 1, 7.0)
    none = np.full(8, -np.inf)
    idx, top2, keys, kept, thr = so.sample_row(none, 0, 0, 0, 1.0, top_k=3)
    assert (idx, top2, kept, thr) == (0, (0, 1), 8, -np.inf) and keys == (-np.inf, -np.inf)


def test_top2_is_the_winner_and_the_runner_up_among_the_kept():
    rng = np.random.default_rng(0)
    x = np.round(rng.normal(size=64) * 2, 2)
    for pos in range(32):
        idx, top2, keys, kept, thr = so.sample_row(x, pos, 1, 9, 0.9, top_k=10)
        key = so.gumbel_keys(x, pos, 1, 9, 0.9)
        order = [j for j in np.argsort(-key, kind="stable") if x[j] >= thr]
        assert kept == len(order) and (idx, top2) == (order[0], (order[0], order[1]))
        assert keys == (key[order[0]], key[order[1]])
