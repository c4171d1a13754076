"""``longspec_amd.Cut`` and the oracle of its two filters (tests/sampling_cut_oracle.py): the keyword's checks, known answers of
the xtc coin -- a public contract, as the watermark's hash is --, and the properties the definitions in longspec_amd/cut.py
promise.  Runs without a GPU."""
import math

import numpy as np
import pytest
import torch

import sampling_band_oracle as sbo
import sampling_cut_oracle as sco
import sampling_oracle as so
from longspec_amd import Cut, Sampling
from longspec_amd.cut import CUT_ENV, env_cut, resolve
from test_host_generate_sampled import build, get_run


def test_cut_validates_its_arguments():
    c = Cut(top_n_sigma=1.0, xtc_probability=0.5, xtc_threshold=0.1)
    assert (c.top_n_sigma, c.xtc_probability, c.xtc_threshold) == (1.0, 0.5, 0.1)
    assert c == Cut(1.0, 0.5, 0.1) and hash(c) == hash(Cut(1.0, 0.5, 0.1)) and c != Cut(1.0, 0.5, 0.2) and c != "cut"
    assert Cut() == Cut(0.0, 0.0, 0.1) and not Cut().on and Cut(top_n_sigma=1).on and Cut(xtc_probability=1).on
    assert eval(repr(c)) == c
    assert Cut.__slots__ == ("top_n_sigma", "xtc_probability", "xtc_threshold")
    for bad in (dict(top_n_sigma=-0.1), dict(top_n_sigma=math.inf), dict(top_n_sigma=math.nan), dict(xtc_probability=-0.1),
                dict(xtc_probability=1.01), dict(xtc_probability=math.nan), dict(xtc_threshold=0.0), dict(xtc_threshold=1.01),
                dict(xtc_threshold=-1), dict(xtc_threshold=math.nan)):
        with pytest.raises(ValueError):
            Cut(**bad)
    for bad in (dict(top_n_sigma="1"), dict(xtc_probability=None), dict(xtc_threshold=True)):
        with pytest.raises(TypeError):
            Cut(**bad)


def test_parse_and_the_environment_default(monkeypatch):
    assert Cut.parse("sigma=1.0,xtcp=0.5,xtct=0.1") == Cut(1.0, 0.5, 0.1)
    assert Cut.parse(" xtct=0.2 , sigma=2") == Cut(2.0, 0.0, 0.2)
    for bad in ("sigma", "sigma=1,sigma=2", "n=1", "sigma=abc", "xtcp=2", "xtct=0", "", "sigma=1,,"):
        with pytest.raises(ValueError):
            Cut.parse(bad)
    monkeypatch.delenv(CUT_ENV, raising=False)
    assert env_cut() is None
    monkeypatch.setenv(CUT_ENV, "sigma=1.0,xtcp=0.5,xtct=0.1")
    assert env_cut() == Cut(1.0, 0.5, 0.1)
    s = Sampling(0.8)
    assert resolve(None, None, use_env=True, sampling=s) == Cut(1.0, 0.5, 0.1)
    assert resolve(None, None, use_env=False, sampling=s) is None
    assert resolve(None, 0.5, use_env=True, sampling=None) is None           # temperature > 0: the default is not consulted
    assert resolve(Cut(2.0), None, use_env=True, sampling=s) == Cut(2.0)
    assert resolve(Cut(), None, use_env=True, sampling=None) is None         # both filters off: "off", with or without sampling=
    with pytest.raises(ValueError, match=r"cut=.*sampling="):
        resolve(None, None, use_env=True, sampling=None)                     # from the environment
    with pytest.raises(ValueError, match=r"cut=.*sampling="):
        resolve(Cut(1.0), None, use_env=False, sampling=None)                # passed
    with pytest.raises(ValueError, match="temperature"):
        resolve(Cut(1.0), 0.5, use_env=True, sampling=s)
    with pytest.raises(TypeError):
        resolve(1.0, None, use_env=True, sampling=s)
    monkeypatch.setenv(CUT_ENV, "xtcp=0.0")
    assert resolve(None, None, use_env=True, sampling=None) is None


def test_the_loops_take_a_cut_and_keep_its_exclusions(monkeypatch):
    from types import SimpleNamespace
    monkeypatch.delenv(CUT_ENV, raising=False)
    monkeypatch.delenv("LONGSPEC_SAMPLING", raising=False)
    run = get_run("llama", "mixed")
    m = build(run, ops=sco.ops)
    pl = torch.tensor([run["prompt_len"]])
    s, c = Sampling(0.8), Cut(1.0, 0.5, 0.1)
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    P = run["prompt_len"]
    out = torch.zeros((1, 8), dtype=torch.int64)
    states = [m.begin_tree_decode(first, lens, P, sampling=s, cut=c), m.begin_chain_decode(first, lens, lens, P, sampling=s, cut=c),
              m.begin_vanilla_decode(out, lens.clone(), lens, P, sampling=s, cut=c),
              m.begin_lookup_decode(first, lens, lens, P, run["prompt"], sampling=s, cut=c),
              m.begin_lookup_decode(first, lens, lens, P, run["prompt"], sampling=s, cut=c, branches=2)]
    for st in states:
        assert st.cut == c and st.rules.cut == c
    assert m.begin_tree_decode(first, lens, P, sampling=s, cut=Cut()).cut is None
    assert m.begin_tree_decode(first, lens, P, sampling=s).cut is None
    kw = dict(max_gen_len=8, eos_id=run["eos_id"])
    for call in (lambda **k: m.vanilla_generate(run["prompt"], pl, **kw, **k),
                 lambda **k: m.spec_generate(run["prompt"], pl, **kw, **k),
                 lambda **k: m.magicdec_generate(run["prompt"], pl, **kw, **k),
                 lambda **k: m.lookup_generate(run["prompt"], pl, **kw, **k),
                 lambda **k: m.lookup_generate(run["prompt"], pl, branches=2, **kw, **k),
                 lambda **k: m.tree_spec_generate(run["prompt"], pl, tree_shape=run["tree_shape"], **kw, **k)):
        with pytest.raises(ValueError, match=r"cut=.*sampling="):
            call(cut=c)
        with pytest.raises(TypeError):
            call(sampling=s, cut=0.5)
    for call in (m.spec_generate, m.magicdec_generate):
        with pytest.raises(ValueError, match="temperature"):
            call(run["prompt"], pl, temperature=0.5, cut=c, **kw)
    with pytest.raises(ValueError, match="temperature"):
        m.tree_spec_generate(run["prompt"], pl, tree_shape=run["tree_shape"], temperature=0.5, cut=c, **kw)
    monkeypatch.setenv(CUT_ENV, "sigma=1.5")
    with pytest.raises(ValueError, match=r"cut=.*sampling="):
        m.begin_tree_decode(first, lens, P)
    assert m.begin_tree_decode(first, lens, P, sampling=s).cut == Cut(1.5)
    assert m.begin_tree_decode(first, lens, P, temperature=0.5).cut is None
    monkeypatch.delenv(CUT_ENV)
    shard = SimpleNamespace(vocab_parallel=True)
    with pytest.raises(ValueError, match="vocabulary-parallel"):
        m.tree_spec_generate(run["prompt"], pl, max_gen_len=16, shard=shard, sampling=s, cut=c)


def test_tokens_passes_the_keyword_only_when_a_cut_is_on():
    """The operator objects of the older CPU tests do not know ``cut=``: a loop without a cut must not name it."""
    from longspec_amd.target_rules import TargetRules
    seen = []

    class Spy:
        def sample_rows(self, logits, positions, sampling, streams=None, **kw):
            seen.append(kw)
            return torch.zeros(logits.shape[:-1], dtype=torch.int64)

    x, pos = torch.zeros((1, 8), dtype=torch.float16), torch.zeros((1,), dtype=torch.int64)
    TargetRules(Spy(), 8, "cpu", sampling=Sampling(1.0)).tokens(x, pos)
    TargetRules(Spy(), 8, "cpu", sampling=Sampling(1.0), cut=Cut()).tokens(x, pos)
    TargetRules(Spy(), 8, "cpu", sampling=Sampling(1.0), cut=Cut(1.0)).tokens(x, pos)
    assert seen == [{}, {}, {"cut": Cut(1.0)}]


# ---- the coin ---------------------------------------------------------------------------------------------------------------

def test_philox_known_answers():
    """The two published Philox4x32-10 vectors of Random123's kat_vectors: the oracle's Philox is the public one."""
    assert sco.philox_words((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert sco.philox_words((0xffffffff,) * 4, (0xffffffff,) * 2) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)


COIN_KNOWN = [   # (seed, position, stream) -> word 0 of Philox(counter (0xFFFFFFFF, position lo, position hi, stream), key seed)
    ((0, 0, 0), 0xc5b20a9d), ((1, 259, 0), 0x11f2dddc), ((0x123456789ABCDEF0, 2 ** 40 + 17, 3), 0xd3a1f763),
    ((7, 4095, 68), 0xd3f47b2e), ((2 ** 64 - 1, 2 ** 63 - 1, 2 ** 31 - 1), 0x1345a484)]


@pytest.mark.parametrize("args,word", COIN_KNOWN)
def test_coin_known_answers(args, word):
    seed, position, stream = args
    u = ((word >> 9) + 0.5) * 2.0 ** -23
    assert sco.coin(seed, position, stream) == u and float(np.float32(u)) == u and 0.0 < u < 1.0
    # the numpy Philox of the sampling oracle, written separately, gives the same word
    w = so.philox4x32_10((0xFFFFFFFF, position & 0xFFFFFFFF, position >> 32, stream), (seed & 0xFFFFFFFF, seed >> 32))[0]
    assert int(w) == word
    for P in (0.0, float(np.float32(u)), float(np.nextafter(np.float32(u), np.float32(1))), 1.0):
        assert sco.fires(seed, position, stream, P) == (u < P)


def test_coin_fires_half_the_time():
    """Positions 0..4095 at P = 0.5 and seed 20261021: the count is a fixed number, 2006, 1.3 binomial deviations (32) below
    2048; P = 0 never fires and P = 1 always does."""
    n = sum(sco.fires(20261021, p, 0, 0.5) for p in range(4096))
    assert abs(n - 2048) <= 5 * math.sqrt(4096 * 0.25)
    assert n == 2006
    assert not any(sco.fires(20261021, p, 0, 0.0) for p in range(256)) and all(sco.fires(20261021, p, 0, 1.0) for p in range(256))
    # streams and seeds give other coins
    a = [sco.fires(20261021, p, 0, 0.5) for p in range(256)]
    assert a != [sco.fires(20261021, p, 1, 0.5) for p in range(256)] and a != [sco.fires(20261022, p, 0, 0.5) for p in range(256)]


# ---- top_n_sigma ------------------------------------------------------------------------------------------------------------

def _rows():
    g = np.random.default_rng(5)
    rows = [torch.from_numpy(g.normal(0, s, 512)).half().double().numpy() for s in (0.5, 2.0, 6.0)]
    holes = rows[1].copy()
    holes[g.random(512) < 0.3] = -np.inf
    return rows + [holes]


def test_sigma_by_hand():
    x = np.array([4.0, 2.0, 2.0, 0.0, -np.inf, -np.inf, -np.inf, -np.inf])       # mean 2, deviations 2 0 0 2: sigma = sqrt(2)
    sigma, t = sco.sigma_threshold(x, 1.0)
    assert sigma == pytest.approx(math.sqrt(2.0), abs=1e-15) and t == pytest.approx(4.0 - math.sqrt(2.0), abs=1e-15)
    assert sco.band(x, 0.7, cut=Cut(1.0)) == (4.0, 4.0)
    assert sco.band(x, 0.7, cut=Cut(1.5)) == (2.0, 4.0)                           # 4 - 2.12 = 1.88
    assert sco.band(x, 0.7, cut=Cut(3.0)) == (0.0, 4.0)
    # not divided by the temperature: the same set at every T
    assert {sco.band(x, T, cut=Cut(1.5)) for T in (0.1, 1.0, 5.0)} == {(2.0, 4.0)}


def test_sigma_kept_set_grows_with_n():
    for x in _rows():
        lows = [sco.band(x, 0.9, cut=Cut(n))[0] for n in (1e-6, 0.5, 1.0, 2.0, 3.0, 10.0, 100.0)]
        fin = x[np.isfinite(x)]
        assert lows == sorted(lows, reverse=True)
        assert lows[0] == fin.max() and lows[-1] == fin.min() and lows[2] > lows[4]
        assert all(sco.band(x, 0.9, cut=Cut(n))[1] == fin.max() for n in (0.5, 3.0))


def test_sigma_edge_rows():
    inf = -np.inf
    assert sco.band(np.full(8, inf), 1.0, cut=Cut(1.0)) == (inf, inf)             # left alone
    assert sco.band(np.full(8, 1.5), 1.0, cut=Cut(1.0)) == (1.5, 1.5)             # all equal: sigma = 0 keeps the maxima
    one = np.full(8, inf)
    one[3] = -2.0
    assert sco.band(one, 1.0, cut=Cut(1.0)) == (-2.0, -2.0)
    idx, _, kept, lo, hi = sco.sample_row(np.full(8, inf), 3, 0, 1, 1.0, cut=Cut(1.0, 1.0, 0.1))
    assert (idx, kept, lo, hi) == (0, 8, inf, inf)


def test_sigma_intersects_with_top_k_and_top_p_weighs_what_both_kept():
    x = _rows()[1]
    for k, n in ((5, 3.0), (200, 1.0)):
        lo_both = sco.band(x, 0.8, top_k=k, cut=Cut(n))[0]
        assert lo_both == max(sbo.band(x, 0.8, top_k=k)[0], sco.band(x, 0.8, cut=Cut(n))[0])
    lo = sco.band(x, 0.8, top_k=200, top_p=0.9, cut=Cut(1.0))[0]
    masked = np.where(x >= sco.band(x, 0.8, top_k=200, cut=Cut(1.0))[0], x, -np.inf)
    assert lo == sbo.band(masked, 0.8, top_p=0.9)[0] and lo > sbo.band(x, 0.8, top_k=200, top_p=0.9)[0]


# ---- xtc --------------------------------------------------------------------------------------------------------------------

def test_xtc_by_hand():
    T = 1.0
    with np.errstate(divide="ignore"):
        x = np.log(np.array([0.5, 0.3, 0.15, 0.05, 0, 0, 0, 0]))                  # shares 0.5 0.3 0.15 0.05, four -inf
    on = Cut(xtc_probability=1.0, xtc_threshold=0.1)
    lo, hi = sco.band(x, T, cut=on, fired=True)
    assert (lo, hi) == (x[3], x[2])                                               # 0.5 and 0.3 go, 0.15 is the last that qualifies
    assert sco.band(x, T, cut=on, fired=False) == (x[3], x[0])
    assert sco.band(x, T, cut=Cut(xtc_probability=1.0, xtc_threshold=0.2), fired=True) == (x[3], x[1])
    # one token qualifies: nothing changes; theta > 0.5 without a tie at the top: nothing changes
    assert sco.band(x, T, cut=Cut(xtc_probability=1.0, xtc_threshold=0.4), fired=True) == (x[3], x[0])
    assert sco.band(x, T, cut=Cut(xtc_probability=1.0, xtc_threshold=0.51), fired=True) == (x[3], x[0])
    assert sco.band(x, T, cut=Cut(xtc_probability=1.0, xtc_threshold=1.0), fired=True) == (x[3], x[0])
    # behind top_k = 2 the shares are 0.625 and 0.375 of S
    assert sco.band(x, T, top_k=2, cut=Cut(xtc_probability=1.0, xtc_threshold=0.37), fired=True) == (x[1], x[1])
    assert sco.band(x, T, top_k=2, cut=Cut(xtc_probability=1.0, xtc_threshold=0.38), fired=True) == (x[1], x[0])


def test_xtc_keeps_every_token_tied_at_the_cut_value():
    x = np.array([2.0, 1.0, 1.0, 1.0, -3.0, -3.0, -np.inf, -np.inf])
    c = Cut(xtc_probability=1.0, xtc_threshold=0.1)
    lo, hi = sco.band(x, 1.0, cut=c, fired=True)
    assert (lo, hi) == (-3.0, 1.0)
    seed = next(s for s in range(64) if sco.fires(s, 11, 0, 1.0))
    idx, _, kept, lo, hi = sco.sample_row(x, 11, 0, seed, 1.0, cut=c)
    assert kept == 5 and idx != 0
    # a tie at the top qualifies together under theta > 0.5 only if each share does: two maxima of 0.5 - eps do not
    tie = np.array([1.0, 1.0, -9.0, -9.0, -9.0, -9.0, -9.0, -9.0])
    assert sco.band(tie, 1.0, cut=Cut(xtc_probability=1.0, xtc_threshold=0.49), fired=True) == (-9.0, 1.0)


def test_xtc_is_a_no_op_above_half_and_never_empties_a_row():
    for x in _rows():
        fin = x[np.isfinite(x)]
        for T in (0.3, 1.0, 1.5):
            for theta in (0.001, 0.01, 0.1, 0.3, 0.5):
                lo, hi = sco.band(x, T, cut=Cut(xtc_probability=1.0, xtc_threshold=theta), fired=True)
                kept = fin[(fin >= lo) & (fin <= hi)]
                assert kept.size >= 1 and lo == fin.min() and hi in fin
                w = np.exp((fin - fin.max()) / T)
                q = w / w.sum()
                assert (q[fin > hi] >= theta).all()                               # only tokens at or above the threshold go
                if (q >= theta).sum() <= 1:
                    assert hi == fin.max()                                        # one token qualifies, or none: unchanged
            if np.unique(fin)[-1] != np.unique(fin)[-2] and (fin == fin.max()).sum() == 1:
                assert sco.band(x, T, cut=Cut(xtc_probability=1.0, xtc_threshold=0.51), fired=True) == (fin.min(), fin.max())


def test_ops_object_extends_the_band_oracle():
    g = torch.Generator().manual_seed(3)
    x = torch.randn((3, 2, 64), generator=g).half()
    pos = torch.arange(6).view(3, 2) + 100
    streams = torch.arange(3, dtype=torch.int32).view(3, 1).expand(3, 2)
    s = Sampling(0.9, top_k=20, seed=4, min_p=0.01)
    assert torch.equal(sco.ops.sample_rows(x, pos, s, streams=streams), sbo.ops.sample_rows(x, pos, s, streams=streams))
    assert torch.equal(sco.ops.sample_rows(x, pos, s, streams=streams, cut=Cut()), sbo.ops.sample_rows(x, pos, s, streams=streams))
    idx, t2i, t2k, kept, thr, upper = sco.ops.sample_rows(x, pos, s, streams=streams, return_top2=True, return_upper=True,
                                                          cut=Cut(1.0, 1.0, 0.05))
    base = sbo.ops.sample_rows(x, pos, s, streams=streams, return_top2=True, return_upper=True)
    assert idx.shape == (3, 2) and (kept <= base[3]).all() and (kept < base[3]).any() and (kept >= 1).all()
    assert (thr >= base[4]).all() and (upper <= base[5]).all()
    assert sco.ops.argmax_rows is sbo.ops.argmax_rows
