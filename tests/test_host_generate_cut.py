"""Sampled decoding under ``cut=`` (top_n_sigma, xtc, and both behind top_k / top_p) through the host loops on the CPU oracle
(tests/sampling_cut_oracle.py): one seed gives one text in the vanilla, chain, tree and prompt-lookup loops, as
test_host_generate_band.py shows for min_p / typical_p (tests/sampled_runs.py has the rule), and a vanishing ``top_n_sigma`` is
greedy decoding.

The (run, seed) pairs were found by running seeds 0, 1, 2, ... through this file's own vanilla oracle run and keeping those
where, at every position, (a) the two best keys are at least 8 tol / T apart and (b) the same holds against every token the
filters COULD keep were the logits off by tol, while the winner stays kept for sure -- at the lower edge of the band and, where
the xtc coin fires, at the upper one (sampling_cut_oracle.robust_cut_gap has the derivation) --, (c) a filter dropped a token
and (d), for xtc, the coin fired and took the row maximum away at least once.  All of it is asserted here for every pair.

T = 1.5 and 12 tokens, as in test_host_generate_band.py: the toy model's distributions are broad.  For the same reason the xtc
thresholds are small: at T = 1.5 the most likely of its 512 tokens holds a few per cent of the mass, so ``xtc_threshold = 0.01``
plays the part 0.1 plays on a real model; behind ``top_k = 40`` the shares are a few times larger and 0.06 does.  fp16 only: the
other files explain why bf16 leaves filters to the kernel tests."""
import numpy as np
import pytest
import torch

import sampled_runs as sr
import sampling_cut_oracle as sco
from longspec_amd import Cut, Sampling
from test_host_generate_sampled import build, get_run

T, GEN, FAMILY = 1.5, 12, "llama"
GROUPS = {
    "top_n_sigma": dict(sampling={}, cut=Cut(top_n_sigma=1.5),
                        pairs=[("forced", 23), ("forced", 151), ("mixed", 219), ("mixed_small_tree", 8), ("mixed_small_tree", 71),
                               ("gqa_mixed", 21)]),
    "xtc": dict(sampling={}, cut=Cut(xtc_probability=0.5, xtc_threshold=0.01),
                pairs=[("forced", 28), ("forced", 33), ("mixed", 39), ("mixed_small_tree", 167), ("mixed_small_tree", 189),
                       ("gqa_mixed", 2)]),
    "both": dict(sampling=dict(top_k=40, top_p=0.95), cut=Cut(top_n_sigma=2.0, xtc_probability=0.5, xtc_threshold=0.06),
                 pairs=[("forced", 2031), ("forced", 2103), ("mixed", 146), ("mixed", 2164), ("mixed_small_tree", 974),
                        ("gqa_mixed", 122)]),
}


def all_pairs():
    return [pytest.param(kind, name, seed, id=f"{kind}-{name}-{seed}") for kind, g in GROUPS.items() for name, seed in g["pairs"]]


def sampling_of(kind, seed):
    return Sampling(T, seed=seed, **GROUPS[kind]["sampling"])


def assert_wide_margin(kind, name, seed, run, v_out, rec):
    P, tol = run["prompt_len"], sr.TOL[run["dtype"]]
    for eos in (run["eos_id"], getattr(run["cfg"], "eos_token_id", None)):
        assert eos not in v_out[0].tolist(), "the pair was chosen so that no loop stops early"
    gap = sr.min_gap(rec, GEN, P)
    robust = sco.min_robust_cut_gap(rec, GEN, P, sampling_of(kind, seed), GROUPS[kind]["cut"], tol)
    print(f"{kind} {name} seed {seed}: smallest key gap {gap:.3f}, against the tokens the filters could keep {robust:.3f}, "
          f"wide margin {8 * tol / T:.3f}")
    assert gap >= 8 * tol / T, "choose another (seed, prompt) pair: a key gap of the vanilla run is inside the wide margin"
    assert robust >= 8 * tol / T, "choose another (seed, prompt) pair: a winner sits too close to an edge of the band"


def assert_the_filters_acted(kind, seed, run, rec):
    """A filter dropped a token; under xtc the coin fired and the row maximum went at least once, and what was emitted there
    is not the arg-max."""
    P, cut = run["prompt_len"], GROUPS[kind]["cut"]
    finite = [int(np.isfinite(rec["rows"][P - 1 + i]).sum()) for i in range(GEN)]
    assert any(rec[P - 1 + i][3] < finite[i] for i in range(GEN)), "the filters never dropped a token: the pair shows nothing"
    if cut.xtc_probability > 0.0:
        fired = [pos for pos in rec["rows"] if sco.fires(seed, pos, 0, cut.xtc_probability)]
        assert fired and len(fired) < GEN, "the coin fired never or always: the pair shows nothing"
        topped = [pos for pos in fired if rec["edges"][pos][1] < rec["rows"][pos].max()]
        assert topped, "xtc never took a row maximum away: the pair shows nothing"
        for pos in topped:
            assert rec["rows"][pos][rec[pos][0]] < rec["rows"][pos].max()
        for pos in set(rec["rows"]) - set(fired):
            assert rec["edges"][pos][1] == rec["rows"][pos].max()


def run_loops(m, run, sampling, cut, device=None):
    """{loop: (output_ids, tokens that count)} of the chain, the tree and the two prompt-lookup loops."""
    ids = run["prompt"].to(device) if device else run["prompt"]
    pl = torch.tensor([run["prompt_len"]], device=device)
    kw = dict(max_gen_len=GEN, eos_id=run["eos_id"], sampling=sampling, cut=cut)
    outs = {}
    out, count, num, _, _ = m.spec_generate(ids, pl, gamma=4, **kw)
    outs["chain"] = (out, min(int(count) + int(num), GEN))
    out, count, num, _, _ = m.tree_spec_generate(ids, pl, tree_shape=run["tree_shape"], **kw)
    outs["tree"] = (out, min(int(count) + int(num), GEN))
    for b in (1, 2):
        out, count, num, _, _ = m.lookup_generate(ids, pl, gamma=4, max_ngram=3, min_ngram=1, branches=b, **kw)
        outs[f"lookup{b}"] = (out, min(int(count) + int(num), GEN))
    return outs


@pytest.mark.parametrize("kind,name,seed", all_pairs())
def test_one_seed_gives_one_text_in_every_loop(kind, name, seed):
    assert len(GROUPS[kind]["pairs"]) >= 5
    run = get_run(FAMILY, name)
    assert run["dtype"] == torch.float16
    sampling, cut = sampling_of(kind, seed), GROUPS[kind]["cut"]
    m = build(run, ops=sco.ops)
    v_out, rec = sco.vanilla_with_record(m, sco.ops, run, sampling, cut, max_gen_len=GEN)
    assert_wide_margin(kind, name, seed, run, v_out, rec)
    assert_the_filters_acted(kind, seed, run, rec)
    P = run["prompt_len"]
    for loop, (out, n) in run_loops(m, run, sampling, cut).items():
        assert n >= GEN - 7, (loop, n)
        # on the CPU all loops compute one function of the same numbers: with that margin no run may part at all
        assert sr.parting(out, n, v_out, rec, P, T, sr.TOL[run["dtype"]], loop) is None, f"{loop} parts from the vanilla text"


@pytest.mark.parametrize("name", ["forced", "mixed_small_tree"])
def test_a_vanishing_sigma_is_greedy_decoding(name):
    """``Cut(top_n_sigma=1e-6)`` keeps the maxima alone: the text of ``top_k=1``, which test_host_generate_sampled.py holds to
    the goldens."""
    run = get_run(FAMILY, name)
    m = build(run, ops=sco.ops)
    pl = torch.tensor([run["prompt_len"]])
    texts = []
    for s, c in ((Sampling(0.7, seed=5), Cut(top_n_sigma=1e-6)), (Sampling(0.7, top_k=1, seed=5), None)):
        kw = dict(max_gen_len=run["max_gen_len"], eos_id=run["eos_id"], sampling=s, cut=c)
        v_out, v_num, _ = m.vanilla_generate(run["prompt"], pl, **kw)
        t_out, t_count, t_num, _, _ = m.tree_spec_generate(run["prompt"], pl, tree_shape=run["tree_shape"], **kw)
        texts.append((v_out, v_num, t_out, int(t_count), int(t_num)))
    a, b = texts
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and torch.equal(a[2], b[2]) and a[3:] == b[3:]
    assert torch.equal(a[0], run["vanilla_out"]) and torch.equal(a[2], run["tree_out"])
