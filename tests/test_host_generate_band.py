"""Sampled decoding with ``min_p`` and with ``typical_p`` through the host loops on the CPU oracle
(tests/sampling_band_oracle.py): one seed gives one text in the vanilla, chain and tree loops, as test_host_generate_sampled.py
shows for top-k / top-p (tests/sampled_runs.py has the rule), and ``min_p=1`` is greedy decoding.

The (run, seed) pairs were found by running seeds 0, 1, 2, ... through this file's own vanilla oracle run and keeping those
where, at every position, (a) the two best keys are at least 8 tol / T apart and (b) the same holds against every token the
filter COULD keep were the logits off by tol, while the winner stays kept for sure (sampling_band_oracle.robust_band_gap: the
edges of the band are steps, as a threshold is).  Both margins are asserted here for every pair.  T = 1.5 and 12 tokens: the toy
model's distributions are broad (hundreds of its 512 tokens kept), so at T = 0.8 and 20 tokens, the setting of the top-k / top-p
pairs, one seed in several hundred passes (b) for typical_p; the filters and the loops do not depend on T.  fp16 only: the other
file explains why bf16 leaves filters to the kernel tests."""
import pytest
import torch

import sampled_runs as sr
import sampling_band_oracle as sbo
from longspec_amd import Sampling
from test_host_generate_sampled import build, get_run

T, GEN, FAMILY = 1.5, 12, "llama"
GROUPS = {
    "min_p": dict(kw=dict(min_p=0.1), pairs=[("forced", 9), ("forced", 12), ("mixed", 0), ("mixed", 2), ("mixed_small_tree", 1),
                                              ("gqa_mixed", 9)]),
    "typical_p": dict(kw=dict(typical_p=0.9), pairs=[("forced", 42), ("forced", 56), ("mixed", 69), ("mixed", 90),
                                                      ("mixed_small_tree", 184), ("gqa_mixed", 209)]),
}


def all_pairs():
    return [pytest.param(kind, name, seed, id=f"{kind}-{name}-{seed}") for kind, g in GROUPS.items() for name, seed in g["pairs"]]


def sampling_of(kind, seed):
    return Sampling(T, seed=seed, **GROUPS[kind]["kw"])


def assert_wide_margin(kind, name, seed, run, v_out, rec):
    P, tol = run["prompt_len"], sr.TOL[run["dtype"]]
    for eos in (run["eos_id"], getattr(run["cfg"], "eos_token_id", None)):
        assert eos not in v_out[0].tolist(), "the pair was chosen so that no loop stops early"
    gap = sr.min_gap(rec, GEN, P)
    robust = sbo.min_robust_band_gap(rec, GEN, P, sampling_of(kind, seed), tol)
    print(f"{kind} {name} seed {seed}: smallest key gap {gap:.3f}, against the tokens the filter could keep {robust:.3f}, "
          f"wide margin {8 * tol / T:.3f}")
    assert gap >= 8 * tol / T, "choose another (seed, prompt) pair: a key gap of the vanilla run is inside the wide margin"
    assert robust >= 8 * tol / T, "choose another (seed, prompt) pair: a winner sits too close to an edge of the band"


def run_loops(m, run, sampling, device=None):
    """{loop: (output_ids, tokens that count)} of the chain and the tree loop."""
    ids = run["prompt"].to(device) if device else run["prompt"]
    pl = torch.tensor([run["prompt_len"]], device=device)
    kw = dict(max_gen_len=GEN, eos_id=run["eos_id"], sampling=sampling)
    outs = {}
    out, count, num, _, _ = m.spec_generate(ids, pl, gamma=4, **kw)
    outs["chain"] = (out, min(int(count) + int(num), GEN))
    out, count, num, _, _ = m.tree_spec_generate(ids, pl, tree_shape=run["tree_shape"], **kw)
    outs["tree"] = (out, min(int(count) + int(num), GEN))
    return outs


@pytest.mark.parametrize("kind,name,seed", all_pairs())
def test_one_seed_gives_one_text_in_every_loop(kind, name, seed):
    assert len(GROUPS[kind]["pairs"]) >= 5
    run = get_run(FAMILY, name)
    assert run["dtype"] == torch.float16
    sampling = sampling_of(kind, seed)
    m = build(run, ops=sbo.ops)
    v_out, rec = sr.vanilla_with_record(m, sbo.ops, run, sampling, max_gen_len=GEN)
    assert_wide_margin(kind, name, seed, run, v_out, rec)
    P = run["prompt_len"]
    finite = [int(torch.isfinite(torch.from_numpy(rec["rows"][P - 1 + i])).sum()) for i in range(GEN)]
    assert any(rec[P - 1 + i][3] < finite[i] for i in range(GEN)), "the filter never dropped a token: the pair shows nothing"
    for loop, (out, n) in run_loops(m, run, sampling).items():
        assert n >= GEN - 7, (loop, n)
        # on the CPU all loops compute one function of the same numbers: with that margin no run may part at all
        assert sr.parting(out, n, v_out, rec, P, T, sr.TOL[run["dtype"]], loop) is None, f"{loop} parts from the vanilla text"


def test_typical_p_drops_the_most_likely_token_somewhere():
    """The toy model's rows are broad: the band of typical_p excludes the row maximum on rows of the runs above (the kernel
    tests have rows of both kinds), and what a run emits there is not the arg-max."""
    name, seed = GROUPS["typical_p"]["pairs"][0]
    run = get_run(FAMILY, name)
    _, rec = sr.vanilla_with_record(build(run, ops=sbo.ops), sbo.ops, run, sampling_of("typical_p", seed), max_gen_len=GEN)
    dropped = [pos for pos, x in rec["rows"].items() if sbo.band(x, T, typical_p=0.9)[1] < x.max()]
    assert dropped, "no row lost its maximum"
    for pos in dropped:
        assert rec["rows"][pos][rec[pos][0]] < rec["rows"][pos].max()


@pytest.mark.parametrize("name", ["forced", "mixed_small_tree"])
def test_min_p_1_is_greedy_decoding(name):
    """``min_p=1`` keeps the maxima alone: the text of ``top_k=1``, which test_host_generate_sampled.py holds to the goldens."""
    run = get_run(FAMILY, name)
    m = build(run, ops=sbo.ops)
    pl = torch.tensor([run["prompt_len"]])
    texts = []
    for s in (Sampling(0.7, seed=5, min_p=1.0), Sampling(0.7, top_k=1, seed=5)):
        kw = dict(max_gen_len=run["max_gen_len"], eos_id=run["eos_id"], sampling=s)
        v_out, v_num, _ = m.vanilla_generate(run["prompt"], pl, **kw)
        t_out, t_count, t_num, _, _ = m.tree_spec_generate(run["prompt"], pl, tree_shape=run["tree_shape"], **kw)
        texts.append((v_out, v_num, t_out, int(t_count), int(t_num)))
    a, b = texts
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and torch.equal(a[2], b[2]) and a[3:] == b[3:]
    assert torch.equal(a[0], run["vanilla_out"]) and torch.equal(a[2], run["tree_out"])


def test_the_loops_take_a_band_sampling_and_keep_their_exclusions():
    run = get_run(FAMILY, "mixed")
    m = build(run, ops=sbo.ops)
    pl = torch.tensor([run["prompt_len"]])
    s = Sampling(0.8, min_p=0.1, typical_p=0.9)
    with pytest.raises(ValueError, match="temperature"):
        m.tree_spec_generate(run["prompt"], pl, tree_shape=run["tree_shape"], max_gen_len=16, temperature=0.5, sampling=s)
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    assert m.begin_tree_decode(first, lens, run["prompt_len"], sampling=s).sampling == s
