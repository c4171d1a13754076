"""Sampled decoding (``sampling=``) through the host loops on the CPU oracle (tests/sampling_oracle.py): with one seed the
vanilla, chain, MagicDec and tree loops emit the same text (tests/sampled_runs.py has the rule), ``top_k=1`` is greedy
decoding, seeds matter, and the keyword's checks."""
import pytest
import torch

import cases
import sampled_runs as sr
import sampling_oracle as so
from longspec_amd import Sampling

# (run, seed) pairs, found by running seeds 0, 1, 2, ... through this file's own vanilla oracle run and keeping those where, at
# every position, (a) the two best keys are at least 8 tol / T apart and (b) the same holds against every token a filter
# COULD keep were the logits off by tol, while the winner stays kept for sure (sampled_runs.robust_gap: a threshold is a
# step, so an ulp can move a token across it however far apart the keys are).  `name@n`: the prompt tiled to n tokens, for
# MagicDec.  `cpu`: how many of the pairs run all four loops on the CPU oracle (every pair's margins are asserted there, and
# every pair runs on the GPU).  fp16: the toy Llama; bf16: the Qwen2 twin.
FP16 = dict(family="llama", temperature=0.8, top_k=40, top_p=0.95, max_gen_len=20, cpu=5,
            pairs=[("forced", 384), ("mixed", 226), ("mixed_small_tree", 729), ("gqa_mixed", 597), ("mixed@1030", 328),
                   ("forced", 420), ("forced", 570), ("mixed_small_tree", 42), ("mixed_small_tree", 477),
                   ("mixed_small_tree", 530), ("mixed@1030", 482)])
# bf16 logits are only good to 0.25, so the wide margin is 2 / T between the two best keys at EVERY position: only a high
# temperature and a short text make such pairs likely enough to be found at all; no filter, the kernel tests cover those
BF16 = dict(family="qwen2_bf16", temperature=6.0, top_k=0, top_p=1.0, max_gen_len=12, cpu=4,
            pairs=[("qwen_bf16_g5", 61), ("qwen_bf16_g5", 112), ("qwen_bf16_g7", 488), ("qwen_bf16_g5@1030", 196),
                   ("qwen_bf16_g5", 84), ("qwen_bf16_g5", 385), ("qwen_bf16_g5", 403), ("qwen_bf16_g5", 535),
                   ("qwen_bf16_g5@1030", 379), ("qwen_bf16_g5@1030", 394)])
GROUPS = {"fp16": FP16, "bf16": BF16}
_RUNS = {}


def get_run(family, name):
    """``name@n``: the run with its prompt tiled to n tokens."""
    if family not in _RUNS:
        _RUNS[family] = {r["name"]: r for r in cases.generate_runs(family)}
    name, _, n = name.partition("@")
    run = _RUNS[family][name]
    return sr.with_long_prompt(run, int(n)) if n else run


def build(run, ops=so.ops, device=None):
    from longspec_amd.llama_glide import LlamaGlide
    from longspec_amd.qwen2_glide import Qwen2Glide
    kw = dict(device=device) if device else dict(ops=ops)
    m = (Qwen2Glide if run["family"] == "qwen2" else LlamaGlide)(run["cfg"], dtype=run.get("dtype", torch.float16), **kw)
    m.load_state_dict({**run["target_sd"], **{"glide." + k: v for k, v in run["draft_sd"].items()}}, strict=True)
    return m


def all_pairs(cpu_only=False):
    return [pytest.param(kind, name, seed, id=f"{kind}-{name}-{seed}") for kind, g in GROUPS.items()
            for name, seed in (g["pairs"][:g["cpu"]] if cpu_only else g["pairs"])]


def run_loops(m, base_ops, run, sampling, gen, device=None):
    """The four loops with one seed: (vanilla text, its per-position record, {loop: (output_ids, tokens that count)})."""
    v_out, rec = sr.vanilla_with_record(m, base_ops, run, sampling, device=device, max_gen_len=gen)
    ids = run["prompt"].to(device) if device else run["prompt"]
    pl = torch.tensor([run["prompt_len"]], device=device)
    kw = dict(max_gen_len=gen, eos_id=run["eos_id"], sampling=sampling)
    outs = {}
    out, count, num, _, _ = m.spec_generate(ids, pl, gamma=4, **kw)
    outs["chain"] = (out, min(int(count) + int(num), gen), int(count))
    if run["prompt_len"] >= 1024:                                      # MagicDec's streaming cache: 32 sink + 1024 window rows
        out, count, num, _, _ = m.magicdec_generate(ids, pl, gamma=3, **kw)
        outs["magicdec"] = (out, min(int(count) + int(num), gen), int(count))
    out, count, num, _, _ = m.tree_spec_generate(ids, pl, tree_shape=run["tree_shape"], **kw)
    outs["tree"] = (out, min(int(count) + int(num), gen), int(count))
    return v_out, rec, outs


def _assert_wide_margin(kind, name, seed, run, v_out, rec):
    g = GROUPS[kind]
    T, gen, P = g["temperature"], g["max_gen_len"], run["prompt_len"]
    tol = sr.TOL[run["dtype"]]
    for eos in (run["eos_id"], getattr(run["cfg"], "eos_token_id", None)):
        assert eos not in v_out[0].tolist(), "the pair was chosen so that no loop stops early"
    gap = sr.min_gap(rec, gen, P)
    robust = sr.min_robust_gap(rec, gen, P, Sampling(T, g["top_k"], g["top_p"], seed), tol)
    print(f"{kind} {name} seed {seed}: smallest key gap {gap:.3f}, against the tokens a filter could keep {robust:.3f}, "
          f"wide margin {8 * tol / T:.3f}")
    assert gap >= 8 * tol / T, "choose another (seed, prompt) pair: a key gap of the vanilla run is inside the wide margin"
    assert robust >= 8 * tol / T, "choose another (seed, prompt) pair: a winner sits too close to a filter's threshold"


@pytest.mark.parametrize("kind,name,seed", all_pairs())
def test_pairs_have_a_wide_margin(kind, name, seed):
    g = GROUPS[kind]
    run = get_run(g["family"], name)
    sampling = Sampling(g["temperature"], g["top_k"], g["top_p"], seed)
    v_out, rec = sr.vanilla_with_record(build(run), so.ops, run, sampling, max_gen_len=g["max_gen_len"])
    _assert_wide_margin(kind, name, seed, run, v_out, rec)


@pytest.mark.parametrize("kind,name,seed", all_pairs(cpu_only=True))
def test_one_seed_gives_one_text_in_every_loop(kind, name, seed):
    g = GROUPS[kind]
    run = get_run(g["family"], name)
    T, gen, P = g["temperature"], g["max_gen_len"], run["prompt_len"]
    tol = sr.TOL[run["dtype"]]
    sampling = Sampling(T, g["top_k"], g["top_p"], seed)
    m = build(run)
    v_out, rec, outs = run_loops(m, so.ops, run, sampling, gen)
    _assert_wide_margin(kind, name, seed, run, v_out, rec)
    assert ("magicdec" in outs) == ("@" in name)
    for loop, (out, n, count) in outs.items():
        assert n >= gen - 7, (loop, n)                               # every loop ran to the end of its buffer
        # on the CPU all loops compute one function of the same numbers: with that margin no run may part at all
        assert sr.parting(out, n, v_out, rec, P, T, tol, loop) is None, f"{loop} parts from the vanilla text"


def _kept_spy():
    """A spy that records out_kept and the number of maxima of every row handed to ``sample_rows``."""
    kept, maxima = [], []

    class Spy(sr.Top2Spy):
        def sample_rows(self, logits, positions, sampling, streams=None, return_top2=False):
            r = self._base.sample_rows(logits, positions, sampling, streams=streams, return_top2=True)
            kept.append(r[3].reshape(-1).clone().cpu())
            x = logits.reshape(-1, logits.shape[-1]).float()
            maxima.append((x == x.max(dim=-1, keepdim=True).values).sum(dim=-1).to(torch.int32).cpu())
            return r if return_top2 else r[0]

    return Spy, kept, maxima


@pytest.mark.parametrize("family,name", [("llama", "forced"), ("llama", "mixed_small_tree"), ("qwen2", "qwen_g5")])
def test_top_k_1_is_greedy_decoding(family, name):
    """``Sampling(top_k=1)`` keeps the maximum alone: the reference's greedy goldens in output_ids, count and num, and
    out_kept == 1 on every row of every pass.  Ties at the k-th value are all kept, so a row whose maximum occurs twice keeps
    two: the two Llama runs have no such row in any pass; the Qwen2 run has two, in tree rows off the accepted path (16-bit
    logits collide), and out_kept must be the number of maxima there.  (The bf16 runs have such rows ON the vanilla path,
    where arg-max takes the first maximum and a draw either: they cannot reproduce the goldens for every seed.)"""
    run = get_run(family, name)
    m = build(run)
    Spy, kept, maxima = _kept_spy()
    m.ops = Spy(so.ops)
    pl = torch.tensor([run["prompt_len"]])
    kw = dict(max_gen_len=run["max_gen_len"], eos_id=run["eos_id"], sampling=Sampling(0.7, top_k=1, seed=5))
    v_out, v_num, _ = m.vanilla_generate(run["prompt"], pl, **kw)
    assert torch.equal(v_out, run["vanilla_out"]) and v_num == run["vanilla_num"]
    t_out, t_count, t_num, _, _ = m.tree_spec_generate(run["prompt"], pl, tree_shape=run["tree_shape"], **kw)
    assert torch.equal(t_out, run["tree_out"]) and (int(t_count), int(t_num)) == (run["tree_count"], run["tree_num"])
    s_out, s_count, s_num, _, _ = m.spec_generate(run["prompt"], pl, gamma=4, **kw)
    assert (int(s_count), int(s_num)) == (run["chain_count"], run["chain_num"])
    n = min(int(s_count) + int(s_num), run["max_gen_len"])
    assert torch.equal(s_out[:, :n], run["chain_out"][:, :n])
    kept, maxima = torch.cat(kept), torch.cat(maxima)
    assert kept.numel() > run["vanilla_num"] and torch.equal(kept, maxima), "a row kept something else than its maxima"
    if family == "llama":
        assert bool((kept == 1).all()), "a row kept more than its maximum"
    else:
        assert int((kept != 1).sum()) <= 2


def test_top_k_1_is_greedy_magicdec():
    run = list(cases.baseline_runs())[0]
    m = build(run)
    Spy, kept, maxima = _kept_spy()
    m.ops = Spy(so.ops)
    out, count, num, _, _ = m.magicdec_generate(run["prompt"], torch.tensor([run["prompt_len"]]), gamma=run["gamma"],
                                                max_gen_len=run["max_gen_len"], sampling=Sampling(1.3, top_k=1, seed=1))
    assert (int(count), int(num)) == (run["magicdec_count"], run["magicdec_num"])
    assert torch.equal(out, run["magicdec_out"])
    assert torch.equal(torch.cat(kept), torch.cat(maxima))


def test_seeds_matter_and_repeat():
    run = get_run("llama", "mixed")
    m = build(run)
    pl = torch.tensor([run["prompt_len"]])

    def tree(seed):
        out, count, num, _, _ = m.tree_spec_generate(run["prompt"], pl, tree_shape=run["tree_shape"], max_gen_len=24,
                                                     eos_id=run["eos_id"], sampling=Sampling(0.8, 40, 0.95, seed))
        return out[0, :int(count) + int(num)]

    a, b, a2 = tree(125), tree(126), tree(125)
    assert torch.equal(a, a2)
    n = min(a.numel(), b.numel())
    assert not torch.equal(a[:n], b[:n])
    greedy, _, _ = m.vanilla_generate(run["prompt"], pl, max_gen_len=24, eos_id=run["eos_id"])
    assert not torch.equal(a[:n], greedy[0, :n])                     # and it is not the arg-max text


def test_vanilla_batch_rows_are_streams():
    """Batch 2 with the same prompt in both rows: row 0 is the batch-1 text, row 1 (stream 1) another one."""
    run = get_run("llama", "mixed")
    m = build(run)
    s = Sampling(0.8, 40, 0.95, 125)
    one, _, _ = m.vanilla_generate(run["prompt"], torch.tensor([run["prompt_len"]]), max_gen_len=16, eos_id=run["eos_id"], sampling=s)
    two, _, _ = m.vanilla_generate(run["prompt"].repeat(2, 1), torch.tensor([run["prompt_len"]] * 2), max_gen_len=16,
                                   eos_id=run["eos_id"], sampling=s)
    assert torch.equal(two[0], one[0]) and not torch.equal(two[1], one[0])


def test_sampling_and_temperature_exclude_each_other():
    run = get_run("llama", "mixed")
    m = build(run)
    pl = torch.tensor([run["prompt_len"]])
    s = Sampling(0.8)
    with pytest.raises(ValueError, match="temperature"):
        m.tree_spec_generate(run["prompt"], pl, tree_shape=run["tree_shape"], max_gen_len=16, temperature=0.5, sampling=s)
    with pytest.raises(ValueError, match="temperature"):
        m.spec_generate(run["prompt"], pl, max_gen_len=16, temperature=0.5, sampling=s)
    with pytest.raises(ValueError, match="temperature"):
        m.magicdec_generate(run["prompt"], pl, max_gen_len=16, temperature=0.5, sampling=s)
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    with pytest.raises(ValueError, match="temperature"):
        m.begin_tree_decode(first, lens, run["prompt_len"], temperature=0.5, sampling=s)
    with pytest.raises(ValueError, match="temperature"):
        m.begin_chain_decode(first, lens, lens, run["prompt_len"], temperature=0.5, sampling=s)
    with pytest.raises(TypeError):
        m.vanilla_generate(run["prompt"], pl, max_gen_len=16, sampling=0.8)


def test_sampling_refuses_a_vocabulary_parallel_shard():
    from types import SimpleNamespace
    run = get_run("llama", "mixed")
    m = build(run)
    shard = SimpleNamespace(vocab_parallel=True)
    with pytest.raises(ValueError, match="vocabulary-parallel"):
        m.tree_spec_generate(run["prompt"], torch.tensor([run["prompt_len"]]), max_gen_len=16, shard=shard, sampling=Sampling(0.8))
    m.model.layers[-1].self_attn.shard = shard
    with pytest.raises(ValueError, match="vocabulary-parallel"):
        m.begin_tree_decode(torch.tensor([3]), torch.tensor([8], dtype=torch.int32), 8, sampling=Sampling(0.8))


def test_sampling_validates_its_arguments():
    s = Sampling(0.6, top_k=40, top_p=0.95, seed=1)
    assert (s.temperature, s.top_k, s.top_p, s.seed) == (0.6, 40, 0.95, 1) and s == Sampling(0.6, 40, 0.95, 1)
    assert Sampling(1) == Sampling(1.0, 0, 1.0, 0)
    for bad in (dict(temperature=0), dict(temperature=-1), dict(temperature=float("nan")), dict(temperature=float("inf")),
                dict(temperature=1, top_k=-1), dict(temperature=1, top_k=1.5), dict(temperature=1, top_p=0),
                dict(temperature=1, top_p=1.01), dict(temperature=1, seed=-1), dict(temperature=1, seed=1 << 64)):
        with pytest.raises(ValueError):
            Sampling(**bad)


def test_environment_default(monkeypatch):
    from longspec_amd.sampling import SAMPLING_ENV, env_sampling
    monkeypatch.delenv(SAMPLING_ENV, raising=False)
    assert env_sampling() is None
    monkeypatch.setenv(SAMPLING_ENV, "t=0.6,k=40,p=0.95,seed=1")
    assert env_sampling() == Sampling(0.6, 40, 0.95, 1)
    monkeypatch.setenv(SAMPLING_ENV, "seed=7, t=1.5")
    assert env_sampling() == Sampling(1.5, seed=7)
    for bad in ("k=40", "t=0.6,q=1", "t=abc", "t=0.6,t=0.7", "0.6", "t=0"):
        monkeypatch.setenv(SAMPLING_ENV, bad)
        with pytest.raises(ValueError):
            env_sampling()
    # the begin_*_decode functions take it when neither sampling nor a temperature is given
    run = get_run("llama", "mixed")
    m = build(run)
    monkeypatch.setenv(SAMPLING_ENV, "t=0.8,k=40,p=0.95,seed=125")
    first, lens = torch.tensor([3]), torch.tensor([run["prompt_len"]], dtype=torch.int32)
    assert m.begin_tree_decode(first, lens, run["prompt_len"]).sampling == Sampling(0.8, 40, 0.95, 125)
    assert m.begin_tree_decode(first, lens, run["prompt_len"], temperature=0.5).sampling is None
    assert m.begin_tree_decode(first, lens, run["prompt_len"], sampling=Sampling(2.0)).sampling == Sampling(2.0)
    assert m.begin_chain_decode(first, lens, lens, run["prompt_len"]).sampling == Sampling(0.8, 40, 0.95, 125)
    out = torch.zeros((1, 8), dtype=torch.int64)
    assert m.begin_vanilla_decode(out, lens.clone(), lens, run["prompt_len"]).sampling == Sampling(0.8, 40, 0.95, 125)
    pl = torch.tensor([run["prompt_len"]])
    env_out, _, _ = m.vanilla_generate(run["prompt"], pl, max_gen_len=12, eos_id=run["eos_id"])
    monkeypatch.delenv(SAMPLING_ENV)
    assert m.begin_tree_decode(first, lens, run["prompt_len"]).sampling is None
    arg_out, _, _ = m.vanilla_generate(run["prompt"], pl, max_gen_len=12, eos_id=run["eos_id"], sampling=Sampling(0.8, 40, 0.95, 125))
    assert torch.equal(env_out, arg_out)
