"""Sampled decoding (``sampling=``) end to end on the HIP kernels: the cross-loop rule of tests/sampled_runs.py on the device
(toy Llama fp16, Qwen2 twin bf16), graph replay against launch-by-launch rounds, the single host read of a replayed round,
``top_k=1`` against the greedy goldens, seeds, batch rows as streams."""
import pytest
import torch

import sampled_runs as sr
from longspec_amd import Sampling
from test_host_generate_sampled import GROUPS, get_run

pytestmark = pytest.mark.gpu


def build(run):
    from longspec_amd.llama_glide import LlamaGlide
    from longspec_amd.qwen2_glide import Qwen2Glide
    m = (Qwen2Glide if run["family"] == "qwen2" else LlamaGlide)(run["cfg"], device="cuda", dtype=run.get("dtype", torch.float16))
    m.load_state_dict({**run["target_sd"], **{"glide." + k: v for k, v in run["draft_sd"].items()}}, strict=True)
    return m


def _loops(m, run, sampling, gen):
    ids = run["prompt"].cuda()
    pl = torch.tensor([run["prompt_len"]], device="cuda")
    kw = dict(max_gen_len=gen, eos_id=run["eos_id"], sampling=sampling)
    outs = {}
    out, count, num, _, _ = m.spec_generate(ids, pl, gamma=4, **kw)
    outs["chain"] = (out, min(int(count) + int(num), gen))
    if run["prompt_len"] >= 1024:
        out, count, num, _, _ = m.magicdec_generate(ids, pl, gamma=3, **kw)
        outs["magicdec"] = (out, min(int(count) + int(num), gen))
    out, count, num, _, _ = m.tree_spec_generate(ids, pl, tree_shape=run["tree_shape"], **kw)
    outs["tree"] = (out, min(int(count) + int(num), gen))
    return outs


@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_one_seed_gives_one_text_in_every_loop(kind):
    """The CPU file's rule with the HIP operators: a loop may leave the vanilla text only where it took the vanilla run's
    runner-up and the two keys were closer than tol / T; at most one (seed, prompt) pair may part before its end."""
    from longspec_amd import ops
    g = GROUPS[kind]
    assert len(g["pairs"]) >= 8
    T, gen = g["temperature"], g["max_gen_len"]
    models, parted = {}, []
    for name, seed in g["pairs"]:
        run = get_run(g["family"], name)
        if name not in models:
            models[name] = build(run)
        m = models[name]
        sampling = Sampling(T, g["top_k"], g["top_p"], seed)
        tol = sr.TOL[run["dtype"]]
        v_out, rec = sr.vanilla_with_record(m, ops, run, sampling, device="cuda", max_gen_len=gen)
        n_v = sr.stop_len(v_out, m._stop_id(run["eos_id"], "vanilla"), gen)
        print(f"{kind} {name} seed {seed}: smallest key gap on the device {sr.min_gap(rec, n_v, run['prompt_len']):.3f}")
        for loop, (out, n) in _loops(m, run, sampling, gen).items():
            at = sr.parting(out, min(n, n_v), v_out, rec, run["prompt_len"], T, tol, f"{name} seed {seed} {loop}")
            if at is not None:
                parted.append((name, seed, loop, at))
    print("parted:", parted)
    assert len({(n, s) for n, s, _, _ in parted}) <= 1, parted


def _tree(m, run, sampling, gen=None, **kw):
    out, count, num, _, _ = m.tree_spec_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"),
                                                 tree_shape=run["tree_shape"], max_gen_len=gen or run["max_gen_len"],
                                                 eos_id=run["eos_id"], sampling=sampling, **kw)
    return out.cpu(), int(count), int(num)


def _vanilla(m, run, sampling, gen=None, batch=1):
    out, num, _ = m.vanilla_generate(run["prompt"].cuda().repeat(batch, 1), torch.tensor([run["prompt_len"]] * batch, device="cuda"),
                                     max_gen_len=gen or run["max_gen_len"], eos_id=run["eos_id"], sampling=sampling)
    return out.cpu(), num


@pytest.mark.parametrize("family,name", [("llama", "mixed"), ("llama", "mixed_small_tree"), ("qwen2_bf16", "qwen_bf16_g5")])
def test_graph_replay_is_bit_identical_to_eager_rounds(family, name):
    run = get_run(family, name)
    m = build(run)
    s = Sampling(0.6, 40, 0.95, 3)
    m.GRAPH_AFTER = 0
    m.GRAPH_ROUNDS = False
    eager_t, eager_v = _tree(m, run, s), _vanilla(m, run, s)
    m.GRAPH_ROUNDS = True
    states = []
    orig = m.begin_tree_decode
    m.begin_tree_decode = lambda *a, **k: states.append(orig(*a, **k)) or states[-1]
    graph_t, graph_v = _tree(m, run, s), _vanilla(m, run, s)
    assert states[0].replayer.captures > 0 and not states[0].replayer.disabled, "no round was replayed"
    assert torch.equal(graph_t[0], eager_t[0]) and graph_t[1:] == eager_t[1:]
    assert torch.equal(graph_v[0], eager_v[0]) and graph_v[1] == eager_v[1]


def test_one_host_read_per_replayed_round():
    """torch.cuda.synchronize and the .tolist / .item / .cpu / int() / bool() reads of device tensors, counted inside every
    sampled round whose graph was already captured when it began (the spy of tests/test_gpu_stochastic_graph.py)."""
    from longspec_amd.llama_glide import LlamaGlide
    run = get_run("llama", "mixed")
    reads, per_round, patched = {"n": 0}, [], []

    def counting(owner, name):
        real = getattr(owner, name)

        def spy(*a, **k):
            if owner is torch.cuda or (a and isinstance(a[0], torch.Tensor) and a[0].is_cuda):
                reads["n"] += 1
            return real(*a, **k)

        patched.append((owner, name, real, name in vars(owner)))
        setattr(owner, name, spy)

    real_round = LlamaGlide.tree_round

    def one_round(self, st):
        replayed = st.use_graphs and st.replayer.captured(st.a)
        reads["n"] = 0
        go = real_round(self, st)
        if replayed:
            per_round.append(reads["n"])
        return go

    m = build(run)
    m.GRAPH_AFTER = 0
    LlamaGlide.tree_round = one_round
    try:
        counting(torch.cuda, "synchronize")
        for name in ("tolist", "item", "cpu", "numpy", "__int__", "__bool__", "__float__", "__index__"):
            counting(torch.Tensor, name)
        out, count, num, _, _ = m.tree_spec_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"),
                                                     tree_shape=run["tree_shape"], max_gen_len=run["max_gen_len"],
                                                     eos_id=run["eos_id"], sampling=Sampling(0.6, 40, 0.95, 3))
    finally:
        LlamaGlide.tree_round = real_round
        for owner, name, real, own in patched:
            if own:
                setattr(owner, name, real)
            else:
                delattr(owner, name)
    assert len(per_round) >= 10, f"only {len(per_round)} rounds were replayed"
    assert set(per_round) == {1}, per_round


@pytest.mark.parametrize("family,name", [("llama", "forced"), ("llama", "mixed_small_tree"), ("qwen2", "qwen_g5")])
def test_top_k_1_is_greedy_decoding(family, name):
    run = get_run(family, name)
    m = build(run)
    s = Sampling(0.7, top_k=1, seed=5)
    v_out, v_num = _vanilla(m, run, s)
    assert torch.equal(v_out, run["vanilla_out"]) and v_num == run["vanilla_num"]
    t_out, t_count, t_num = _tree(m, run, s)
    assert torch.equal(t_out, run["tree_out"]) and (t_count, t_num) == (run["tree_count"], run["tree_num"])
    s_out, s_count, s_num, _, _ = m.spec_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"), gamma=4,
                                                  max_gen_len=run["max_gen_len"], eos_id=run["eos_id"], sampling=s)
    assert (int(s_count), int(s_num)) == (run["chain_count"], run["chain_num"])
    n = min(int(s_count) + int(s_num), run["max_gen_len"])
    assert torch.equal(s_out[:, :n].cpu(), run["chain_out"][:, :n])


def test_a_second_generation_takes_its_own_seed():
    """The seed and the parameters are launch arguments of graphs that belong to one generation: the next generation on the
    same model object, with another seed, captures its own."""
    run = get_run("llama", "mixed")
    m = build(run)
    m.GRAPH_AFTER = 0
    a = _tree(m, run, Sampling(0.8, 40, 0.95, 125))
    b = _tree(m, run, Sampling(0.8, 40, 0.95, 126))
    b2 = _tree(m, run, Sampling(0.8, 40, 0.95, 126))
    a2 = _tree(m, run, Sampling(0.8, 40, 0.95, 125))
    n = min(a[1] + a[2], b[1] + b[2])
    assert not torch.equal(a[0][0, :n], b[0][0, :n])
    assert torch.equal(b[0], b2[0]) and b[1:] == b2[1:]
    assert torch.equal(a[0], a2[0]) and a[1:] == a2[1:]


def test_vanilla_batch_rows_are_streams():
    run = get_run("llama", "mixed")
    m = build(run)
    s = Sampling(0.8, 40, 0.95, 125)
    one, _ = _vanilla(m, run, s, gen=24)
    two, _ = _vanilla(m, run, s, gen=24, batch=2)
    assert torch.equal(two[0], one[0]), "row 0 of a batch is not the batch-1 text"
    assert not torch.equal(two[1], one[0]), "row 1 drew row 0's noise"


def test_sampled_rounds_accept_draft_tokens():
    """The forced-agreement toy weights: the draft's beams hold the target's likely tokens, so a sampled round accepts some."""
    run = get_run("llama", "forced")
    m = build(run)
    out, count, num = _tree(m, run, Sampling(0.3, 40, 0.95, 7))
    assert count > 0 and num > 0, (count, num)
