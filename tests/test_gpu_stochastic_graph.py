"""temperature > 0 tree rounds replayed from HIP graphs (LlamaGlide.tree_round_stochastic with GRAPH_STOCHASTIC): the commit
kernel against the torch statements it replaces, and the seeded golden generations of the eager tests run again with every
round on the graph path -- same tokens, same counters, same random streams afterwards, one host read per replayed round."""
import random
import warnings

import numpy as np
import pytest
import torch

import cases

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------- #
# ls_tree_commit_stochastic
# --------------------------------------------------------------------------- #
def _commit_torch(acc_ids, acc_num, used, out, cache_lens, input_len, gamma, eos, tm, spec, logp, dl, acc_pad):
    """The statements of LlamaGlide.tree_round_stochastic behind verify_stochastic (llama_glide.py:1102-1121), batch 1."""
    W = acc_ids.size(-1)
    cols = (cache_lens - input_len).long().unsqueeze(1) + torch.arange(W)[None, :]
    out[torch.arange(1)[:, None], cols] = acc_ids
    dl += acc_num.to(torch.int32)
    n = int(acc_num[0])
    tm.fill_(0)
    tm[:, :, 0] = 1
    spec.fill_(0)
    spec[:, 0] = acc_ids[:, n - 1]
    logp.zero_()
    acc_pad.zero_()
    acc_pad[:, :W] = acc_ids
    over = int((cache_lens + acc_num.to(torch.int32) - input_len).max()) + gamma + 2 > out.size(1)
    hit = eos is not None and bool(out.eq(eos).any())
    return torch.tensor([[n, int(hit), int(used[0]), int(over)]], dtype=torch.int64)


@pytest.mark.parametrize("eos", [None, 7, 99], ids=["no_eos", "eos_stale", "eos_absent"])
@pytest.mark.parametrize("gamma", [1, 2, 3, 4, 5])
def test_commit_stochastic_matches_the_torch_statements(gamma, eos):
    from longspec_amd import ops
    W, Fn = gamma + 2, 1 + 2 * gamma
    rng = np.random.RandomState(40 + gamma)
    col0 = 5
    cap = col0 + W + 3                   # the budget test (:1118) trips for acc_num > 3 in the first round
    flags = set()
    for n in range(1, W + 1):
        input_len = torch.tensor([37], dtype=torch.int32)
        cache_lens = torch.tensor([37 + col0], dtype=torch.int32)
        out = torch.from_numpy(rng.randint(10, 20, size=(1, cap))).long()
        if eos == 7:
            out[0, 2] = 7                # a column written long ago: the whole buffer is tested (:1120)
        tm = torch.from_numpy(rng.randint(0, 2, size=(1, Fn, Fn))).long()
        spec = torch.from_numpy(rng.randint(0, 99, size=(1, Fn))).long()
        logp = torch.from_numpy(rng.randn(1, Fn).astype(np.float32))
        dl = torch.from_numpy(rng.randint(0, 1000, size=(1,))).int()
        acc_pad = torch.from_numpy(rng.randint(20, 30, size=(1, W))).long()
        cpu = [out, cache_lens, input_len, tm, spec, logp, dl, acc_pad]
        dev = [t.clone().cuda() for t in cpu]
        names = ("output_ids", "cache_lens", "input_len", "tree_mask", "all_spec", "logp_sum", "draft_kv_lens", "acc_pad")
        # two rounds on the same buffers: the second one's write position overlaps the first one's (cache_lens += a - 1)
        for rnd, (n_r, used_r) in enumerate(((n, 7), (1 + (n + 2) % W, -1))):
            acc_num = torch.tensor([n_r])
            acc_ids = torch.from_numpy(rng.randint(30, 90, size=(1, W))).long()
            acc_ids[:, n_r:] = 0
            used = torch.tensor([used_r], dtype=torch.int32)
            want = _commit_torch(acc_ids, acc_num, used, cpu[0], cpu[1], cpu[2], gamma, eos, *cpu[3:])
            got = ops.tree_commit_stochastic(acc_ids.cuda(), acc_num.cuda(), used.cuda(), dev[0], dev[1], dev[2], gamma, eos,
                                             *dev[3:])
            assert torch.equal(got.cpu(), want), (n, rnd, got.cpu(), want)
            for tc, td, name in zip(cpu, dev, names):
                assert torch.equal(tc, td.cpu()), (name, n, rnd)
            flags.add(int(want[0, 3]))
            if int(want[0, 3]):          # the loop stops here (:1118): a further round would write beyond the buffer
                break
            for t in (cpu[1], dev[1]):   # the next round's `cache_lens += a - 1` (:1094)
                t += n_r - 1
    if gamma >= 2:
        assert flags == {0, 1}


# --------------------------------------------------------------------------- #
# end to end
# --------------------------------------------------------------------------- #
def _build(run):
    from longspec_amd.llama_glide import LlamaGlide
    m = LlamaGlide(run["cfg"], device="cuda")
    m.load_state_dict({**run["target_sd"], **{"glide." + k: v for k, v in run["draft_sd"].items()}}, strict=True)
    return m


def _generate(run, graph, trace=True, before_rounds=None):
    """One seeded generation (seeds and noise hook of tests/test_gpu_generate.py) with every round eligible for the graph path
    (GRAPH_AFTER = 0) or none (GRAPH_STOCHASTIC off).  Returns the decode state, the per-round (acc_ids, acc_num) trace in the
    goldens' layout, the random states afterwards and the model."""
    from longspec_amd import ops
    m = _build(run)
    m.GRAPH_AFTER, m.GRAPH_STOCHASTIC = 0, graph
    states, ids, num = [], [], []
    orig_begin, orig_round = m.begin_tree_decode, m.tree_round_stochastic

    def begin(*a, **k):
        states.append(orig_begin(*a, **k))
        if before_rounds is not None:
            before_rounds(states[-1])
        return states[-1]

    def one_round(st):
        go = orig_round(st)
        if trace:
            pad = torch.full((1, 8), -1, dtype=torch.int64)
            pad[:, :st.acc_pad.shape[1]] = st.acc_pad.cpu()
            ids.append(pad)
            num.append(torch.tensor([st.a]))
        return go

    m.begin_tree_decode, m.tree_round_stochastic = begin, one_round
    ops.stochastic_noise_fn = lambda V, dtype, device: torch.empty(V, dtype=dtype).exponential_(1).to(device)
    try:
        random.seed(7000 + run["wseed"])
        torch.manual_seed(8000 + run["wseed"])
        try:
            m.tree_spec_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"),
                                 tree_shape=run["tree_shape"], max_gen_len=run["max_gen_len"], temperature=run["temperature"])
        except RuntimeError as e:          # a run that has left the reference's trajectory may accept gamma + 2 tokens (:1081)
            assert "verification batch" in str(e)
    finally:
        ops.stochastic_noise_fn = None
    rng = (random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state())
    return states[0], (ids, num), rng, m


def _same_generation(a, b):
    (st_a, _, rng_a, _), (st_b, _, rng_b, _) = a, b
    if not torch.equal(st_a.output_ids, st_b.output_ids):
        k = int((st_a.output_ids[0] != st_b.output_ids[0]).nonzero()[0])
        raise AssertionError(f"the graph rounds and the eager rounds part at output column {k}: a stochastic acceptance decided "
                             f"differently (to be traced to a ratio within the log-prob bound of tests/test_gpu_topk_store.py)")
    assert (int(st_a.count), int(st_a.num)) == (int(st_b.count), int(st_b.num))
    assert rng_a[0] == rng_b[0], "Python's generator is not where the eager path leaves it"
    assert torch.equal(rng_a[1], rng_b[1]) and torch.equal(rng_a[2], rng_b[2]), "torch's generators differ"


EAGER = {}


def _eager(run):
    """The eager generation of a run: computed once, shared by the tests that compare with it."""
    if run["name"] not in EAGER:
        EAGER[run["name"]] = _generate(run, graph=False)[:3] + (None,)
    return EAGER[run["name"]]


def _count_replays():
    real = torch.cuda.CUDAGraph.replay
    calls = {"n": 0}

    def replay(self):
        calls["n"] += 1
        return real(self)

    torch.cuda.CUDAGraph.replay = replay
    return calls, real


@pytest.mark.parametrize("run", list(cases.stochastic_runs()), ids=lambda r: r["name"])
def test_graph_rounds_match_eager_and_reference(run):
    calls, real = _count_replays()
    try:
        got = _generate(run, graph=True)
    finally:
        torch.cuda.CUDAGraph.replay = real
    st, (ids, num), _, _ = got
    assert st.use_graphs and st.graphs is not False and st.graph_captures >= 1 and calls["n"] >= 1, (st.graph_captures, calls)
    _same_generation(got, _eager(run))
    # the reference's golden run, in full (as test_tree_spec_generate_with_temperature_matches_reference)
    assert torch.equal(torch.cat(num, 0), run["tr_acc_num"])
    assert torch.equal(torch.cat(ids, 0), run["tr_acc_ids"])
    assert (int(st.count), int(st.num)) == (run["count"], run["num"])
    assert torch.equal(st.output_ids.cpu(), run["out"])


@pytest.mark.parametrize("run", list(cases.stochastic_runs(long=True)), ids=lambda r: r["name"])
def test_long_graph_rounds_match_eager_and_reference(run):
    calls, real = _count_replays()
    try:
        got = _generate(run, graph=True)
    finally:
        torch.cuda.CUDAGraph.replay = real
    st, (ids, num), _, _ = got
    assert st.use_graphs and st.graphs is not False and st.graph_captures >= 1 and calls["n"] >= 1, (st.graph_captures, calls)
    print(f"{run['name']}: {int(st.num) - 1} rounds, {st.graph_captures} captures, {calls['n']} replays")
    _same_generation(got, _eager(run))
    # the reference's trace: the leading rounds (as test_long_tree_run_with_temperature)
    ids, num = torch.cat(ids, 0), torch.cat(num, 0)
    n = min(ids.shape[0], run["tr_acc_ids"].shape[0])
    same = [torch.equal(ids[i], run["tr_acc_ids"][i]) and int(num[i]) == int(run["tr_acc_num"][i]) for i in range(n)]
    lead = same.index(False) if False in same else n
    print(f"{run['name']}: {lead} of {run['tr_acc_ids'].shape[0]} rounds reproduce the reference's stochastic trace")
    assert lead >= 16


def test_one_host_read_per_replayed_round():
    """torch.cuda.synchronize and the .tolist / .item / .cpu / int() / bool() reads of device tensors, counted inside every
    round whose graph was already captured when it began."""
    run = list(cases.stochastic_runs(long=True))[0]
    reads = {"n": 0}
    per_round = []
    patched = []

    def counting(owner, name):
        real = getattr(owner, name)

        def spy(*a, **k):
            if owner is torch.cuda or (a and isinstance(a[0], torch.Tensor) and a[0].is_cuda):
                reads["n"] += 1
            return real(*a, **k)

        patched.append((owner, name, real, name in vars(owner)))
        setattr(owner, name, spy)

    from longspec_amd.llama_glide import LlamaGlide
    real_round = LlamaGlide.tree_round_stochastic

    def one_round(self, st):
        replayed = st.use_graphs and st.replayer.captured((st.a, st.d0_rows))
        reads["n"] = 0
        go = real_round(self, st)
        if replayed:
            per_round.append(reads["n"])
        return go

    LlamaGlide.tree_round_stochastic = one_round
    try:
        counting(torch.cuda, "synchronize")
        for name in ("tolist", "item", "cpu", "numpy", "__int__", "__bool__", "__float__", "__index__"):
            counting(torch.Tensor, name)
        got = _generate(run, graph=True, trace=False)
    finally:
        LlamaGlide.tree_round_stochastic = real_round
        for owner, name, real, own in patched:
            if own:
                setattr(owner, name, real)
            else:
                delattr(owner, name)
    assert len(per_round) >= 20, f"only {len(per_round)} rounds were replayed"
    assert set(per_round) == {1}, per_round
    _same_generation(got, _eager(run))


def test_failed_capture_falls_back_to_eager_without_drawing_twice():
    """An exception in front of the first warm-up: that round runs eagerly on the words and the noise already drawn for it, the
    later ones on the eager path -- the generation is the eager one, token for token, and so are the random streams."""
    run = list(cases.stochastic_runs())[0]

    def before_rounds(st):
        def boom():
            raise RuntimeError("injected: sizing the capture failed")
        st.replayer._set_hints = boom

    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = _generate(run, graph=True, before_rounds=before_rounds)
    assert any("running eagerly" in str(x.message) for x in w), "the injected failure was not hit"
    st = got[0]
    assert st.graphs is False and st.graph_captures == 0
    _same_generation(got, _eager(run))
    assert torch.equal(st.output_ids.cpu(), run["out"])


def test_switch_and_prepare():
    """GRAPH_STOCHASTIC = False keeps the launch-by-launch rounds; prepare_tree_graphs captures nothing at temperature > 0."""
    run = list(cases.stochastic_runs())[0]
    m = _build(run)
    first = torch.tensor([3], device="cuda")
    lens = torch.tensor([run["prompt_len"]], dtype=torch.int32, device="cuda")
    st = m.begin_tree_decode(first, lens, run["prompt_len"], run["tree_shape"], 64, temperature=0.8)
    assert st.use_graphs
    m.prepare_tree_graphs(st)
    assert st.graph_captures == 0 and not st.graphs_forced and not st.replayer.entries
    m.GRAPH_STOCHASTIC = False
    assert not m.begin_tree_decode(first, lens, run["prompt_len"], run["tree_shape"], 64, temperature=0.8).use_graphs
