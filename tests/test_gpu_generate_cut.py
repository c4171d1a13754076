"""Sampled decoding under ``cut=`` end to end on the HIP kernels (toy Llama, fp16): the pairs of tests/test_host_generate_cut.py
on the device under the cross-loop rule of tests/sampled_runs.py, graph replay against launch-by-launch rounds, the single host
read of a replayed round, a vanishing ``top_n_sigma`` as greedy decoding, and the cuts behind ``penalties=``, ``ban=`` and
``guide=``."""
import numpy as np
import pytest
import torch

import sampled_runs as sr
import sampling_cut_oracle as sco
import test_host_generate_cut as hc
from longspec_amd import Ban, Cut, Guide, Penalties, Sampling
from test_gpu_generate_sampled import build
from test_host_generate_sampled import get_run

pytestmark = pytest.mark.gpu
_models = {}


def model_of(name):
    if name not in _models:
        _models[name] = build(get_run(hc.FAMILY, name))
    return get_run(hc.FAMILY, name), _models[name]


def _tree(m, run, sampling, cut, **kw):
    out, count, num, _, _ = m.tree_spec_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"),
                                                 tree_shape=run["tree_shape"], max_gen_len=run["max_gen_len"],
                                                 eos_id=run["eos_id"], sampling=sampling, cut=cut, **kw)
    return out.cpu(), int(count), int(num)


def _vanilla(m, run, sampling, cut, **kw):
    out, num, _ = m.vanilla_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"),
                                     max_gen_len=run["max_gen_len"], eos_id=run["eos_id"], sampling=sampling, cut=cut, **kw)
    return out.cpu(), num


@pytest.mark.parametrize("kind", list(hc.GROUPS))
def test_one_seed_gives_one_text_in_every_loop(kind):
    """The CPU file's pairs with the HIP operators: a loop may leave the device's vanilla text only where it took the vanilla
    run's runner-up and the two keys were closer than tol / T; at most one (seed, prompt) pair may part before its end."""
    from longspec_amd import ops
    parted, cut = [], hc.GROUPS[kind]["cut"]
    for name, seed in hc.GROUPS[kind]["pairs"]:
        run, m = model_of(name)
        sampling = hc.sampling_of(kind, seed)
        tol = sr.TOL[run["dtype"]]
        v_out, rec = sco.vanilla_with_record(m, ops, run, sampling, cut, device="cuda", max_gen_len=hc.GEN)
        n_v = sr.stop_len(v_out, m._stop_id(run["eos_id"], "vanilla"), hc.GEN)
        print(f"{kind} {name} seed {seed}: smallest key gap on the device {sr.min_gap(rec, n_v, run['prompt_len']):.3f}")
        for loop, (out, n) in hc.run_loops(m, run, sampling, cut, device="cuda").items():
            at = sr.parting(out, min(n, n_v), v_out, rec, run["prompt_len"], hc.T, tol, f"{name} seed {seed} {loop}")
            if at is not None:
                parted.append((name, seed, loop, at))
    print("parted:", parted)
    assert len({(n, s) for n, s, _, _ in parted}) <= 1, parted


@pytest.mark.parametrize("name", ["mixed", "mixed_small_tree"])
def test_graph_replay_is_bit_identical_to_eager_rounds(name):
    run = get_run(hc.FAMILY, name)
    m = build(run)
    s, c = Sampling(0.6, 40, 0.95, 3), Cut(2.0, 0.5, 0.05)
    m.GRAPH_AFTER = 0
    m.GRAPH_ROUNDS = False
    eager_t, eager_v = _tree(m, run, s, c), _vanilla(m, run, s, c)
    m.GRAPH_ROUNDS = True
    states = []
    orig = m.begin_tree_decode
    m.begin_tree_decode = lambda *a, **k: states.append(orig(*a, **k)) or states[-1]
    graph_t, graph_v = _tree(m, run, s, c), _vanilla(m, run, s, c)
    assert states[0].cut == c
    assert states[0].replayer.captures > 0 and not states[0].replayer.disabled, "no round was replayed"
    assert torch.equal(graph_t[0], eager_t[0]) and graph_t[1:] == eager_t[1:]
    assert torch.equal(graph_v[0], eager_v[0]) and graph_v[1] == eager_v[1]
    plain = _vanilla(m, run, s, None)
    assert not torch.equal(plain[0], graph_v[0]), "the cut left the text alone: the run shows nothing"


def test_one_host_read_per_replayed_round():
    """The spy of test_gpu_generate_band.py with both cuts on: the filters add launches, no host read."""
    from longspec_amd.llama_glide import LlamaGlide
    run = get_run(hc.FAMILY, "mixed")
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
        m.tree_spec_generate(run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda"), tree_shape=run["tree_shape"],
                             max_gen_len=run["max_gen_len"], eos_id=run["eos_id"], sampling=Sampling(0.6, seed=3),
                             cut=Cut(2.0, 0.5, 0.05))
    finally:
        LlamaGlide.tree_round = real_round
        for owner, name, real, own in patched:
            if own:
                setattr(owner, name, real)
            else:
                delattr(owner, name)
    assert len(per_round) >= 10, f"only {len(per_round)} rounds were replayed"
    assert set(per_round) == {1}, per_round


@pytest.mark.parametrize("name", ["forced", "mixed_small_tree"])
def test_a_vanishing_sigma_is_greedy_decoding(name):
    """``Cut(top_n_sigma=1e-6)`` keeps the maxima alone: the ``top_k=1`` text, loop by loop."""
    run = get_run(hc.FAMILY, name)
    m = build(run)
    a, b, c = Sampling(0.7, seed=5), Sampling(0.7, top_k=1, seed=5), Cut(top_n_sigma=1e-6)
    va, vb = _vanilla(m, run, a, c), _vanilla(m, run, b, None)
    assert torch.equal(va[0], vb[0]) and va[1] == vb[1] and torch.equal(va[0], run["vanilla_out"])
    ta, tb = _tree(m, run, a, c), _tree(m, run, b, None)
    assert torch.equal(ta[0], tb[0]) and ta[1:] == tb[1:] and torch.equal(ta[0], run["tree_out"])
    ids, pl = run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda")
    kw = dict(max_gen_len=run["max_gen_len"], eos_id=run["eos_id"])
    for call in (lambda **k: m.spec_generate(ids, pl, gamma=4, **kw, **k),
                 lambda **k: m.lookup_generate(ids, pl, gamma=4, max_ngram=3, min_ngram=1, **kw, **k),
                 lambda **k: m.lookup_generate(ids, pl, gamma=4, max_ngram=3, min_ngram=1, branches=2, **kw, **k)):
        ra, rb = call(sampling=a, cut=c), call(sampling=b)
        assert torch.equal(ra[0], rb[0]) and int(ra[1]) == int(rb[1]) and int(ra[2]) == int(rb[2])


class _DrawSpy:
    """The device's operator module; keeps, of every ``sample_rows`` call, the logit of each drawn token (host reads: for
    launch-by-launch runs only)."""

    def __init__(self):
        from longspec_amd import ops
        self._base, self.drawn, self.masked, self.cuts = ops, [], 0, 0

    def __getattr__(self, name):
        return getattr(self._base, name)

    def sample_rows(self, logits, positions, sampling, streams=None, **kw):
        out = self._base.sample_rows(logits, positions, sampling, streams=streams, **kw)
        idx = out[0] if isinstance(out, tuple) else out
        x = logits.reshape(-1, logits.shape[-1]).float()
        self.drawn += x.gather(1, idx.reshape(-1, 1)).view(-1).cpu().tolist()
        self.masked += int(torch.isinf(x).sum())
        self.cuts += kw.get("cut") is not None
        return out


@pytest.mark.parametrize("what", ["penalties", "ban", "guide"])
def test_a_draw_never_takes_a_masked_token(what):
    """Both cuts behind the operators that write -inf (or move logits): every token drawn in a vanilla and a tree run has a
    finite logit in the row the sampler was handed, and rows with -inf entries did reach the sampler."""
    run = get_run(hc.FAMILY, "mixed")
    m = build(run)
    V = run["cfg"].vocab_size
    extra = {"penalties": Penalties(1.3, 0.5, 0.25), "ban": Ban(no_repeat_ngram=2),
             "guide": Guide([[1, -1], [-1, 0]], np.arange(V) % 2)}[what]
    spy = _DrawSpy()
    m.ops, m.GRAPH_ROUNDS = spy, False
    try:
        kw = {what: extra, "sampling": Sampling(1.2, seed=11), "cut": Cut(2.0, 0.5, 0.01), "max_gen_len": 16, "eos_id": run["eos_id"]}
        ids, pl = run["prompt"].cuda(), torch.tensor([run["prompt_len"]], device="cuda")
        m.vanilla_generate(ids, pl, **kw)
        m.tree_spec_generate(ids, pl, tree_shape=run["tree_shape"], **kw)
    finally:
        m.ops, m.GRAPH_ROUNDS = spy._base, True
    assert spy.cuts >= 16, "the sampler was not handed the cut"
    assert len(spy.drawn) >= 32 and all(np.isfinite(v) for v in spy.drawn), spy.drawn
    if what != "penalties":
        assert spy.masked > 0, "no masked row reached the sampler: the run shows nothing"
