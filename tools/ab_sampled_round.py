"""A/B/C timing of the tree round on ONE box: blocks of the greedy round (temperature 0), of the sampled round
(``sampling=``: the greedy round with ``ops.sample_rows`` in place of ``ops.argmax_rows``) and of the reference-style
temperature > 0 round alternate, all replayed from HIP graphs, on the synthetic-KV setting of bench.py (Llama-3-8B dimensions,
16k-token prefix, tree 4 16 16 16 16).  Writes profiles/sampled_round_ab.json.

    python tools/ab_sampled_round.py [--blocks 6] [--per 15] [--sampling t=0.6,k=50,p=0.95,seed=1]
                                     [--more t=0.6,m=0.05,seed=1 --more t=0.6,typ=0.9,seed=1]
                                     [--more "t=0.6,k=50,p=0.95,seed=1;sigma=1.0,xtcp=0.5,xtct=0.1"]

``--more SPEC`` adds a further sampled arm (named ``sampled[SPEC]``) to the interleaving: the min_p and typical_p rounds are
held against the ``sampled`` arm (top-k / top-p, the launches of ``ls_sample_rows``) of the same run.  ``SPEC;CUT`` adds a
LONGSPEC_CUT string (``cut=``: top_n_sigma, xtc) to the arm.

Each figure is a host clock around `per` rounds that end in a device synchronise; the spread is what the blocks of ONE arm
differ by on this box in this run, the yardstick for the difference between the arms.  The three arms keep their own decode
state over the same synthetic caches.  Tokens per round on random weights say nothing about a real model: not reported."""
import argparse
import json
import os
import random
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from longspec_amd import Cut, Sampling  # noqa: E402

PREFIX, TEMPERATURE = 16384, 0.8
ARMS = ("greedy", "sampled", "stochastic")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per", type=int, default=15)
    ap.add_argument("--sampling", default="t=0.6,k=50,p=0.95,seed=1")
    ap.add_argument("--more", action="append", default=[],
                    help="a further sampled arm, a LONGSPEC_SAMPLING string, optionally ';' and a LONGSPEC_CUT string")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampled_round_ab.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    blocks, per, warm = args.blocks, args.per, 12
    sampling = Sampling.parse(args.sampling)
    dev = torch.device("cuda", 0)
    cfg = bench.make_config("llama3-8b-262k")
    gamma = len(bench.TREE)
    max_gen = (gamma + 2) * (blocks * (per + 1) + warm + 8) + 16      # a round emits at most gamma + 2 tokens
    m = bench.build_model(cfg, dev, 0.02, seed=1234)
    m.GRAPH_AFTER = 0
    m.set_max_gen_len(max_gen + 256)
    m.glide.set_max_gen_len(max_gen + 256)
    bench.synth_kv(m, PREFIX, PREFIX, max_gen + 256, dev, seed=4321)
    lens = torch.tensor([PREFIX], dtype=torch.int32, device=dev)
    first = torch.tensor([1000], dtype=torch.int64, device=dev)
    random.seed(99)
    torch.manual_seed(99)
    more = {f"sampled[{spec}]": (Sampling.parse(spec.partition(";")[0]), Cut.parse(spec.partition(";")[2]) if ";" in spec else None)
            for spec in args.more}
    arms = ARMS + tuple(more)
    t = {a: [] for a in arms}

    def one_round(arm, st):
        if arm != "stochastic":
            assert m.tree_round(st), "the token budget of the run is used up"
            return
        # random weights now and then accept gamma + 2 tokens, which do not fit the next verification batch (the generate
        # loop raises there, as the reference does): a timing run goes on with gamma + 1 of them
        if st.a + st.Fn - 1 > st.R:
            st.a = st.gamma + 1
            st.acc_ids = st.acc_pad[:, :st.a]
        assert m.tree_round_stochastic(st), "the token budget of the run is used up"

    with torch.inference_mode():
        states = {"greedy": m.begin_tree_decode(first, lens, PREFIX, bench.TREE, max_gen, eos_id=-1),
                  "sampled": m.begin_tree_decode(first, lens, PREFIX, bench.TREE, max_gen, eos_id=-1, sampling=sampling),
                  "stochastic": m.begin_tree_decode(first, lens, PREFIX, bench.TREE, max_gen, eos_id=-1, temperature=TEMPERATURE)}
        for arm, (s, c) in more.items():
            states[arm] = m.begin_tree_decode(first, lens, PREFIX, bench.TREE, max_gen, eos_id=-1, sampling=s, cut=c)
        assert states["greedy"].sampling is None, "unset LONGSPEC_SAMPLING: the greedy arm must be greedy"
        for arm, st in states.items():                 # every shape an arm uses, and the captures, before the clock
            st.eos = None
            assert st.use_graphs, "the graph path is off on this device"
            if arm != "stochastic":
                m.prepare_tree_graphs(st)
            for _ in range(warm):
                one_round(arm, st)
        for b in range(blocks):
            for arm, st in states.items():
                one_round(arm, st)
                torch.cuda.synchronize()
                captures = st.graph_captures
                t0 = time.perf_counter()
                for _ in range(per):
                    one_round(arm, st)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / per * 1e3
                if st.graph_captures != captures:      # a block that paid for a capture (a first-seen accepted count)
                    print(f"block {b} {arm}: {ms:.3f} ms/round with {st.graph_captures - captures} capture(s) inside, dropped")
                    continue
                t[arm].append(ms)
        for arm, st in states.items():
            assert st.graphs is not False, f"the {arm} arm fell back to eager rounds during the run"

    def stats(v):
        v = sorted(v)
        return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "blocks_ms": [round(x, 4) for x in v],
                "spread": (v[-1] - v[0]) / v[len(v) // 2]}

    res = {a: stats(t[a]) for a in arms}
    spread = max(r["spread"] for r in res.values())
    g = res["greedy"]["median_ms"]
    out = {"what": "ms per tree round replayed from HIP graphs: greedy, sampled (sampling=) and the reference-style temperature > 0 "
                   "round, interleaved blocks on one box",
           "model": "llama3-8b dims, random weights", "prefix_tokens": PREFIX, "tree_shape": list(bench.TREE),
           "sampling": repr(sampling), "stochastic_temperature": TEMPERATURE, "rounds_per_block": per,
           "device": torch.cuda.get_device_name(0), **res, "same_box_spread": spread,
           "sampled_over_greedy": res["sampled"]["median_ms"] / g, "stochastic_over_greedy": res["stochastic"]["median_ms"] / g,
           "sampled_within_2_percent_of_greedy": res["sampled"]["median_ms"] <= g * 1.02,
           "more_over_sampled": {a: res[a]["median_ms"] / res["sampled"]["median_ms"] for a in more}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
