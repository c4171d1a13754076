"""A/B timing of the temperature > 0 tree round on ONE box: blocks of rounds replayed from HIP graphs
(LlamaGlide.GRAPH_STOCHASTIC) alternate with blocks issued launch by launch, on the synthetic-KV setting of bench.py
(Llama-3-8B dimensions, 16k-token prefix, tree 4 16 16 16 16, T = 0.8).  Writes profiles/stochastic_round_ab.json.

    python tools/ab_stochastic_round.py [--blocks 6] [--per 15]

Each figure is a host clock around `per` rounds that end in a device synchronise; the spread is what the blocks of ONE arm
differ by on this box in this run, the yardstick for the difference between the arms."""
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

PREFIX, TEMPERATURE = 16384, 0.8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stochastic_round_ab.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    blocks, per, warm = args.blocks, args.per, 12
    dev = torch.device("cuda", 0)
    cfg = bench.make_config("llama3-8b-262k")
    gamma = len(bench.TREE)
    max_gen = (gamma + 2) * (2 * blocks * (per + 1) + 2 * warm + 8) + 16      # a round emits at most gamma + 2 tokens
    m = bench.build_model(cfg, dev, 0.02, seed=1234)
    m.GRAPH_AFTER = 0
    m.set_max_gen_len(max_gen + 256)
    m.glide.set_max_gen_len(max_gen + 256)
    bench.synth_kv(m, PREFIX, PREFIX, max_gen + 256, dev, seed=4321)
    lens = torch.tensor([PREFIX], dtype=torch.int32, device=dev)
    first = torch.tensor([1000], dtype=torch.int64, device=dev)
    random.seed(99)
    torch.manual_seed(99)
    t = {True: [], False: []}
    accepted = {True: 0, False: 0}

    def one_round(st):
        # random weights now and then accept gamma + 2 tokens, which do not fit the next verification batch (the generate
        # loop raises there, as the reference does): a timing run goes on with gamma + 1 of them
        if st.a + st.Fn - 1 > st.R:
            st.a = st.gamma + 1
            st.acc_ids = st.acc_pad[:, :st.a]
        assert m.tree_round_stochastic(st), "the token budget of the run is used up"

    with torch.inference_mode():
        st = m.begin_tree_decode(first, lens, PREFIX, bench.TREE, max_gen, eos_id=-1, temperature=TEMPERATURE)
        st.eos = None
        assert st.use_graphs, "the graph path is off on this device"
        for flag in (True, False):                     # every shape both arms use, and the captures, before the clock
            st.use_graphs = flag
            for _ in range(warm):
                one_round(st)
        for b in range(blocks):
            for flag in (True, False):
                st.use_graphs = flag
                one_round(st)
                torch.cuda.synchronize()
                before, captures = st.emitted, st.graph_captures
                t0 = time.perf_counter()
                for _ in range(per):
                    one_round(st)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / per * 1e3
                if st.graph_captures != captures:      # a block that paid for a capture (a first-seen accepted count)
                    print(f"block {b} graph={flag}: {ms:.3f} ms/round with {st.graph_captures - captures} capture(s) inside, dropped")
                    continue
                t[flag].append(ms)
                accepted[flag] += st.emitted - before
        assert st.graphs is not False, "the graph path fell back to eager rounds during the run"

    def stats(v):
        v = sorted(v)
        return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "blocks_ms": [round(x, 4) for x in v],
                "spread": (v[-1] - v[0]) / v[len(v) // 2]}

    eager, graph = stats(t[False]), stats(t[True])
    spread = max(eager["spread"], graph["spread"])
    out = {"what": "ms per temperature > 0 tree round, graph replay vs launch by launch, interleaved blocks on one box",
           "model": "llama3-8b dims, random weights", "prefix_tokens": PREFIX, "tree_shape": list(bench.TREE),
           "temperature": TEMPERATURE, "rounds_per_block": per, "device": torch.cuda.get_device_name(0),
           "eager": eager, "graph": graph, "speedup": eager["median_ms"] / graph["median_ms"], "same_box_spread": spread,
           "tokens_per_round": {"eager": accepted[False] / (per * len(t[False])), "graph": accepted[True] / (per * len(t[True]))},
           "graph_captures": st.graph_captures,
           "graph_not_slower": graph["median_ms"] <= eager["median_ms"] * (1.0 + spread)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0 if out["graph_not_slower"] else 1


if __name__ == "__main__":
    sys.exit(main())
