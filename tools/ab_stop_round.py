"""A/B timing of the tree round with ``stop=`` on ONE box: blocks of the plain greedy round (``stop=None``: the device code of
the round as it was before stop conditions existed -- the yardstick), the round with ``Stop(2 ids, 4 sequences of 4 tokens)``
and the same with ``min_tokens`` beyond the run, so that the ban launch is live in every round, alternate, all replayed from HIP
graphs, on the synthetic-KV setting of bench.py (Llama-3-8B dimensions, 16k-token prefix, tree 4 16 16 16 16).  Writes
profiles/stop_round_ab.json.

    python tools/ab_stop_round.py [--blocks 6] [--per 15]

Each figure is a host clock around `per` rounds that end in a device synchronise; the spread is what the blocks of ONE arm
differ by on this box in this run, the yardstick for the difference between the arms.  The arms keep their own decode state
over the same synthetic caches; the stops name ids at the very end of the vocabulary, and a round that stops ends the run
loudly."""
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
from longspec_amd import Stop  # noqa: E402

PREFIX = 16384
ARMS = ("plain", "stop", "stop_min_tokens")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stop_round_ab.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    blocks, per, warm = args.blocks, args.per, 12
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
    V = m.lm_head.out_features
    ids = [V - 1, V - 2]
    seqs = [[V - 3 - q] * 4 for q in range(4)]
    random.seed(99)
    torch.manual_seed(99)
    t = {a: [] for a in ARMS}

    def one_round(arm, st):
        assert m.tree_round(st), f"{arm}: the token budget of the run is used up, or a stop matched"

    with torch.inference_mode():
        begin = lambda **kw: m.begin_tree_decode(first, lens, PREFIX, bench.TREE, max_gen, eos_id=-1, **kw)
        states = {"plain": begin(), "stop": begin(stop=Stop(ids, seqs)), "stop_min_tokens": begin(stop=Stop(ids, seqs, max_gen + 1))}
        assert all(st.sampling is None and st.penalties is None and st.logprobs is None for st in states.values()) \
            and states["plain"].stop is None, \
            "unset LONGSPEC_SAMPLING / LONGSPEC_PENALTIES / LONGSPEC_LOGPROBS / LONGSPEC_STOP: the yardstick arm must be plain"
        for arm, st in states.items():                 # every shape an arm uses, and the captures, before the clock
            st.eos = None
            assert st.use_graphs, "the graph path is off on this device"
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
            assert st.stop is None or st.last_stop.length.tolist() == [-1], f"{arm}: a stop matched"

    def stats(v):
        v = sorted(v)
        return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "blocks_ms": [round(x, 4) for x in v],
                "spread": (v[-1] - v[0]) / v[len(v) // 2]}

    res = {a: stats(t[a]) for a in ARMS}
    spread = max(r["spread"] for r in res.values())
    g = res["plain"]["median_ms"]
    out = {"what": "ms per greedy tree round replayed from HIP graphs: plain, with stop=Stop(2 ids, 4 x 4-token sequences) and the "
                   "same with min_tokens beyond the run (the ban launch live), interleaved blocks on one box",
           "model": "llama3-8b dims, random weights", "prefix_tokens": PREFIX, "tree_shape": list(bench.TREE),
           "rounds_per_block": per,
           "device": torch.cuda.get_device_name(0), **res, "same_box_spread": spread,
           "stop_over_plain": res["stop"]["median_ms"] / g,
           "stop_min_tokens_over_plain": res["stop_min_tokens"]["median_ms"] / g}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
