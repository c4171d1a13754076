"""A/B timing of the prompt-lookup TREE round against the chain round and the vanilla step on ONE box: blocks of the graphed
vanilla step, of ``lookup_round`` at gamma 7 and 15 (the chain) and of ``lookup_round`` at gamma 7 with 2, 4 and 8 branches
alternate, all replayed from HIP graphs, on Llama-3-8B dimensions over synthetic KV at a 16k- and a 128k-token prefix.  Writes
profiles/lookup_tree_ab.json.

    python tools/ab_lookup_tree.py [--blocks 5] [--per 20] [--replay profiles/lookup_tree_replay.json]

Each figure is a host clock around `per` steps / rounds that end in a device synchronise; the spread is what the blocks of ONE
arm differ by on this box in this run, the yardstick for the difference between the arms.  Reported: ms per round, the
break-even acceptance ``t_round / t_step`` and the cost ratio ``t_tree(B) / t_chain(gamma 7)``; with ``--replay`` (the output of
tools/lookup_replay.py) the token ratio ``tokens_per_round(B) / tokens_per_round(1)`` of every replayed text is set next to the
cost ratio.  On random weights and a random prompt every round accepts one token, so the tree rounds timed are those of
``a = 1``; the pass has its R rows whatever ``a`` is.  The acceptance itself is not quoted from this run."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

PREFIXES = (16384, 131072)
GAMMA = 7
CHAINS = (7, 15)
BRANCHES = (2, 4, 8)
ARMS = ("vanilla",) + tuple(f"chain_g{g}" for g in CHAINS) + tuple(f"tree_g{GAMMA}_b{b}" for b in BRANCHES)


def stats(v):
    v = sorted(v)
    return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "blocks_ms": [round(x, 4) for x in v],
            "spread": (v[-1] - v[0]) / v[len(v) // 2]}


def measure(m, prefix, blocks, per, warm, dev):
    calls = blocks * (per + 1) + warm + 8
    max_gen = (max(CHAINS) + 1) * calls + 64                          # a round emits at most gamma + 1 tokens
    m.set_max_gen_len(max_gen + 256)
    bench.synth_kv(m, prefix, prefix, max_gen + 256, dev, seed=4321)
    lens = torch.tensor([prefix], dtype=torch.int32, device=dev)
    first = torch.tensor([1000], dtype=torch.int64, device=dev)
    g = torch.Generator().manual_seed(7)
    prompt = torch.randint(0, 50_000, (1, prefix), generator=g).to(dev)
    out_v = torch.zeros((1, calls + 8), dtype=torch.int64, device=dev)
    out_v[:, 0] = first
    states = {"vanilla": m.begin_vanilla_decode(out_v, lens.clone(), lens.clone(), prefix)}
    for gamma in CHAINS:
        states[f"chain_g{gamma}"] = m.begin_lookup_decode(first, lens.clone(), lens.clone(), prefix, prompt, gamma=gamma,
                                                          max_gen_len=max_gen, eos_id=-1)
    for b in BRANCHES:
        states[f"tree_g{GAMMA}_b{b}"] = m.begin_lookup_decode(first, lens.clone(), lens.clone(), prefix, prompt, gamma=GAMMA,
                                                              max_gen_len=max_gen, eos_id=-1, branches=b)
    for arm, st in states.items():
        assert st.sampling is None and st.penalties is None and st.logprobs is None and st.stop is None, \
            "unset LONGSPEC_SAMPLING / LONGSPEC_PENALTIES / LONGSPEC_LOGPROBS / LONGSPEC_STOP: the arms must be plain"
        assert st.use_graphs, "the graph path is off on this device"
        if arm != "vanilla":
            st.eos = None

    def one(arm, st):
        if arm == "vanilla":
            m.vanilla_step(st)
        else:
            assert m.lookup_round(st), f"{arm}: the token budget of the run is used up"

    t = {a: [] for a in ARMS}
    for arm, st in states.items():                                    # the capture, before the clock
        for _ in range(warm):
            one(arm, st)
    for blk in range(blocks):
        for arm, st in states.items():
            one(arm, st)
            torch.cuda.synchronize()
            captures = st.graph_captures
            t0 = time.perf_counter()
            for _ in range(per):
                one(arm, st)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / per * 1e3
            if st.graph_captures != captures:                         # a block that paid for a capture (a new tier, a new `a`)
                print(f"block {blk} {arm}: {ms:.3f} ms with {st.graph_captures - captures} capture(s) inside, dropped")
                continue
            t[arm].append(ms)
    for arm, st in states.items():
        assert st.graphs is not False and st.graph_captures > 0, f"the {arm} arm fell back to eager launches during the run"
    res = {a: stats(t[a]) for a in ARMS}
    step, chain = res["vanilla"]["median_ms"], res[f"chain_g{GAMMA}"]["median_ms"]
    res["same_box_spread"] = max(res[a]["spread"] for a in ARMS)
    res["break_even_tokens_per_round"] = {a: res[a]["median_ms"] / step for a in ARMS if a != "vanilla"}
    res["cost_ratio_to_chain_g7"] = {a: res[a]["median_ms"] / chain for a in ARMS if a.startswith("tree")}
    res["verification_rows"] = {a: states[a].R for a in ARMS if a.startswith("tree")}
    res["hist_nb"] = {a: states[a].hist_nb[0].tolist() for a in ARMS if a.startswith("tree")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--per", type=int, default=20)
    ap.add_argument("--replay", default=None, help="json of tools/lookup_replay.py: its token ratios are set next to the cost ratios")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_tree_ab.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda", 0)
    cfg = bench.make_config("llama3-8b-262k")
    m = bench.build_model(cfg, dev, 0.02, seed=1234)
    m.GRAPH_AFTER = 0
    torch.manual_seed(99)
    out = {"what": "ms per graphed vanilla step, per prompt-lookup chain round (gamma 7 / 15) and per tree round (gamma 7, 2 / 4 / 8 "
                   "branches; max_ngram 3, min_ngram 1), replayed from HIP graphs, interleaved blocks on one box; "
                   "break_even_tokens_per_round = t_round / t_step; cost_ratio_to_chain_g7 = t_tree / t_chain(gamma 7)",
           "model": "llama3-8b dims, random weights, random prompt ids", "rounds_per_block": args.per,
           "device": torch.cuda.get_device_name(0)}
    with torch.inference_mode():
        for prefix in PREFIXES:
            out[f"prefix_{prefix}"] = measure(m, prefix, args.blocks, args.per, 12, dev)
            print(json.dumps({prefix: out[f"prefix_{prefix}"]}), flush=True)
    if args.replay:
        with open(args.replay) as f:
            replay = json.load(f)
        out["token_ratio_to_branches_1"] = {
            name: {f"tree_g{GAMMA}_b{b}": r["tokens_per_round"][str(b)] / r["tokens_per_round"]["1"] for b in BRANCHES}
            for name, r in replay["texts"].items()}
        out["token_ratio_source"] = replay["what"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
