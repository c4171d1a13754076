"""Time ``ops.watermark_rows`` next to ``ops.penalize_rows``, ``ops.guide_rows`` and ``ops.argmax_rows`` at [69, 128 256] fp16 (rows
that follow a 4/16/16/16/16-shaped level-major tree over 1 024 generated columns), and ``ops.watermark_score`` at n = 1 024 and
131 072.  Event timing: the median over blocks of 50 back-to-back calls, launch overhead included.  With ``--rounds``: the
greedy tree round under ``watermark=`` against the plain round, interleaved blocks on one box, on the synthetic-KV setting of
bench.py (Llama-3-8B dimensions, 16k-token prefix), replayed from HIP graphs.

    python tools/prof_watermark.py [--json out.json]
    python tools/prof_watermark.py --rounds [--blocks 6] [--per 15] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from longspec_amd import Guide, Penalties, Watermark, ops  # noqa: E402

R, V, CALLS, BLOCKS, PREFIX = 69, 128256, 50, 7, 16384


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(BLOCKS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / CALLS)
    return {"median_us": round(statistics.median(out), 2), "min_us": round(min(out), 2), "max_us": round(max(out), 2)}


def tree_mask():
    mask = torch.zeros((R, R - 1), dtype=torch.int64)
    parent, level, nodes = [0] * R, [0], 1
    for width in (4, 16, 16, 16, 16):
        new = []
        for j in range(width):
            parent[nodes] = level[j % len(level)]
            new.append(nodes)
            nodes += 1
        level = new
    for r in range(1, R):
        mask[r] = mask[parent[r]]
        mask[r, r - 1] = 1
    return mask


def kernels():
    dev = "cuda"
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn((1, R, V), generator=g) * 3).to(torch.float16).to(dev)
    mask = tree_mask().to(dev)
    w = 1024
    out = torch.randint(0, 32000, (1, w + 8), generator=g).to(dev)
    ids = torch.randint(0, 32000, (1, R - 1), generator=g).to(dev)
    base = torch.tensor([w], dtype=torch.int32, device=dev)
    res = {"what": __doc__.split("\n\n")[0], "rows": R, "vocab": V, "calls_per_block": CALLS, "blocks": BLOCKS,
           "device": torch.cuda.get_device_name(0), "bytes_read_per_call": 2 * R * V, "rows_kernels": {}, "score": {}}
    x = logits.clone()
    case = res["rows_kernels"]
    for name, wm in (("gamma_0.25_ctx_1", Watermark(1, 0.25, 2.0)), ("gamma_0.5_ctx_8", Watermark(1, 0.5, 2.0, context=8))):
        table = wm.table(V, dev)
        case[f"watermark_rows_{name}"] = timed(lambda: ops.watermark_rows(x, table, out, base=base, extra_ids=ids, extra_mask=mask))
        x.copy_(logits)
    never = Watermark(1, 0.25, 2.0, context=8).table(V, dev)              # w = 0 and no path: every row returns before the sweep
    case["watermark_rows_unmarked"] = timed(lambda: ops.watermark_rows(x, never, None))
    state = torch.zeros((1, V), dtype=torch.int32)
    state[0, torch.randperm(V, generator=g)[:2048]] = 1
    state = state.to(dev)
    pen = Penalties(1.1, 0.5, 0.2)
    case["penalize_rows"] = timed(lambda: ops.penalize_rows(x, state, pen, ids, mask))
    x.copy_(logits)
    guide = Guide([[0, 0]], torch.arange(V).numpy() % 2)                  # one state, nothing forbidden: the rows are streamed
    gtable, gstate = guide.table(V, dev), torch.zeros((1,), dtype=torch.int32, device=dev)
    case["guide_rows"] = timed(lambda: ops.guide_rows(x, gtable, gstate, extra_ids=ids, extra_mask=mask))
    case["argmax_rows"] = timed(lambda: ops.argmax_rows(x))
    for k, v in case.items():
        print(f"{k}: {v['median_us']} us ({v['min_us']} .. {v['max_us']})", flush=True)
    wm = Watermark(1, 0.25, 2.0, context=4)
    table = wm.table(V, dev)
    for n in (1024, 131072):
        doc = torch.randint(0, V, (1, n), generator=g).to(dev)
        res["score"][f"n_{n}"] = timed(lambda: ops.watermark_score(doc, table))
        res["score"][f"n_{n}_counts_only"] = timed(lambda: ops.watermark_score(doc, table, want_flags=False))
        print(f"watermark_score n={n}: {res['score'][f'n_{n}']['median_us']} us with flags, "
              f"{res['score'][f'n_{n}_counts_only']['median_us']} us counts only (allocations of the outputs included)", flush=True)
    return res


def rounds(blocks, per):
    import bench
    warm = 12
    dev = torch.device("cuda", 0)
    cfg = bench.make_config("llama3-8b-262k")
    gamma = len(bench.TREE)
    max_gen = (gamma + 2) * (blocks * (per + 1) + warm + 8) + 16            # a round emits at most gamma + 2 tokens
    m = bench.build_model(cfg, dev, 0.02, seed=1234)
    m.GRAPH_AFTER = 0
    m.set_max_gen_len(max_gen + 256)
    m.glide.set_max_gen_len(max_gen + 256)
    bench.synth_kv(m, PREFIX, PREFIX, max_gen + 256, dev, seed=4321)
    lens = torch.tensor([PREFIX], dtype=torch.int32, device=dev)
    first = torch.tensor([998], dtype=torch.int64, device=dev)
    arms = {"plain": None, "watermark": Watermark(1, 0.25, 2.0)}
    t = {a: [] for a in arms}
    with torch.inference_mode():
        states = {}
        for arm, wm in arms.items():
            st = m.begin_tree_decode(first, lens, PREFIX, bench.TREE, max_gen, eos_id=-1, watermark=wm)
            assert st.sampling is None and st.penalties is None and st.logprobs is None and st.stop is None and st.ban is None \
                and st.guide is None and st.dry is None and (st.watermark is None) == (wm is None), \
                "unset the LONGSPEC_* defaults: the yardstick arm must be plain"
            st.eos = None
            assert st.use_graphs, "the graph path is off on this device"
            m.prepare_tree_graphs(st)
            for _ in range(warm):
                assert m.tree_round(st)
            states[arm] = st
        emitted0 = {arm: st.emitted for arm, st in states.items()}
        count = {arm: 0 for arm in arms}
        for b in range(blocks):
            for arm, st in states.items():
                assert m.tree_round(st)
                torch.cuda.synchronize()
                captures = st.graph_captures
                t0 = time.perf_counter()
                for _ in range(per):
                    assert m.tree_round(st), f"{arm}: the token budget of the run is used up"
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / per * 1e3
                count[arm] += per + 1
                if st.graph_captures != captures:      # a block that paid for a capture (a first-seen accepted count)
                    print(f"block {b} {arm}: {ms:.3f} ms/round with {st.graph_captures - captures} capture(s) inside, dropped")
                    continue
                t[arm].append(ms)
        for arm, st in states.items():
            assert st.graphs is not False, f"the {arm} arm fell back to eager rounds during the run"
        tokens = {arm: (st.emitted - emitted0[arm]) / count[arm] for arm, st in states.items()}

    def stats(v):
        v = sorted(v)
        return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "blocks_ms": [round(x, 4) for x in v],
                "spread": (v[-1] - v[0]) / v[len(v) // 2]}

    res = {a: stats(v) for a, v in t.items()}
    return {"what": "ms per greedy tree round replayed from HIP graphs: plain and under Watermark(1, 0.25, 2.0), interleaved blocks "
                    "on one box", "model": "llama3-8b dims, random weights", "prefix_tokens": PREFIX, "tree_shape": list(bench.TREE),
            "rounds_per_block": per, "device": torch.cuda.get_device_name(0), "rounds": res, "tokens_per_round": tokens,
            "same_box_spread": max(r["spread"] for r in res.values()),
            "watermark_over_plain": res["watermark"]["median_ms"] / res["plain"]["median_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--rounds", action="store_true")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per", type=int, default=15)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    res = rounds(args.blocks, args.per) if args.rounds else kernels()
    if args.rounds:
        print(json.dumps({k: v for k, v in res.items() if k != "what"}, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
