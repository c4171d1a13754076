"""A/B timing of the tree round with ``ban=`` on ONE box, and the kernel time of ``ls_ban_rows`` next to ``ls_argmax_rows``.

    python tools/ab_ban_round.py [--blocks 6] [--per 15] [--out profiles/ban_ab.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/ab_ban_round.py --kernels            (a run of its own)
    python tools/ab_ban_round.py --summarise <db> [--out profiles/ban_ab.json]                     (adds "kernels" to the file)

The A/B: blocks of the plain greedy round (``ban=None``: the device code of the round as it was before the keyword existed -- the
yardstick) and of the round with ``Ban(no_repeat_ngram=4)`` plus 8 sequences of 4 tokens alternate, all replayed from HIP graphs,
on the synthetic-KV setting of bench.py (Llama-3-8B dimensions, 16k-token prefix, tree 4 16 16 16 16), once with about 1k and once
with about 20k generated columns behind them: the states start at that width over random committed ids (no 4-gram of which
repeats), the plain arm too, so that both arms of a pair size their launches alike.  Each figure is a host clock around `per`
rounds that end in a device synchronise; the spread is what the blocks of ONE arm differ by on this box in this run."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PREFIX = 16384
WIDTHS = (1024, 20480)
V, ROWS, WARM, CALLS = 128256, 69, 5, 50


def the_ban(vocab):
    from longspec_amd import Ban
    return Ban(sequences=[[vocab - 1 - q] * 4 for q in range(8)], no_repeat_ngram=4)


def rounds(args):
    import torch
    import bench
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    blocks, per, warm = args.blocks, args.per, 12
    dev = torch.device("cuda", 0)
    cfg = bench.make_config("llama3-8b-262k")
    gamma = len(bench.TREE)
    budget = (gamma + 2) * (blocks * (per + 1) + warm + 8) + 16         # a round emits at most gamma + 2 tokens
    max_gen = max(WIDTHS) + budget
    m = bench.build_model(cfg, dev, 0.02, seed=1234)
    m.GRAPH_AFTER = 0
    m.set_max_gen_len(max_gen + 256)
    m.glide.set_max_gen_len(max_gen + 256)
    bench.synth_kv(m, PREFIX, PREFIX, max_gen + 256, dev, seed=4321)
    lens = torch.tensor([PREFIX], dtype=torch.int32, device=dev)
    first = torch.tensor([1000], dtype=torch.int64, device=dev)
    vocab = m.lm_head.out_features
    ban = the_ban(vocab)
    g = torch.Generator().manual_seed(99)
    text = torch.randint(0, vocab - 16, (1, max(WIDTHS)), generator=g).to(dev)
    arms = [(f"{kind}_{w}", kind, w) for w in WIDTHS for kind in ("plain", "ban")]
    t = {a[0]: [] for a in arms}

    def one_round(arm, st):
        assert m.tree_round(st), f"{arm}: the token budget of the run is used up"

    with torch.inference_mode():
        states = {}
        for arm, kind, w in arms:
            st = m.begin_tree_decode(first, lens, PREFIX, bench.TREE, w + budget, eos_id=-1, ban=ban if kind == "ban" else None)
            assert st.sampling is None and st.penalties is None and st.logprobs is None and st.stop is None \
                and (st.ban is None) == (kind == "plain"), "unset the LONGSPEC_* defaults: the yardstick arm must be plain"
            st.output_ids[:, :w] = text[:, :w]                            # w columns are written: the width the ban scans
            st.output_ids[:, w - 1] = first
            st.emitted_dev.fill_(w)
            st.emitted = w
            st.eos = None
            assert st.use_graphs, "the graph path is off on this device"
            m.prepare_tree_graphs(st)
            for _ in range(warm):
                one_round(arm, st)
            states[arm] = st
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
        widths_end = {arm: st.emitted for arm, st in states.items()}

    def stats(v):
        v = sorted(v)
        return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "blocks_ms": [round(x, 4) for x in v],
                "spread": (v[-1] - v[0]) / v[len(v) // 2]}

    res = {a: stats(t[a]) for a in t}
    out = {"what": "ms per greedy tree round replayed from HIP graphs: plain, and with ban=Ban(no_repeat_ngram=4, 8 x 4-token "
                   "sequences), at about 1k and about 20k generated columns, interleaved blocks on one box",
           "model": "llama3-8b dims, random weights", "prefix_tokens": PREFIX, "tree_shape": list(bench.TREE), "rounds_per_block": per,
           "device": torch.cuda.get_device_name(0), "rounds": res, "generated_columns_at_the_end": widths_end,
           "same_box_spread": max(r["spread"] for r in res.values())}
    for w in WIDTHS:
        out[f"ban_over_plain_{w}"] = res[f"ban_{w}"]["median_ms"] / res[f"plain_{w}"]["median_ms"]
    return out


def kernels():
    """The traced workload: ops.ban_rows on fp16 logits [69, 128256] whose rows follow a 4/16/16/16/16-shaped level-major tree, over
    1k and then 20k committed columns, and ops.argmax_rows on the same logits."""
    import torch
    from longspec_amd import ops
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(1, ROWS, V, generator=g) * 3).to(torch.float16).cuda()
    table = the_ban(V).table(V, "cuda")
    text = torch.randint(0, V - 16, (1, max(WIDTHS) + 64), generator=g).cuda()
    ids = torch.randint(0, V - 16, (1, ROWS - 1), generator=g).cuda()
    mask = torch.zeros((1, ROWS, ROWS - 1), dtype=torch.int64)
    parent = [0] * ROWS
    level, nodes = [0], 1
    for width in (4, 16, 16, 16, 16):
        new = []
        for j in range(width):
            parent[nodes] = level[j % len(level)]
            new.append(nodes)
            nodes += 1
        level = new
    for r in range(1, ROWS):
        mask[0, r] = mask[0, parent[r]]
        mask[0, r, r - 1] = 1
    mask = mask.cuda()
    for w in WIDTHS:
        base = torch.tensor([w], dtype=torch.int32, device="cuda")
        for _ in range(WARM + CALLS):
            ops.ban_rows(x, table, text, base=base, extra_ids=ids, extra_mask=mask)
        torch.cuda.synchronize()
    x = (torch.randn(1, ROWS, V, generator=g) * 3).to(torch.float16).cuda()
    for _ in range(WARM + CALLS):
        ops.argmax_rows(x)
    torch.cuda.synchronize()


def summarise(db, out):
    import sqlite3
    c = sqlite3.connect(db)
    tables = [r[0] for r in c.execute("select name from sqlite_master where type='table'")]
    disp = [t for t in tables if t.startswith("rocpd_kernel_dispatch")][0]
    sym = [t for t in tables if t.startswith("rocpd_info_kernel_symbol")][0]
    cols = [r[1] for r in c.execute(f"pragma table_info({sym})")]
    name_col = "display_name" if "display_name" in cols else ("kernel_name" if "kernel_name" in cols else "name")
    per = {}                                                              # launches in time order: the widths come one after the other
    for name, start, end in c.execute(f"select s.{name_col}, d.start, d.end from {disp} d join {sym} s on d.kernel_id = s.id order by d.start"):
        per.setdefault(name, []).append((end - start) / 1e3)
    med = lambda v: round(sorted(v)[len(v) // 2], 2)
    res = {"what": f"rocprofv3 --kernel-trace --stats, a run of its own: median microseconds of the last {CALLS} launches at "
                   f"fp16 [{ROWS}, {V}], Ban(no_repeat_ngram=4, 8 x 4-token sequences), rows on a 4/16/16/16/16 tree"}
    for name, v in per.items():
        if "ban_rows_kernel" in name:
            assert len(v) == len(WIDTHS) * (WARM + CALLS), len(v)
            for i, w in enumerate(WIDTHS):
                res[f"ls_ban_rows_us_{w}_columns"] = med(v[i * (WARM + CALLS) + WARM:(i + 1) * (WARM + CALLS)])
        elif len(v) >= WARM + CALLS:                                      # the kernels of ops.argmax_rows (torch's fills are fewer)
            import re
            k = re.search(r"(\w+_kernel)(<[^>]*>)?", name)
            res.setdefault("ls_argmax_rows_kernels_us", {})[k.group(0) if k else name[:60]] = med(v[-CALLS:])
    res["ls_argmax_rows_us"] = round(sum(res.get("ls_argmax_rows_kernels_us", {}).values()), 2)
    data = {}
    if os.path.exists(out):
        with open(out) as f:
            data = json.load(f)
    data["kernels"] = res
    with open(out, "w") as f:
        json.dump(data, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per", type=int, default=15)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--summarise", metavar="DB")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ban_ab.json"))
    args = ap.parse_args()
    if args.kernels:
        kernels()
        return 0
    if args.summarise:
        summarise(args.summarise, args.out)
        return 0
    out = rounds(args)
    data = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            data = json.load(f)
    data.update(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(data, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
