"""A/B timing of the tree round with ``guide=`` on ONE box, and the kernel times of ``ls_guide_rows`` / ``ls_guide_advance`` next
to ``ls_argmax_rows``.

    python tools/ab_guide_round.py [--blocks 6] [--per 15] [--out profiles/guide_ab.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/ab_guide_round.py --kernels            (a run of its own)
    python tools/ab_guide_round.py --summarise <db> [--tag slice_8192] [--out profiles/guide_ab.json]
    python tools/ab_guide_round.py --build-slices            (no GPU: the measurement builds of csrc/guide.hip, one per slice size)

The A/B: blocks of the plain greedy round (``guide=None``: the device code of the round as it was before the keyword existed -- the
yardstick), of the round under a 2-state guide that forbids half of the vocabulary in either state (even and odd ids alternate)
and of the round under a guide that forbids all but 1 000 ids alternate, all replayed from HIP graphs, on the synthetic-KV setting
of bench.py (Llama-3-8B dimensions, 16k-token prefix, tree 4 16 16 16 16).  Each figure is a host clock around `per` rounds that
end in a device synchronise; the spread is what the blocks of ONE arm differ by on this box in this run.  The arms accept
differently (a guided target rejects most drafts of an unguided drafter), so the tokens per round are kept next to the times.

The kernels: ``--kernels`` is the traced workload, ``--summarise`` reads the trace.  With LONGSPEC_HIP_LIB set to one of the
``--build-slices`` libraries the same workload measures another vocabulary slice per workgroup (``--tag`` keeps the results
apart)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PREFIX = 16384
V, ROWS, WARM, CALLS, ADVANCE_N = 128256, 69, 5, 50, 17
SLICES = (4096, 16384, 32768, 65536)        # next to the product's LS_GUIDE_SLICE (8192)
KERNEL_GUIDES = ("half", "1k", "c16384", "half_no_path")


def the_guide(kind, vocab):
    import numpy as np
    from longspec_amd import Guide
    v = np.arange(vocab)
    if kind == "half":                    # 2 states, each forbids half of the vocabulary: every group of eight ids is mixed
        return Guide([[1, -1], [-1, 0]], v % 2)
    if kind == "1k":                      # all but 1 000 ids forbidden: the store stream
        return Guide([[0]], np.where(v < 1000, 0, -1))
    assert kind == "c16384"               # C = 16384, S = 1024: a 64 MB transition area, half of it -1
    rng = np.random.default_rng(16384)
    nx = rng.integers(0, 1024, size=(1024, 16384), dtype=np.int32)
    nx[rng.integers(0, 2, size=nx.shape, dtype=np.int8) == 0] = -1
    nx[:, :2] = ((np.arange(1024) + 1) % 1024)[:, None]
    return Guide(nx, v % 16384)


def rounds(args):
    import torch
    import bench
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    blocks, per, warm = args.blocks, args.per, 12
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
    first = torch.tensor([998], dtype=torch.int64, device=dev)             # (legal under both guides)
    vocab = m.lm_head.out_features
    arms = ["plain", "half", "1k"]
    t = {a: [] for a in arms}

    def one_round(arm, st):
        assert m.tree_round(st), f"{arm}: the token budget of the run is used up"

    with torch.inference_mode():
        states = {}
        for arm in arms:
            guide = None if arm == "plain" else the_guide(arm, vocab)
            st = m.begin_tree_decode(first, lens, PREFIX, bench.TREE, max_gen, eos_id=-1, guide=guide)
            assert st.sampling is None and st.penalties is None and st.logprobs is None and st.stop is None and st.ban is None \
                and (st.guide is None) == (arm == "plain"), "unset the LONGSPEC_* defaults: the yardstick arm must be plain"
            st.eos = None
            assert st.use_graphs, "the graph path is off on this device"
            m.prepare_tree_graphs(st)
            for _ in range(warm):
                one_round(arm, st)
            states[arm] = st
        emitted0 = {arm: st.emitted for arm, st in states.items()}
        timed = {arm: 0 for arm in arms}
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
                timed[arm] += per + 1
                if st.graph_captures != captures:      # a block that paid for a capture (a first-seen accepted count)
                    print(f"block {b} {arm}: {ms:.3f} ms/round with {st.graph_captures - captures} capture(s) inside, dropped")
                    continue
                t[arm].append(ms)
        for arm, st in states.items():
            assert st.graphs is not False, f"the {arm} arm fell back to eager rounds during the run"
            if st.guide is not None:
                assert int(st.guide.state[0]) >= 0, f"the {arm} arm left its language"
        tokens = {arm: (st.emitted - emitted0[arm]) / timed[arm] for arm, st in states.items()}

    def stats(v):
        v = sorted(v)
        return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "blocks_ms": [round(x, 4) for x in v],
                "spread": (v[-1] - v[0]) / v[len(v) // 2]}

    res = {a: stats(t[a]) for a in t}
    out = {"what": "ms per greedy tree round replayed from HIP graphs: plain, under a 2-state guide forbidding half of the vocabulary "
                   "(half) and under a guide forbidding all but 1 000 ids (1k), interleaved blocks on one box",
           "model": "llama3-8b dims, random weights", "prefix_tokens": PREFIX, "tree_shape": list(bench.TREE), "rounds_per_block": per,
           "device": torch.cuda.get_device_name(0), "rounds": res, "tokens_per_round": tokens,
           "same_box_spread": max(r["spread"] for r in res.values())}
    for arm in arms[1:]:
        out[f"{arm}_over_plain"] = res[arm]["median_ms"] / res["plain"]["median_ms"]
    return out


def tree_mask():
    import torch
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
    return mask


def kernels():
    """The traced workload: ops.guide_rows on fp16 logits [69, 128256] whose rows follow a 4/16/16/16/16-shaped level-major tree of
    ids that stay inside the language (every row live: every row is streamed), under the three guides one after the other, then
    under the first one without extras (no path to assemble or walk: what a pre-pass for the walk could save at the most);
    ops.guide_advance at n = 17; and ops.argmax_rows on the same logits."""
    import torch
    from longspec_amd import ops
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(1, ROWS, V, generator=g) * 3).to(torch.float16).cuda()
    mask = tree_mask()
    depth = mask[0].ne(0).sum(dim=1)                                       # of row r; node r - 1 lies at depth[r]
    state = torch.zeros((1,), dtype=torch.int32, device="cuda")
    for kind in KERNEL_GUIDES:
        guide = the_guide("half" if kind == "half_no_path" else kind, V)
        table = guide.table(V, "cuda")
        # a node at depth d: an id of parity d - 1 (half), below 1 000 (1k), of class 0 or 1 (c16384): every path is legal
        ids = (2 * torch.randint(0, 400, (1, ROWS - 1), generator=g) + (depth[1:] - 1) % 2)[:, :ROWS - 1]
        if kind == "c16384":
            ids = ids % 2
        kw = {} if kind == "half_no_path" else dict(extra_ids=ids.cuda(), extra_mask=mask.cuda())
        for _ in range(WARM + CALLS):
            ops.guide_rows(x, table, state, **kw)
        torch.cuda.synchronize()
    table = the_guide("half", V).table(V, "cuda")
    acc = (2 * torch.randint(0, 400, (1, ADVANCE_N), generator=g) + torch.arange(ADVANCE_N) % 2).cuda()
    for _ in range(WARM + CALLS):
        state.zero_()
        ops.guide_advance(state, table, acc)
    torch.cuda.synchronize()
    assert int(state[0]) == ADVANCE_N % 2, "the advance workload left the language"
    x = (torch.randn(1, ROWS, V, generator=g) * 3).to(torch.float16).cuda()
    for _ in range(WARM + CALLS):
        ops.argmax_rows(x)
    torch.cuda.synchronize()


def summarise(db, out, tag):
    import re
    import sqlite3
    c = sqlite3.connect(db)
    tables = [r[0] for r in c.execute("select name from sqlite_master where type='table'")]
    disp = [t for t in tables if t.startswith("rocpd_kernel_dispatch")][0]
    sym = [t for t in tables if t.startswith("rocpd_info_kernel_symbol")][0]
    cols = [r[1] for r in c.execute(f"pragma table_info({sym})")]
    name_col = "display_name" if "display_name" in cols else ("kernel_name" if "kernel_name" in cols else "name")
    per = {}                                                              # launches in time order: the guides come one after the other
    for name, start, end in c.execute(f"select s.{name_col}, d.start, d.end from {disp} d join {sym} s on d.kernel_id = s.id order by d.start"):
        per.setdefault(name, []).append((end - start) / 1e3)
    med = lambda v: round(sorted(v)[len(v) // 2], 2)
    res = {"what": f"rocprofv3 --kernel-trace --stats, a run of its own: median microseconds of the last {CALLS} launches at "
                   f"fp16 [{ROWS}, {V}], every row live, rows on a 4/16/16/16/16 tree; half_no_path: the same rows without extras"}
    for name, v in per.items():
        if "guide_rows_kernel" in name:
            assert len(v) == len(KERNEL_GUIDES) * (WARM + CALLS), len(v)
            for i, kind in enumerate(KERNEL_GUIDES):
                res[f"ls_guide_rows_us_{kind}"] = med(v[i * (WARM + CALLS) + WARM:(i + 1) * (WARM + CALLS)])
        elif "guide_advance_kernel" in name:
            res[f"ls_guide_advance_us_n{ADVANCE_N}"] = med(v[-CALLS:])
        elif len(v) >= WARM + CALLS and "topk" in name:                   # the kernels of ops.argmax_rows
            k = re.search(r"(\w+_kernel)(<[^>]*>)?", name)
            res.setdefault("ls_argmax_rows_kernels_us", {})[k.group(0) if k else name[:60]] = med(v[-CALLS:])
    res["ls_argmax_rows_us"] = round(sum(res.get("ls_argmax_rows_kernels_us", {}).values()), 2)
    data = {}
    if os.path.exists(out):
        with open(out) as f:
            data = json.load(f)
    if tag:
        data.setdefault("kernels_by_slice", {})[tag] = {k: v for k, v in res.items() if k.startswith("ls_guide_rows_us")}
    else:
        data["kernels"] = res
    with open(out, "w") as f:
        json.dump(data, f, indent=1)
    print(json.dumps(res))


def build_slices():
    from longspec_amd import build
    for s in SLICES:
        print(build.build_variant(f"slice{s}", [f"-DLS_GUIDE_SLICE={s}"], sources=("guide.hip",)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per", type=int, default=15)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--build-slices", action="store_true")
    ap.add_argument("--summarise", metavar="DB")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guide_ab.json"))
    args = ap.parse_args()
    if args.build_slices:
        build_slices()
        return 0
    if args.kernels:
        kernels()
        return 0
    if args.summarise:
        summarise(args.summarise, args.out, args.tag)
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
