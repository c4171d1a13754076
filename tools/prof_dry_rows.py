"""Time ``ops.dry_rows`` (both launches) next to ``ops.ban_rows`` and ``ops.argmax_rows`` at [69, 128 256] over about 1k and about
20k generated columns: a benign text (random over 32 000 ids: almost nothing matches) and the worst case (one repeated token:
every position matches to depth 32 and competes for one cell per row).  Event timing: the median over blocks of 50 back-to-back
calls, launch overhead included.

    python tools/prof_dry_rows.py [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longspec_amd import Ban, Dry, ops  # noqa: E402

R, V, C, CALLS, BLOCKS = 69, 128256, 68, 50, 7


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = "cuda"
    g = torch.Generator().manual_seed(1)
    logits = torch.randn((1, R, V), generator=g).to(torch.float16).to(dev)
    scratch = torch.zeros((R * V,), dtype=torch.int32, device=dev)
    mask = torch.zeros((R, C), dtype=torch.int64)
    for j in range(4):                                                    # 4 branches of depth 17, level-major
        for d in range(1, 18):
            for dd in range(1, d + 1):
                mask[1 + (d - 1) * 4 + j, (dd - 1) * 4 + j] = 1
    mask = mask.to(dev)
    dry_t = Dry(0.8, 1.75, 2, breakers=(13, 198)).table(V, dev)
    ban_t = Ban(no_repeat_ngram=4).table(V, dev)
    res = {"what": __doc__.split("\n\n")[0], "rows": R, "vocab": V, "calls_per_block": CALLS, "blocks": BLOCKS,
           "device": torch.cuda.get_device_name(0), "cases": {}}
    for w in (1024, 20480):
        base = torch.tensor([w], dtype=torch.int32, device=dev)
        for kind in ("benign", "one_token"):
            if kind == "benign":
                out = torch.randint(0, 32000, (1, w + 8), generator=g).to(dev)
                ids = torch.randint(0, 32000, (1, C), generator=g).to(dev)
            else:
                out = torch.full((1, w + 8), 5, dtype=torch.int64, device=dev)
                ids = torch.full((1, C), 5, dtype=torch.int64, device=dev)
            x = logits.clone()
            case = {"dry_rows": timed(lambda: ops.dry_rows(x, dry_t, out, scratch, base=base, extra_ids=ids, extra_mask=mask))}
            assert int(scratch.count_nonzero()) == 0
            case["ban_rows"] = timed(lambda: ops.ban_rows(x, ban_t, out, base=base, extra_ids=ids, extra_mask=mask))
            case["argmax_rows"] = timed(lambda: ops.argmax_rows(x))
            res["cases"][f"{kind}_{w}"] = case
            print(f"{kind} w={w}: " + ", ".join(f"{k} {v['median_us']} us" for k, v in case.items()), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
