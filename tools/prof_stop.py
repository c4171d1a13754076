"""Kernel time of ``ls_stop_scan`` and ``ls_stop_ban_rows`` next to ``ls_argmax_rows``, fp16 logits [69, 128256].

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/prof_stop.py                  (a run of its own)
    python tools/prof_stop.py --summarise <db> --out profiles/stop_kernel_stats.json

The workload: 5 warm-up calls and 50 timed calls of ``ops.stop_scan`` (one row, 6 new columns of a 4096-column buffer, 2 ids and
4 sequences of 4 tokens, log-prob buffers with top_n = 5, nothing matches), of ``ops.stop_ban_rows`` with the depth from a tree
mask (every row banned: 2 stores a row; and past ``min_tokens``: the rows exit early) and of ``ops.argmax_rows`` on the same
logits.  The summary keeps the median of the last 50 launches of every kernel."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
V, ROWS, WARM, CALLS = 128256, 69, 5, 50


def workload():
    import torch
    from longspec_amd import Stop, ops
    from longspec_amd.logprobs import new_buffers
    from longspec_amd.stop import new_state
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(1, ROWS, V, generator=g) * 3).to(torch.float16).cuda()
    mask = torch.ones((1, ROWS, ROWS), dtype=torch.int64).tril().cuda()
    out = torch.randint(0, V - 8, (1, 4096), generator=g).cuda()
    seqs = [[V - 3 - q] * 4 for q in range(4)]
    live, past = (Stop([V - 1, V - 2], seqs, min_tokens=m).table(V, "cuda") for m in (10 ** 6, 5))
    state, lp = new_state(1, "cuda"), new_buffers(1, 4096, 5, "cuda")
    written = torch.tensor([2000], dtype=torch.int32, device="cuda")
    num = torch.tensor([6], dtype=torch.int64, device="cuda")
    round_state = torch.zeros((1, 2), dtype=torch.int64, device="cuda")
    calls = (lambda: ops.stop_scan(out, past, state, written, num=num, state=round_state, logprobs=lp),
             lambda: ops.stop_ban_rows(x, live, base=written, depth="tree", tree_mask=mask),
             lambda: ops.stop_ban_rows(x, past, base=written, depth="tree", tree_mask=mask),
             lambda: ops.argmax_rows(x))
    for fn in calls:
        for _ in range(WARM + CALLS):
            fn()
        torch.cuda.synchronize()
    assert state[0, 0].item() == -1


def summarise(path, out):
    from rocprof_summary import from_db
    per = {}
    for name, us in from_db(path):                       # (in dispatch order: one process, one stream)
        per.setdefault(name, []).append(us)
    kernels = {}
    for name, v in per.items():
        if not any(k in name for k in ("stop_scan", "stop_ban_rows", "topk_chunk", "topk_merge")):
            continue
        m = re.search(r"(\w+_kernel)(<[^>]*>)?", name)
        label = m.group(0) if m else name
        if "stop_ban_rows" in name:                      # two workloads, in call order: every row banned, then every row past min_tokens
            for tag, part in (("all rows banned", v[:WARM + CALLS]), ("past min_tokens", v[WARM + CALLS:])):
                part = sorted(part[-CALLS:])
                kernels[f"{label} ({tag})"] = {"launches": len(part), "median_us": round(part[len(part) // 2], 2), "min_us": round(part[0], 2)}
            continue
        v = sorted(v[-CALLS:])
        kernels[label] = {"launches": len(per[name]), "median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2)}
    res = {"what": f"rocprofv3 --kernel-trace --stats, a run of its own: median microseconds of the last {CALLS} launches of the kernels "
                   f"of ops.stop_scan, ops.stop_ban_rows and ops.argmax_rows at [{ROWS}, {V}] fp16",
           "kernels": kernels, "argmax_rows_us": round(sum(k["median_us"] for n, k in kernels.items() if "topk_" in n), 2)}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stop_kernel_stats.json"))
    a = ap.parse_args()
    if a.summarise:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        summarise(a.summarise, a.out)
    else:
        workload()
