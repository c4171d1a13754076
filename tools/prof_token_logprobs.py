"""Kernel time of ``ls_token_logprobs`` next to ``ls_argmax_rows``, fp16 logits [rows, 128256], T = 0.6.

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/prof_token_logprobs.py --rows 69 --n 5    (a run of its own, per shape)
    python tools/prof_token_logprobs.py --summarise rows=69,n=5:<db> rows=1,n=0:<db> ... --out profiles/token_logprobs_kernel_stats.json

The workload: 5 warm-up calls and 50 timed calls of ``ops.token_logprobs`` (random chosen ids) and of ``ops.argmax_rows`` on the
same logits.  The summary keeps the median of the last 50 launches of every kernel, the two stages of ``ls_token_logprobs``
apart, their sum, and the time the logits (read once by stage 1) would take at --hbm-tbs."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
V, WARM, CALLS, T = 128256, 5, 50, 0.6


def workload(rows, n):
    import torch
    from longspec_amd import ops
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(1, rows, V, generator=g) * 3).to(torch.float16).cuda()
    ids = torch.randint(0, V, (1, rows), generator=g).cuda()
    for fn in (lambda: ops.token_logprobs(x, ids, T, n), lambda: ops.argmax_rows(x)):
        for _ in range(WARM + CALLS):
            fn()
        torch.cuda.synchronize()


def summarise(specs, out, hbm_tbs):
    from rocprof_summary import from_db
    res = {"what": f"rocprofv3 --kernel-trace --stats, a run of its own per shape: median microseconds of the last {CALLS} launches of "
                   f"every kernel of ops.token_logprobs (T = {T}) and ops.argmax_rows at [rows, {V}] fp16",
           "hbm_roofline_tb_per_s": hbm_tbs, "shapes": {}}
    for spec in specs:
        label, path = spec.split(":", 1)
        rows = int(re.search(r"rows=(\d+)", label).group(1))
        per = {}
        for name, us in from_db(path):
            per.setdefault(name, []).append(us)
        kernels = {}
        for name, v in per.items():
            if not any(k in name for k in ("logprob_chunk", "logprob_row", "topk_chunk", "topk_merge")):
                continue
            v = sorted(v[-CALLS:])
            m = re.search(r"(\w+_kernel)(<[^>]*>)?", name)          # demangled: "void (anonymous namespace)::x_kernel<ElemF16, true>(...)"
            kernels[m.group(0) if m else name] = {"launches": len(per[name]), "median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2)}
        lp = sum(v["median_us"] for k, v in kernels.items() if "logprob_" in k)
        am = sum(v["median_us"] for k, v in kernels.items() if "topk_" in k)
        res["shapes"][label] = {"kernels": kernels, "token_logprobs_us": round(lp, 2), "argmax_rows_us": round(am, 2),
                                "hbm_floor_us": round(rows * V * 2 / (hbm_tbs * 1e12) * 1e6, 2)}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=69)
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--summarise", nargs="*")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_logprobs_kernel_stats.json"))
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    a = ap.parse_args()
    if a.summarise:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        summarise(a.summarise, a.out, a.hbm_tbs)
    else:
        workload(a.rows, a.n)
