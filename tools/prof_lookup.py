"""Kernel time of ``ls_ngram_draft`` (the drafter of ``lookup_generate``) next to ``ls_argmax_rows`` at fp16 [8, 128256].

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/prof_lookup.py                (a run of its own)
    python tools/prof_lookup.py --summarise <db> --out profiles/lookup_kernel_stats.json

The workload: batch 1, gamma 7, max_ngram 3, min_ngram 1, a prompt of 16k and of 128k random ids below 50 000 with 4k generated
columns behind it, the host bound gamma + 2 above the text; 5 warm-up calls and 50 timed calls of ``ops.ngram_draft`` at each
length, then of ``ops.argmax_rows``.  The summary keeps the median of the last 50 launches of every kernel and the bytes the
search reads (8 per token of text)."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
V, ROWS, WARM, CALLS = 128256, 8, 5, 50
PROMPTS, GENERATED, GAMMA, MAX_N, MIN_N = (16384, 131072), 4096, 7, 3, 1


def workload():
    import torch
    from longspec_amd import ops
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(1, ROWS, V, generator=g) * 3).to(torch.float16).cuda()
    for P in PROMPTS:
        prompt = torch.randint(0, 50_000, (1, P), generator=g).cuda()
        out = torch.randint(0, 50_000, (1, GENERATED + GAMMA), generator=g).cuda()
        il = torch.tensor([P], dtype=torch.int32, device="cuda")
        cl = torch.tensor([P + GENERATED - 1], dtype=torch.int32, device="cuda")
        spec = torch.zeros((1, GAMMA + 1), dtype=torch.int64, device="cuda")
        hist = torch.zeros((1, MAX_N + 1), dtype=torch.int64, device="cuda")
        for _ in range(WARM + CALLS):
            info = ops.ngram_draft(prompt, il, out, cl, P + GENERATED + GAMMA + 2, GAMMA, MAX_N, MIN_N, spec, hist=hist)
        torch.cuda.synchronize()
        assert int(hist.sum()) == WARM + CALLS and info[0, 0].item() >= 0
    for _ in range(WARM + CALLS):
        ops.argmax_rows(x)
    torch.cuda.synchronize()


def summarise(path, out):
    from rocprof_summary import from_db
    per = {}
    for name, us in from_db(path):                       # (in dispatch order: one process, one stream)
        per.setdefault(name, []).append(us)
    kernels = {}
    for name, v in per.items():
        if not any(k in name for k in ("ngram_", "topk_chunk", "topk_merge")):
            continue
        m = re.search(r"(\w+_kernel)(<[^>]*>)?", name)
        label = m.group(0) if m else name
        if "ngram_" in name:                             # one workload per text length, in call order
            for i, P in enumerate(PROMPTS):
                part = sorted(v[i * (WARM + CALLS):(i + 1) * (WARM + CALLS)][-CALLS:])
                kernels[f"{label} (text {P} + {GENERATED})"] = {"launches": len(part), "median_us": round(part[len(part) // 2], 2),
                                                                "min_us": round(part[0], 2)}
            continue
        v = sorted(v[-CALLS:])
        kernels[label] = {"launches": len(per[name]), "median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2)}
    res = {"what": f"rocprofv3 --kernel-trace --stats, a run of its own: median microseconds of the last {CALLS} launches of the two "
                   f"kernels of ops.ngram_draft (batch 1, gamma {GAMMA}, max_ngram {MAX_N}) and of ops.argmax_rows at [{ROWS}, {V}] fp16",
           "kernels": kernels,
           "ngram_draft_us": {str(P): round(sum(k["median_us"] for n, k in kernels.items() if "ngram_" in n and f"(text {P} " in n), 2)
                              for P in PROMPTS},
           "text_bytes_read": {str(P): 8 * (P + GENERATED) for P in PROMPTS},
           "argmax_rows_us": round(sum(k["median_us"] for n, k in kernels.items() if "topk_" in n), 2)}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_kernel_stats.json"))
    a = ap.parse_args()
    if a.summarise:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        summarise(a.summarise, a.out)
    else:
        workload()
