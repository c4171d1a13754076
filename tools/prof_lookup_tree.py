"""Kernel time of ``ls_ngram_tree_draft`` (the tree drafter of ``lookup_generate(branches=B)``) next to ``ls_ngram_draft`` in the
same run.

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/prof_lookup_tree.py                (a run of its own)
    python tools/prof_lookup_tree.py --summarise <db> --out profiles/lookup_tree_kernel_stats.json

The workload: batch 1, gamma 7, max_ngram 3, min_ngram 1, a prompt of 16k and of 128k ids with 4k generated columns behind it (a
20k and a 135k text), the host bound a verification pass above the text.  Two kinds of text: random ids below 50 000 (hardly a
candidate per chunk, the common case of a real vocabulary) and random ids below 64 (every chunk holds more than eight
candidates: all eight extraction rounds of the match kernel run).  5 warm-up calls and 50 timed calls of ``ops.ngram_draft``,
then of ``ops.ngram_tree_draft`` with 4 and with 8 branches, per text.  The summary keeps the median of the last 50 launches
of every kernel in every phase."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM, CALLS = 5, 50
PROMPTS, VOCABS, GENERATED, GAMMA, MAX_N, MIN_N = (16384, 131072), (50_000, 64), 4096, 7, 3, 1
BRANCHES = (4, 8)
PHASES = [(P, V) for P in PROMPTS for V in VOCABS]                # in call order


def workload():
    import torch
    from longspec_amd import ops
    g = torch.Generator().manual_seed(1)
    for P, V in PHASES:
        prompt = torch.randint(0, V, (1, P), generator=g).cuda()
        out = torch.randint(0, V, (1, GENERATED + 2 * GAMMA), generator=g).cuda()
        il = torch.tensor([P], dtype=torch.int32, device="cuda")
        cl = torch.tensor([P + GENERATED - 1], dtype=torch.int32, device="cuda")
        wr = torch.tensor([GENERATED], dtype=torch.int32, device="cuda")
        bound = P + GENERATED + 8 * GAMMA + GAMMA + 1
        spec = torch.zeros((1, GAMMA + 1), dtype=torch.int64, device="cuda")
        hist = torch.zeros((1, MAX_N + 1), dtype=torch.int64, device="cuda")
        for _ in range(WARM + CALLS):
            ops.ngram_draft(prompt, il, out, cl, bound, GAMMA, MAX_N, MIN_N, spec, hist=hist)
        for B in BRANCHES:
            F = 1 + B * GAMMA
            all_spec = torch.zeros((1, F), dtype=torch.int64, device="cuda")
            mask = torch.zeros((1, F, F), dtype=torch.int64, device="cuda")
            hist_nb = torch.zeros((1, B + 1), dtype=torch.int64, device="cuda")
            for _ in range(WARM + CALLS):
                ops.ngram_tree_draft(prompt, il, out, wr, bound, GAMMA, B, MAX_N, MIN_N, all_spec, mask, hist=hist, hist_nb=hist_nb)
            torch.cuda.synchronize()
            assert int(hist_nb.sum()) == WARM + CALLS
            assert all_spec[0, 1:].view(GAMMA, B)[:, 0].tolist() == spec[0, 1:].tolist(), "slot 0 is the chain's draft"
            print(f"text {P} + {GENERATED}, ids below {V}, {B} branches: nb histogram {hist_nb[0].tolist()}", flush=True)


def summarise(path, out):
    from rocprof_summary import from_db
    per = {}
    for name, us in from_db(path):                       # (in dispatch order: one process, one stream)
        per.setdefault(name, []).append(us)
    n = WARM + CALLS

    def med(v):
        v = sorted(v[-CALLS:])
        return {"launches": len(v), "median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2)}

    def label(name):
        m = re.search(r"(\w+_kernel)", name)
        return m.group(1) if m else name

    kernels, totals = {}, {}
    for name, v in per.items():
        if "ngram_tree_" in name:                        # per phase: the 4-branch calls, then the 8-branch calls
            assert len(v) == n * len(BRANCHES) * len(PHASES), (name, len(v))
            for i, (P, V) in enumerate(PHASES):
                for j, B in enumerate(BRANCHES):
                    k = (i * len(BRANCHES) + j) * n
                    key = f"text {P} + {GENERATED}, ids below {V}"
                    kernels[f"{label(name)} ({key}, {B} branches)"] = s = med(v[k:k + n])
                    totals.setdefault(key, {}).setdefault(f"ngram_tree_draft_b{B}_us", 0.0)
                    totals[key][f"ngram_tree_draft_b{B}_us"] = round(totals[key][f"ngram_tree_draft_b{B}_us"] + s["median_us"], 2)
        elif "ngram_" in name:
            assert len(v) == n * len(PHASES), (name, len(v))
            for i, (P, V) in enumerate(PHASES):
                key = f"text {P} + {GENERATED}, ids below {V}"
                kernels[f"{label(name)} ({key})"] = s = med(v[i * n:(i + 1) * n])
                totals.setdefault(key, {}).setdefault("ngram_draft_us", 0.0)
                totals[key]["ngram_draft_us"] = round(totals[key]["ngram_draft_us"] + s["median_us"], 2)
    for key, t in totals.items():
        for B in BRANCHES:
            t[f"tree_b{B}_over_chain"] = round(t[f"ngram_tree_draft_b{B}_us"] / t["ngram_draft_us"], 2)
    res = {"what": f"rocprofv3 --kernel-trace --stats, a run of its own: median microseconds of the last {CALLS} launches of the two "
                   f"kernels of ops.ngram_draft and of ops.ngram_tree_draft ({' / '.join(map(str, BRANCHES))} branches) in the same run "
                   f"(batch 1, gamma {GAMMA}, max_ngram {MAX_N}); totals: the sum of an operator's two kernels",
           "kernels": kernels, "totals": totals,
           "text_bytes_read": {str(P): 8 * (P + GENERATED) for P in PROMPTS}}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_tree_kernel_stats.json"))
    a = ap.parse_args()
    if a.summarise:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        summarise(a.summarise, a.out)
    else:
        workload()
