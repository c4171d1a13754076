"""Kernel time of ``ls_penalize_rows`` next to ``ls_argmax_rows`` and ``ls_sample_rows`` (no filter), fp16 logits [rows, 128256].

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/prof_penalize_rows.py --rows 69      (a run of its own, per shape)
    python tools/prof_penalize_rows.py --summarise rows=69:<db> rows=1:<db> --out profiles/penalize_rows_kernel_stats.json

The workload: 68 extras under the mask of a 4/16/16/16/16 tree (row 0 alone for one row), a state with 2048 generated and 4096
prompt tokens, rep = 1.1, pres = 0.5, freq = 0.2; 5 warm-up calls and 50 timed calls of each operator.  The summary keeps the
median of the last 50 launches of every kernel and, for ``ls_penalize_rows``, the fraction of the HBM roofline its bytes
(logits read once and written once) would take at --hbm-tbs."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
V, WARM, CALLS = 128256, 5, 50


def workload(rows):
    import numpy as np
    import torch
    import toy
    from longspec_amd import Penalties, Sampling, ops
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(1, rows, V, generator=g) * 3).to(torch.float16).cuda()
    state = torch.zeros((1, V), dtype=torch.int32)
    state[0, torch.randperm(V, generator=g)[:2048]] = 1
    state[0, torch.randperm(V, generator=g)[:4096]] |= torch.tensor(np.array([0x80000000], dtype=np.uint32).view(np.int32))[0]
    state = state.cuda()
    mask = torch.from_numpy(toy.tree_mask_from_parents(toy.random_beam_tree([4, 16, 16, 16, 16], 7)))[None].to(torch.int64)
    spec = torch.randint(0, V, (1, mask.shape[1]), generator=g)
    ids, mask = spec.cuda()[:, 1:], mask.cuda()[:, :rows, 1:]
    pen, smp = Penalties(1.1, 0.5, 0.2), Sampling(0.6, seed=1)
    pos = torch.arange(rows, dtype=torch.int64, device="cuda").view(1, rows) + 16384
    for fn in (lambda: ops.penalize_rows(x, state, pen, ids, mask), lambda: ops.argmax_rows(x), lambda: ops.sample_rows(x, pos, smp)):
        for _ in range(WARM + CALLS):
            fn()
        torch.cuda.synchronize()


def summarise(specs, out, hbm_tbs):
    from rocprof_summary import from_db
    res = {"what": f"rocprofv3 --kernel-trace --stats, a run of its own per shape: median microseconds of the last {CALLS} launches of "
                   f"every kernel of ops.penalize_rows / ops.argmax_rows / ops.sample_rows (no filter) at [rows, {V}] fp16",
           "hbm_roofline_tb_per_s": hbm_tbs, "shapes": {}}
    for spec in specs:
        label, path = spec.split(":", 1)
        rows = int(label.split("=")[1])
        per = {}
        for name, us in from_db(path):
            per.setdefault(name, []).append(us)
        kernels = {}
        for name, v in per.items():
            if not any(k in name for k in ("penalize_rows", "sample_", "argmax", "topk")):
                continue
            v = sorted(v[-CALLS:])
            m = re.search(r"(\w+_kernel)(<[^>]*>)?", name)          # demangled: "void (anonymous namespace)::x_kernel<ElemF16>(...)"
            kernels[m.group(0) if m else name] = {"launches": len(per[name]), "median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2)}
        pn = next(v for k, v in kernels.items() if "penalize_rows" in k)
        moved = 2 * rows * V * 2
        floor_us = moved / (hbm_tbs * 1e12) * 1e6
        res["shapes"][label] = {"kernels": kernels, "penalize_rows_bytes_moved": moved, "hbm_floor_us": round(floor_us, 2),
                                "penalize_rows_fraction_of_roofline": round(floor_us / pn["median_us"], 3)}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=69)
    ap.add_argument("--summarise", nargs="*")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "penalize_rows_kernel_stats.json"))
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    a = ap.parse_args()
    if a.summarise:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        summarise(a.summarise, a.out, a.hbm_tbs)
    else:
        workload(a.rows)
