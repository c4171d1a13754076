"""Kernel time per call of ``ops.sample_rows`` under ``cut=`` (top_n_sigma, xtc) at [69, 128256] and [1, 128256], fp16, T = 0.6,
next to ``ops.argmax_rows``, the unfiltered draw and top_p alone, from a kernel trace taken in a run of its own (no counters):

    rocprofv3 --kernel-trace --stats -d <dir> -o trace --output-format csv -- python tools/prof_sample_cut.py run
    python tools/prof_sample_cut.py parse <dir> [--out profiles/sample_cut_kernel_times.json]

``run`` issues, per configuration, 5 warm-up calls and 50 measured ones, and a tiny ``ops.rmsnorm`` between configurations: the
parser cuts the trace at those markers, drops the warm-up calls and sums the kernels of a call (launch count = kernels of the
segment / 55).  ``xtc P=0``-like rows: ``xtc_probability = 2^-24`` is below every coin (u >= 2^-24), so the filter is on and no
row fires: the early return of its two grid kernels."""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, T, WARM, CALLS = 128256, 0.6, 5, 50
CONFIGS = [("argmax_rows", None, None),
           ("sample_rows filter off", {}, None),
           ("sample_rows top_p=0.95", dict(top_p=0.95), None),
           ("sample_rows top_n_sigma=1.0", {}, dict(top_n_sigma=1.0)),
           ("sample_rows xtc P=1 theta=0.1", {}, dict(xtc_probability=1.0, xtc_threshold=0.1)),
           ("sample_rows xtc on, no row fires", {}, dict(xtc_probability=2.0 ** -24, xtc_threshold=0.1)),
           ("sample_rows top_k=50 top_p=0.95", dict(top_k=50, top_p=0.95), None),
           ("sample_rows top_k=50 top_p=0.95 top_n_sigma=1.0 xtc P=1 theta=0.1", dict(top_k=50, top_p=0.95),
            dict(top_n_sigma=1.0, xtc_probability=1.0, xtc_threshold=0.1))]
ROWS = (69, 1)
KERNELS = ("sample_hist", "sample_select", "sample_key", "sample_merge", "sample_minp", "sample_count", "sample_band",
           "sample_sigma_part", "sample_sigma_finish", "sample_xtc_sum", "sample_xtc_cut", "sample_xtc_find", "sample_xtc_store",
           "topk_chunk", "topk_merge")


def run():
    import torch
    from longspec_amd import Cut, Sampling, ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(7)
    w = torch.ones(8, dtype=torch.float16, device=dev)
    mark = torch.zeros(2, 8, dtype=torch.float16, device=dev)
    for rows in ROWS:
        x = (torch.randn(rows, V, generator=g) * 3.0).to(torch.float16).to(dev)
        pos = torch.arange(rows, dtype=torch.int64, device=dev) + 1000
        for name, kw, cut in CONFIGS:
            ops.rmsnorm(mark, w, 1e-5)
            c = Cut(**cut) if cut else None
            for _ in range(WARM + CALLS):
                if kw is None:
                    ops.argmax_rows(x)
                else:
                    ops.sample_rows(x, pos, Sampling(T, seed=1, **kw), cut=c)
            torch.cuda.synchronize()
    ops.rmsnorm(mark, w, 1e-5)
    torch.cuda.synchronize()


def parse(directory, out):
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    segments, cur = [], None
    for r in rows:
        if "rmsnorm" in r["Kernel_Name"]:
            cur = []
            segments.append(cur)
        elif cur is not None and "at::native" not in r["Kernel_Name"]:       # (PyTorch's own kernels set the next inputs up)
            cur.append(r)
    segments = segments[:-1]                                          # after the closing marker: nothing
    assert len(segments) == len(ROWS) * len(CONFIGS), len(segments)
    calls = {}
    for i, seg in enumerate(segments):
        n_rows, name = ROWS[i // len(CONFIGS)], CONFIGS[i % len(CONFIGS)][0]
        assert len(seg) % (WARM + CALLS) == 0, (name, len(seg))
        per = len(seg) // (WARM + CALLS)
        groups = [seg[c * per:(c + 1) * per] for c in range(WARM, WARM + CALLS)]
        dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        short = lambda n: next((s for s in KERNELS if s in n), n[:40])
        total = sorted(sum(dur(r) for r in grp) for grp in groups)
        span = sorted((int(grp[-1]["End_Timestamp"]) - int(grp[0]["Start_Timestamp"])) / 1e3 for grp in groups)
        per_kernel, per_count = {}, {}
        for grp in groups:
            for r in grp:
                k = short(r["Kernel_Name"])
                per_kernel[k] = per_kernel.get(k, 0.0) + dur(r) / CALLS
                per_count[k] = per_count.get(k, 0) + 1
        calls[f"rows={n_rows} {name}"] = {"launches": per, "kernel_time_us_median": round(total[len(total) // 2], 2),
                                          "first_start_to_last_end_us_median": round(span[len(span) // 2], 2),
                                          "per_kernel_us_per_call": {k: round(v, 2) for k, v in per_kernel.items()},
                                          "per_kernel_launches_per_call": {k: v // CALLS for k, v in per_count.items()}}
    res = {"what": f"rocprofv3 --kernel-trace --stats, a run of its own: per call of ops.sample_rows / ops.argmax_rows at [rows, {V}] "
                   f"fp16, T = {T}, {CALLS} calls after {WARM} warm-up calls; microseconds", "calls": calls}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["parse"]:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "sample_cut_kernel_times.json")
        parse(sys.argv[2], out)
    else:
        sys.exit(__doc__)
