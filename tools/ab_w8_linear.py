"""A/B of the skinny GEMM with 16-bit and with 8-bit (e4m3) weights, per launch, on the Llama-3-8B projection shapes.

    python tools/ab_w8_linear.py [--launches 200] [--rows 1 16 74] [--out profiles/w8_linear_ab.json]

Per-launch time = the ev_start / ev_stop pair of the descriptor (recorded by the C ABI around the kernel).  The two kernels are
launched alternately (A, B, A, B, ...) on the same weights -- the 16-bit operand is the de-quantised 8-bit one --, and the
weights of consecutive launches rotate over enough copies (>= 600 MB per format) that nothing is served from L2 / MALL.
Reported: medians in us, and the bytes of W over the median (TB/s).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from longspec_amd import ops, quant

K = 4096
CASES = [  # name, kind, rows of W
    ("qkv_rope", "qkv", (4096, 1024, 1024)), ("o_proj", "plain", (4096,)), ("gate_up_silu", "mlp", (14336,)),
    ("down_proj", "plain_k", (4096,)), ("lm_head", "plain", (128256,)),
]


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 16, 74])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dtype = torch.float16
    gen = torch.Generator(device="cuda").manual_seed(0)
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 128, 2).float() / 128))
    results = []
    for name, kind, ns in CASES:
        k = 14336 if kind == "plain_k" else K
        rows_w = sum(ns) * (2 if kind == "mlp" else 1)
        bytes8 = rows_w * k
        copies = max(2, -(-600_000_000 // bytes8))
        sets = []
        for _ in range(copies):
            n_w = 2 if kind == "mlp" else len(ns)
            qs = [ops.quantize_rows_e4m3((torch.randn(ns[0] if kind == "mlp" else ns[i], k, generator=gen, device="cuda") * 0.02).to(dtype))
                  for i in range(n_w)]
            w16 = [quant.dequantize_rows_e4m3(q, s, dtype) for q, s in qs]
            if kind == "mlp":
                sets.append((ops.pack_gate_up(*w16), ops.pack_gate_up8(*qs)))
            else:
                rope = kind == "qkv"
                sets.append(([ops.pack_weight(w, rope=rope and i < 2) for i, w in enumerate(w16)],
                             [ops.pack_weight8(p, rope=rope and i < 2) for i, p in enumerate(qs)]))
            del qs, w16
        for M in args.rows:
            x = torch.randn(1, M, k, generator=gen, device="cuda").to(dtype)
            cos, sin = ops.rope_cos_sin(torch.arange(1000, 1000 + M, device="cuda")[None], inv_freq.cuda(), 1.0, dtype)

            def launch(w, ev):
                if kind == "mlp":
                    return ops.mlp_gate_up(x, w, timing=ev)
                if kind == "qkv":
                    return ops.linear_qkv_rope(x, w, None, cos, sin, timing=ev)
                return ops.linear(x, w[0], timing=ev)

            n = args.launches
            evs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)] for _ in range(2)]
            for side in evs:
                for a, b in side:
                    a.record(), b.record()                 # creates the events
            for i in range(2 * len(sets)):                 # warm-up: both kernels, every copy
                launch(sets[i % len(sets)][0], None), launch(sets[i % len(sets)][1], None)
            torch.cuda.synchronize()
            same = True
            for i in range(n):
                w16, w8 = sets[i % len(sets)]
                y16 = launch(w16, evs[0][i])
                y8 = launch(w8, evs[1][i])
                if i < len(sets):
                    same = same and all(torch.equal(a, b) for a, b in zip(y16 if isinstance(y16, list) else [y16], y8 if isinstance(y8, list) else [y8]))
            torch.cuda.synchronize()
            t16 = _median([a.elapsed_time(b) * 1e3 for a, b in evs[0]])
            t8 = _median([a.elapsed_time(b) * 1e3 for a, b in evs[1]])
            r = dict(case=name, M=M, rows_w=rows_w, K=k, copies=copies, launches=n, us_w16=round(t16, 2), us_w8=round(t8, 2),
                     speedup=round(t16 / t8, 3), tbps_w16=round(2 * bytes8 / t16 / 1e6, 3), tbps_w8=round(bytes8 / t8 / 1e6, 3),
                     bit_identical=same)
            results.append(r)
            print(json.dumps(r), flush=True)
        del sets
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), dtype="float16", results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
