"""A/B/C of the skinny GEMM with 16-bit, 8-bit (e4m3) and 4-bit (MXFP4) weights, per launch, on the Llama-3-8B projection shapes.

    python tools/ab_w4_linear.py [--launches 200] [--rows 1 16 74] [--out profiles/w4_linear_ab.json]

Per-launch time = the ev_start / ev_stop pair of the descriptor (recorded by the C ABI around the kernel).  The three kernels
are launched alternately (16, 8, 4, 16, 8, 4, ...), and the weights of consecutive launches rotate over enough copies (>= 600 MB
of the smallest, 4-bit, format) that nothing is served from L2 / MALL.  The 16-bit operand is the de-quantised 4-bit one: every
pair of (16-bit, 4-bit) outputs of the first pass over the copies is compared bit for bit.  The 8-bit operand is the e4m3
rounding of the same weight -- other numbers, so its outputs are compared, on the first copy, with a 16-bit launch on ITS
de-quantised weight.  Reported: medians in us, and the streamed bytes of W over the median (TB/s).
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


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a if isinstance(a, list) else [a], b if isinstance(b, list) else [b]))


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
        bytes4 = rows_w * k * 17 // 32
        bytes8 = rows_w * k
        copies = max(2, -(-600_000_000 // bytes4))
        rope = kind == "qkv"

        def packs16(ws):
            return ops.pack_gate_up(*ws) if kind == "mlp" else [ops.pack_weight(w, rope=rope and i < 2) for i, w in enumerate(ws)]

        sets, twin8 = [], None
        for c in range(copies):
            n_w = 2 if kind == "mlp" else len(ns)
            ws = [(torch.randn(ns[0] if kind == "mlp" else ns[i], k, generator=gen, device="cuda") * 0.02).to(dtype) for i in range(n_w)]
            q4 = [ops.quantize_blocks_mxfp4(w) for w in ws]
            q8 = [ops.quantize_rows_e4m3(w) for w in ws]
            w16 = [quant.dequantize_blocks_mxfp4(q, e, dtype) for q, e in q4]
            if kind == "mlp":
                sets.append((packs16(w16), ops.pack_gate_up8(*q8), ops.pack_gate_up4(*q4)))
            else:
                sets.append((packs16(w16), [ops.pack_weight8(p, rope=rope and i < 2) for i, p in enumerate(q8)],
                             [ops.pack_weight4(p, rope=rope and i < 2) for i, p in enumerate(q4)]))
            if c == 0:
                twin8 = packs16([quant.dequantize_rows_e4m3(q, s, dtype) for q, s in q8])
            del ws, q4, q8, w16
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
            evs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)] for _ in range(3)]
            for side in evs:
                for a, b in side:
                    a.record(), b.record()                 # creates the events
            for i in range(2 * len(sets)):                 # warm-up: all three kernels, every copy
                for f in range(3):
                    launch(sets[i % len(sets)][f], None)
            same8 = _same(launch(sets[0][1], None), launch(twin8, None))
            torch.cuda.synchronize()
            same4 = True
            for i in range(n):
                ys = [launch(sets[i % len(sets)][f], evs[f][i]) for f in range(3)]
                if i < len(sets):
                    same4 = same4 and _same(ys[0], ys[2])
            torch.cuda.synchronize()
            t16, t8, t4 = (_median([a.elapsed_time(b) * 1e3 for a, b in evs[f]]) for f in range(3))
            r = dict(case=name, M=M, rows_w=rows_w, K=k, copies=copies, launches=n, us_w16=round(t16, 2), us_w8=round(t8, 2),
                     us_w4=round(t4, 2), speedup_w4_vs_w16=round(t16 / t4, 3), speedup_w4_vs_w8=round(t8 / t4, 3),
                     tbps_w16=round(2 * bytes8 / t16 / 1e6, 3), tbps_w8=round(bytes8 / t8 / 1e6, 3), tbps_w4=round(bytes4 / t4 / 1e6, 3),
                     w4_bit_identical_to_w16=same4, w8_bit_identical_to_its_w16=same8)
            results.append(r)
            print(json.dumps(r), flush=True)
        del sets, twin8
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), dtype="float16", results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
