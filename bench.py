#!/usr/bin/env python3
"""bench.py -- accepted tokens/s of the LongSpec draft-then-verify decode round on MI355X.

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A *step* is one decode round of ``LlamaGlide.tree_spec_generate`` (tree_shape 4 16 16 16 16): five
draft passes growing the 69-node beam tree, one 74-row target pass through all 32 layers with the
hybrid tree-verification attention, accept/collapse.  Default workload = the configuration BASELINE.json's
metric is quoted on: Llama-3-8B-Instruct-262k dimensions + longspec draft layer, **131072-token** synthetic
prefix, fp16, temperature 0 -- it fits one GPU (16 GiB of KV).  ``--gpus N`` splits that FIXED prefix N ways
by sequence (strong scaling; 16k rows per GPU at N = 8 = configs[2]); partial attention outputs travel rank to
rank through IPC-mapped mailboxes (csrc/xgmi.hip; --exchange collective = one RCCL all-gather per call instead).  ``--prefix-per-gpu R`` is the secondary
weak-scaling mode (R rows on every GPU; ``--prefix-per-gpu 16384`` at N = 1 is configs[1]).

Synthetic data: random-init weights of the named architecture made "mixed-agreement" (o_proj and
down_proj scaled by --agreement) so that the shared-embedding draft is accepted
some of the time without a trained checkpoint; prefix KV ~ N(0,1) written straight into the caches
(inputs resident in HBM when the timed region starts; prefill is outside the metric, as in the
reference: llama_glide.py:993-994).  tau is printed next to the rate because synthetic tau is not
the published tau.  One JSON line on rank 0.

A plain run sets up, warms up, times the K steps and prints the line (metric, value, unit, higher_is_better, dtype,
ms_per_step, tau, config).  ``--full`` adds what the headline figure does not need: the event-bracketed rounds of the
timed region and the roofline objects built from them, the vanilla-decode denominator and speed-up, the CPU baselines.
``--dump-outputs DIR`` writes what the timed path handed back after its last step (token ids, speculation mask,
counters; float64) as ``DIR/<name>.npy``: inputs are seeded, so two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist

MODELS = {
    # gradientai/Llama-3-8B-Instruct-262k
    "llama3-8b-262k": dict(hidden_size=4096, intermediate_size=14336, num_hidden_layers=32, num_attention_heads=32,
                           num_key_value_heads=8, vocab_size=128256, max_position_embeddings=262144, rms_norm_eps=1e-5,
                           rope_theta=283461213.0, pad_token_id=128001, eos_token_id=128009, bos_token_id=128000),
    # lmsys/vicuna-7b-v1.5-16k
    "vicuna-7b-16k": dict(hidden_size=4096, intermediate_size=11008, num_hidden_layers=32, num_attention_heads=32,
                          num_key_value_heads=32, vocab_size=32000, max_position_embeddings=16384, rms_norm_eps=1e-5,
                          rope_theta=10000.0, rope_scaling={"type": "linear", "factor": 4.0}, pad_token_id=0,
                          eos_token_id=2, bos_token_id=1),
    # lmsys/longchat-13b-16k (configs[3]: MHA, 40 heads)
    "longchat-13b-16k": dict(hidden_size=5120, intermediate_size=13824, num_hidden_layers=40, num_attention_heads=40,
                             num_key_value_heads=40, vocab_size=32000, max_position_embeddings=16384, rms_norm_eps=1e-5,
                             rope_theta=10000.0, rope_scaling={"type": "linear", "factor": 8.0}, pad_token_id=0,
                             eos_token_id=2, bos_token_id=1),
    # Qwen/QwQ-32B-Preview (configs[4]: Qwen2, GQA 40/8, q/k/v bias, bf16)
    "qwq-32b": dict(hidden_size=5120, intermediate_size=27648, num_hidden_layers=64, num_attention_heads=40,
                    num_key_value_heads=8, vocab_size=152064, max_position_embeddings=32768, rms_norm_eps=1e-5,
                    rope_theta=1000000.0, pad_token_id=151643, eos_token_id=151645, bos_token_id=151643,
                    family="qwen2", dtype="bf16"),
}
TREE = [4, 16, 16, 16, 16]

# BASELINE.json "configs", verbatim, and what each means for this script (prefix_per_gpu applies at --gpus 1)
BASELINE_CONFIGS = [
    dict(name="Vicuna-7B-v1.5-16k + longspec draft, tree_shape 4 16 16 16 16, 4k-token synthetic prefix, temperature 0, CPU reference path (plumbing, no GPU)",
         model="vicuna-7b-16k", prefix_total=4096, prefix_per_gpu=4096),
    dict(name="Llama-3-8B-Instruct-262k + longspec draft, 16k synthetic prefix, tree_shape 4 16 16 16 16, 1\u00d7MI355X",
         model="llama3-8b-262k", prefix_total=16384, prefix_per_gpu=16384),
    dict(name="Llama-3-8B-Instruct-262k, 128k synthetic prefix, KV sequence-sharded across 8\u00d7MI355X with RCCL over xGMI",
         model="llama3-8b-262k", prefix_total=131072, prefix_per_gpu=0),
    dict(name="LongChat-13B-16k, GovReport-length (\u22488k) prefixes, chain vs tree method A/B on 1\u00d7MI355X",
         model="longchat-13b-16k", prefix_total=8192, prefix_per_gpu=8192),
    dict(name="QwQ-32B-Preview + longspec draft, 20k-token long-CoT generation, 32k prefix, bf16, 2\u00d7MI355X KV shard",
         model="qwq-32b", prefix_total=32768, prefix_per_gpu=0),
]


def make_config(name):
    d = dict(MODELS[name])
    d.setdefault("rope_scaling", None)
    d.setdefault("family", "llama")
    d.setdefault("dtype", "fp16")
    d["head_dim"] = d["hidden_size"] // d["num_attention_heads"]
    d.update(attention_bias=d["family"] == "qwen2", mlp_bias=False)
    return SimpleNamespace(**d)


def algo_bytes_verify(L, H, Hkv, R=74, D=128):
    """Algorithmic bytes of one verification-attention call: K and V of the prefix, the R
    new K/V rows, q in + o out, the mask bits."""
    return 2 * L * Hkv * D * 2 + 2 * R * Hkv * D * 2 + 2 * R * H * D * 2 + R * R // 8


def committed_traffic(which, algo_bytes, tol=0.03):
    """{"traffic", "traffic_source"} of a roofline object: HBM bytes per launch from the newest committed PMC profile of
    the kernel (profiles/r*_pmc_traffic_<which>_v*.json), only if its launches are this run's launches -- the profile
    records the algorithmic bytes it was taken at, or (older files) its HBM bytes must lie within 0.9-1.25 x of ours."""
    import glob
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    files = sorted(glob.glob(os.path.join(here, "profiles", f"r*_pmc_traffic_{which}_v*.json")),
                   key=lambda f: [int(x) for x in re.findall(r"\d+", os.path.basename(f))])
    for f in reversed(files):
        try:
            with open(f) as fh:
                prof = json.load(fh)
        except (OSError, ValueError):
            continue
        hbm = prof.get("hbm_bytes_per_launch")
        ref = prof.get("algorithmic_bytes_per_launch")
        if not hbm:
            continue
        same = abs(ref - algo_bytes) <= tol * algo_bytes if ref else 0.9 * algo_bytes <= hbm <= 1.25 * algo_bytes
        if same:
            return {"traffic": int(hbm), "traffic_source": f"profiles/{os.path.basename(f)} (separate rocprofv3 --pmc passes of "
                                                             f"this command, per launch; not collected in this run)"}
    return {"traffic": None}


def build_model(cfg, device, agreement, seed):
    from longspec_amd.llama_glide import LlamaGlide
    from longspec_amd.qwen2_glide import Qwen2Glide
    torch.manual_seed(seed)
    with torch.device(device):
        m = (Qwen2Glide if cfg.family == "qwen2" else LlamaGlide)(cfg, dtype=torch.bfloat16 if cfg.dtype == "bf16" else torch.float16)
    g = torch.Generator(device=device).manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("norm.weight"):
                p.fill_(1.0)
            elif name.endswith(".bias"):
                p.zero_()
            elif name.endswith("embed_tokens.weight"):
                p.normal_(0.0, 1.0, generator=g)          # unit-scale residual stream: branch outputs are O(agreement)
            else:
                p.normal_(0.0, 0.02, generator=g)
                if name.endswith("o_proj.weight") or name.endswith("down_proj.weight"):
                    p.mul_(agreement)
    return m


def synth_kv(m, L_local, L_total, max_rows, device, seed):
    """Prefix KV ~ N(0,1) fp16 in every target layer (local shard) and in the draft's own cache."""
    g = torch.Generator(device=device).manual_seed(seed)
    cfg = m.config
    Hkv, D = cfg.num_key_value_heads, 128
    for layer in m.model.layers:
        attn = layer.self_attn
        for nm in ("K_Cache", "V_Cache"):
            t = torch.zeros((1, L_local + max_rows, Hkv, D), dtype=next(m.parameters()).dtype, device=device)
            t[:, :L_local].normal_(0.0, 1.0, generator=g)
            setattr(attn, nm, t)
    sa = m.glide.self_attn
    # the draft only ever reads its last 512 + tree rows; positions are absolute, so the cache is
    # allocated like the reference's (q_len + max_len + 128 rows, llama_glide.py:223-224)
    for nm in ("K_Cache", "V_Cache"):
        t = torch.zeros((1, L_total + max_rows + 128, Hkv, D), dtype=next(m.parameters()).dtype, device=device)
        t[:, max(0, L_total - 1024):L_total].normal_(0.0, 1.0, generator=g)
        setattr(sa, nm, t)


def issued_rows(rows):
    """Query rows the warp-specialised verification kernel multiplies for a `rows`-row block (g * 74 rows of one kv head): the 16-row
    tiles are dealt to 4 S/O wave pairs, so the block is padded to a multiple of 64 (csrc/attn.hip, attn_partial_ws_kernel;
    296 -> 320 for GQA-4, 370 -> 384 as two 192-row chunks for GQA-5); other shapes run the general kernel in 16-row tiles."""
    tiles = (rows + 15) // 16
    if 17 <= tiles <= 24:
        return ((tiles + 3) // 4) * 64
    return tiles * 16


class EventPool:
    """hipEvent pairs recorded by the C ABI around the streaming kernel of every verification-attention
    call of the timed region (on the launch stream)."""

    def __init__(self, n):
        self.ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in self.ev:          # force creation of the underlying hipEvents
            a.record()
            b.record()
        self.i = 0
        self.on = False

    def next(self):
        if not self.on or self.i >= len(self.ev):
            return None
        p = self.ev[self.i]
        self.i += 1
        return p

    def mean_us(self):
        if self.i == 0:
            return None
        return sum(a.elapsed_time(b) for a, b in self.ev[:self.i]) * 1e3 / self.i


class GemmPool:
    """Event pairs + algorithmic bytes of every weight-streaming GEMM launch (ls_linear_fwd) of the timed region."""

    def __init__(self, n):
        self.ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in self.ev:
            a.record()
            b.record()
        self.bytes = []
        self.on = False

    def hook(self, nbytes):
        if not self.on or len(self.bytes) >= len(self.ev):
            return None
        self.bytes.append(nbytes)
        return self.ev[len(self.bytes) - 1]

    def stats(self):
        n = len(self.bytes)
        if n == 0:
            return None
        us = [a.elapsed_time(b) * 1e3 for a, b in self.ev[:n]]
        big = [(b, t) for b, t in zip(self.bytes, us) if b >= 100e6]      # the MLP / lm_head launches
        return {"launches": n, "bytes": float(sum(self.bytes)), "us": float(sum(us)),
                "big_gbps": (sum(b for b, _ in big) / (sum(t for _, t in big) * 1e-6) / 1e9) if big else None}


def cpu_baseline(cfg, L, sample_calls, tau):
    """The oracle's C restatement of the verification attention (kind "port"), timed on the host cores on
    a bounded sample: `sample_calls` layer-calls at the full prefix length; a round needs one per target
    layer (+5 draft cross-attention reads, not timed).  Expressed in the metric's unit as the token rate
    the CPU port would reach if the round consisted of its verification attention alone."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import toy
    from oracle import c_port
    H, Hkv = cfg.num_attention_heads, cfg.num_key_value_heads
    q, k, v, _, _, tm = toy.verify_inputs(H, Hkv, 1, 1235)
    g = torch.Generator().manual_seed(1235)
    kc = torch.randn(1, L + 80, Hkv, 128, generator=g).to(torch.float16)
    vc = torch.randn(1, L + 80, Hkv, 128, generator=g).to(torch.float16)
    c_port.verify_attention(q, k, v, kc, vc, 64, tm, False)             # warm-up (loads the library)
    t0 = time.time()
    done = 0
    while done < sample_calls and (done < 4 or time.time() - t0 < 12.0):     # bounded: ~10 s of host time, >= 4 calls
        c_port.verify_attention(q, k, v, kc, vc, L, tm, False)
        done += 1
    sample_calls = done
    per_call = (time.time() - t0) / sample_calls
    round_s = per_call * cfg.num_hidden_layers
    return {"value": round(tau / round_s, 4), "unit": "accepted tokens/s", "cores": os.cpu_count(), "kind": "port",
            "sample": f"{sample_calls} calls of oracle/oracle_c.c::oracle_verify_attention_f16 (OpenMP, all host cores) at "
                      f"L={L}, H={H}, Hkv={Hkv}, 74 rows: {per_call * 1e3:.1f} ms per layer-call; x{cfg.num_hidden_layers} "
                      f"layers = one round's verification attention only (GEMMs and draft passes not included), at the "
                      f"measured tau"}


def cpu_baseline_round(tree, layers_sample=4, prefix=4096, rounds=2):
    """The FULL decode round on the host cores at BASELINE.json configs[0] scale (Vicuna-7B-v1.5-16k dimensions,
    4k-token synthetic prefix, tree_shape 4 16 16 16 16, fp16 storage): this repository's host logic driven by the
    oracle's CPU operators (tests/oracle_ops.py; verification attention through the OpenMP C restatement).  Bounded
    sample: `layers_sample` of the 32 target layers are instantiated and timed (they are identical in shape), the
    draft layer / lm_head / tree bookkeeping run in full; the round time is extrapolated as
    non_layer_time + 32 / layers_sample * layer_time."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_ops
    from oracle import c_port, ref_ops
    from longspec_amd.llama_glide import LlamaGlide

    class CpuOps:
        def __getattr__(self, name):
            return getattr(oracle_ops, name)

        @staticmethod
        def verify_attention(q, k_new, v_new, k_cache, v_cache, cache_lens, mask_bits, last_layer, softmax_scale=1 / (128 ** 0.5),
                             kv_len_hint=None, n_splits=0):
            return c_port.verify_attention(q.contiguous(), k_new.contiguous(), v_new.contiguous(), k_cache, v_cache,
                                           int(cache_lens[0]), mask_bits, last_layer, softmax_scale)

    cfg = make_config("vicuna-7b-16k")
    full_layers = cfg.num_hidden_layers
    cfg.num_hidden_layers = layers_sample
    torch.manual_seed(7)
    m = LlamaGlide(cfg, ops=CpuOps(), dtype=torch.float16)
    with torch.no_grad():
        for name, prm in m.named_parameters():
            if name.endswith("norm.weight"):
                prm.fill_(1.0)
            elif name.endswith(".bias"):
                prm.zero_()
            else:
                prm.copy_(torch.randn(prm.shape, dtype=torch.float32).mul_(0.02 if "embed" not in name else 1.0))
    max_gen = 6 * (rounds + 3) + 16
    max_rows = max_gen + 256
    m.set_max_gen_len(max_rows)
    m.glide.set_max_gen_len(max_rows)
    synth_kv(m, prefix, prefix, max_rows, "cpu", seed=99)
    lens = torch.tensor([prefix], dtype=torch.int32)
    first = torch.tensor([1000], dtype=torch.int64)
    layer_s = [0.0]
    for layer in m.model.layers:
        fwd = layer.forward

        def timed(*a, _f=fwd, **k):
            t = time.time()
            r = _f(*a, **k)
            layer_s[0] += time.time() - t
            return r
        layer.forward = timed
    with torch.inference_mode():
        st = m.begin_tree_decode(first, lens, prefix, tree, max_gen, eos_id=-1)
        st.eos = None
        st.use_graphs = False
        m.tree_round(st)                                   # warm-up (thread pools, allocator)
        layer_s[0] = 0.0
        tok0 = st.emitted
        t0 = time.time()
        for _ in range(rounds):
            m.tree_round(st)
        total = (time.time() - t0) / rounds
        tokens = (st.emitted - tok0) / rounds
    lay = layer_s[0] / rounds
    full = (total - lay) + lay * full_layers / layers_sample          # EXTRAPOLATED: labelled so in the JSON ("kind_detail")
    return {"value": round(tokens / full, 4), "unit": "accepted tokens/s", "cores": os.cpu_count(), "kind": "port",
            "extrapolated": True, "measured_ms_per_round_at_sampled_layers": round(total * 1e3, 1),
            "extrapolated_ms_per_round": round(full * 1e3, 1),
            "sample": f"EXTRAPOLATED from {layers_sample} of {full_layers} layers: {rounds} full decode rounds (5 draft passes + 74-row verify pass + tree bookkeeping) of vicuna-7b-16k dims, "
                      f"{prefix}-token synthetic prefix, host logic of this repository on the oracle's CPU operators (torch-CPU fp16 "
                      f"linears, oracle/ref_ops.py, oracle/oracle_c.c OpenMP verification attention); {layers_sample} of "
                      f"{full_layers} target layers instantiated: measured {total * 1e3:.0f} ms/round of which {lay * 1e3:.0f} ms in "
                      f"the {layers_sample} layers -> {full * 1e3:.0f} ms/round extrapolated to {full_layers} layers; tau {tokens:.2f} "
                      f"of this random-weight model"}


def dump_outputs(d, st, emitted_before_last):
    """What a caller of the timed path receives (``tree_spec_generate`` / ``spec_generate`` return output_ids, count, num,
    spec_mask), taken from the decode state after the last timed step, plus the tokens that step emitted.  Token ids are
    exact in float64."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    arrays = {
        "output_ids": st.output_ids,
        "spec_mask": st.spec_mask,
        "last_step_tokens": st.output_ids[:, emitted_before_last:st.emitted],
        "counters": torch.tensor([st.emitted, st.count, st.num]),          # emitted tokens, accepted draft tokens, rounds
    }
    for name, t in arrays.items():
        np.save(os.path.join(d, name + ".npy"), t.detach().cpu().to(torch.float64).numpy())


SAMPLE = 10      # every SAMPLE-th timed round is issued launch by launch with HIP events around the attention kernel (32 pairs)
GSAMPLE = 20     # ... and every GSAMPLE-th also around the ~165 projection launches: an event record costs ~5 us of stream time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="llama3-8b-262k", choices=sorted(MODELS))
    ap.add_argument("--prefix-total", type=int, default=131072,
                    help="prefix tokens of the whole job, split by sequence over --gpus (strong scaling; the metric's config)")
    ap.add_argument("--prefix-per-gpu", type=int, default=0,
                    help="secondary mode: this many prefix rows on EVERY GPU (weak scaling; 16384 at N = 1 is configs[1])")
    ap.add_argument("--agreement", type=float, default=None,
                    help="scale of the o_proj / down_proj weights of the random model (smaller = the draft agrees more often).  Default "
                         "0.02, and 0.01 for qwq-32b: a 64-layer residual stream drifts twice as far from the shared embedding, and "
                         "0.02 leaves tau = 1.3 there against ~3 for the 32/40-layer models (round 4: tau 3.0 at 0.01)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: event-bracketed rounds inside the timed region "
                         "(roofline objects, per-rank kernel times), the vanilla-decode denominator and speed-up, the CPU baselines. "
                         "The --no-* options below switch parts of it off")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed (output_ids, spec_mask, the last step's "
                         "tokens, counters) as DIR/<name>.npy in float64")
    ap.add_argument("--vanilla-steps", type=int, default=16)
    ap.add_argument("--cpu-sample-calls", type=int, default=64)     # bounded by time below: ~12 s of host time
    ap.add_argument("--no-cpu-round", action="store_true", help="--full: skip the full-round CPU baseline at configs[0] scale")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip both CPU baselines")
    ap.add_argument("--no-vanilla", action="store_true", help="--full: skip the vanilla-decode denominator (profiling runs)")
    ap.add_argument("--no-graphs", action="store_true", help="issue every round launch by launch (no HIP-graph replay)")
    ap.add_argument("--no-kernel-timing", action="store_true",
                    help="--full, diagnostic: no event-bracketed rounds (no roofline objects): every round is a graph replay")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="diagnostic: gloo lets several ranks share ONE GPU (with --share-gpu) to exercise the N > 1 code path")
    ap.add_argument("--exchange", default="peer", choices=["peer", "collective"],
                    help="N > 1: how the per-rank attention records travel -- peer stores into IPC mailboxes (graph-capturable, "
                         "default) or one torch.distributed all-gather per attention call")
    ap.add_argument("--no-exchange-check", action="store_true", help="skip the 4-round peer-vs-collective cross-check before the clock starts")
    ap.add_argument("--share-gpu", action="store_true",
                    help="diagnostic: every rank uses cuda:0.  (Full-size kernels of two processes cannot co-reside on one GPU: a rank "
                         "spinning for its peer's record keeps the peer's attention kernel off the CUs until the wait times out -- "
                         "the cross-check then moves the run to the collective.)")
    ap.add_argument("--no-vocab-parallel", action="store_true",
                    help="N > 1 (or --shard-path): keep the lm_head replicated instead of sharding it by vocabulary over the ranks")
    ap.add_argument("--shard-path", action="store_true",
                    help="diagnostic: take the sequence-sharded attention path (partial -> reduce -> all-gather -> finish) even "
                         "with one rank, to price its extra launches without a second GPU")
    ap.add_argument("--config", type=int, default=None, choices=range(len(BASELINE_CONFIGS)),
                    help="one of BASELINE.json's configs by index: sets the model / prefix / dtype and names the config verbatim in "
                         "config.workload (configs[2] is the default workload; 0 runs the Vicuna-7B 4k case on the GPU)")
    ap.add_argument("--method", default="tree", choices=["tree", "seq"],
                    help="tree = tree_spec_generate rounds (the metric); seq = the chain method (spec_generate, gamma 4) on the same model "
                         "and prefix -- configs[3]'s chain-vs-tree A/B (inference_long-bench.py --method seq | tree).  The line of a seq "
                         "run carries no roofline objects (its target pass is a 5-row decode pass, not the 74-row verification)")
    args = ap.parse_args()
    if args.config is not None:
        preset = BASELINE_CONFIGS[args.config]
        args.model = preset["model"]
        if preset.get("prefix_per_gpu") and args.gpus == 1:
            args.prefix_per_gpu = preset["prefix_per_gpu"]
        else:
            args.prefix_total, args.prefix_per_gpu = preset["prefix_total"], 0

    if args.agreement is None:
        args.agreement = 0.01 if args.model == "qwq-32b" else 0.02

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # started as `python bench.py --gpus N`: become the launcher -- one rank per GPU under torch.distributed.run, rendezvous on
        # 127.0.0.1 at a free port.  Rank 0's JSON line stays the last line of stdout (the children inherit it).
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.stdout.flush()
        sys.exit(subprocess.call(cmd, env=env))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    if os.environ.get("LS_BENCH_DRY_RUN"):
        # launcher test (tests/test_bench_launcher.py, no GPU): the ranks rendezvous over gloo, rank 0 prints the line's skeleton
        dist.init_process_group("gloo")
        seen = dist.get_world_size()
        dist.barrier()
        dist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"dry_run": True, "n_gpus": world, "ranks_seen": seen, "steps": args.steps, "warmup": args.warmup}), flush=True)
        return
    if args.share_gpu:
        local_rank = 0
        if world > 1 and args.backend != "gloo":     # RCCL refuses two ranks on one device ("Duplicate GPU detected")
            if rank == 0:
                print("[bench] --share-gpu: ranks share cuda:0, the collective backend is gloo", file=sys.stderr, flush=True)
            args.backend = "gloo"
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC (RCCL, hipIpc mailboxes): before the runtime starts
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1 or args.shard_path:
        if world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29511")
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=device)
        elif args.backend == "gloo":
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)

    cfg = make_config(args.model)
    H, Hkv = cfg.num_attention_heads, cfg.num_key_value_heads
    weak = args.prefix_per_gpu > 0
    if weak:
        Ls = args.prefix_per_gpu
    else:
        assert args.prefix_total % world == 0, "--prefix-total must divide by --gpus"
        Ls = args.prefix_total // world
    L_total = Ls * world
    rounds = args.steps + args.warmup
    max_gen = 6 * (rounds + 2) + 16
    max_rows = max_gen + 256
    exchange_forced = None
    m = build_model(cfg, device, args.agreement, seed=1234)          # replicated weights: same seed on every rank
    m.set_max_gen_len(max_rows)
    m.glide.set_max_gen_len(max_rows)
    synth_kv(m, Ls, L_total, max_rows, device, seed=4321 + rank)
    if world > 1 or args.shard_path:
        from longspec_amd.dist import KVShard
        shard = KVShard(rank, world, shard_rows=Ls, vocab_parallel=not args.no_vocab_parallel)
        for layer in m.model.layers:
            layer.self_attn.shard = shard
        m.glide.cross_attn.shard = shard
        if args.exchange == "peer" and args.share_gpu and world > 1:
            exchange_forced = "ranks share one GPU: a rank polling for its peer's record keeps the peer's full-size kernels off the CUs"
            args.exchange = "collective"
        if args.exchange == "peer":
            # records go rank to rank through IPC-mapped mailboxes (csrc/xgmi.hip): the round stays a HIP graph.  Falls
            # back to the library collective (and says so) when the mapping or its self-check fails.
            shard.enable_peer_exchange(128 * max(H, m.glide.config.num_attention_heads) * 129, device)

    lens = torch.tensor([L_total], dtype=torch.int32, device=device)
    first = torch.tensor([1000], dtype=torch.int64, device=device)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # every rank brackets the same rounds (round 4: the line carries per-rank figures); a plain run replays every round
    timing = args.full and not args.no_kernel_timing
    from longspec_amd import ops as _ops

    def fresh_state():
        s_ = m.begin_tree_decode(first, lens, L_total, TREE, max_gen, eos_id=-1)
        s_.eos = None                                    # run a fixed number of rounds
        return s_

    if args.method == "seq":
        # ---- the chain method (llama_glide.py:621-774), one GPU: K rounds of gamma = 4 draft steps + one 5-row target pass
        assert world == 1 and not args.shard_path, "--method seq is a one-GPU A/B leg"
        gamma = 4
        with torch.inference_mode():
            cst = m.begin_chain_decode(first, lens.clone(), lens.to(torch.int64), L_total, gamma=gamma,
                                       max_gen_len=(gamma + 1) * (rounds + 2) + 8, eos_id=-1)
            cst.eos = None                                   # a fixed number of rounds
            for _ in range(args.warmup):
                m.chain_round(cst)
            barrier()
            tok0 = e_last = cst.emitted
            t0 = time.time()
            for _ in range(args.steps):
                e_last = cst.emitted
                m.chain_round(cst)
            barrier()
            elapsed = time.time() - t0
            tokens = cst.emitted - tok0
            if args.dump_outputs:
                dump_outputs(args.dump_outputs, cst, e_last)
        out = {"metric": "accepted tokens/sec (chain speculative decode, gamma 4, temperature 0)", "value": round(tokens / elapsed, 3),
               "unit": "accepted tokens/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak" if weak else "strong",
               "vs_baseline": None, "dtype": cfg.dtype, "data": "synthetic",
               "config": {"workload": (BASELINE_CONFIGS[args.config]["name"] + " -- " if args.config is not None else "") +
                                      f"{args.model} dims + longspec draft layer, {L_total}-token synthetic prefix, --method seq (chain, gamma {gamma}), "
                                      "temperature 0, batch 1", "prefix_tokens": L_total, "kv_rows_per_gpu": Ls, "parallelism": "1 GPU",
                          "method": "seq"},
               "tau": round(tokens / args.steps, 3), "rounds_per_s": round(args.steps / elapsed, 3), "hip_graphs": False}
        print(json.dumps(out), flush=True)
        return

    exchange_note = exchange_forced
    if world > 1 and shard.peer is not None and not args.no_exchange_check:
        # The peer-store exchange on THIS machine against the library collective, on the real workload: the same four
        # rounds from the same state, once with each, must emit the same tokens on every rank (and no wait may time out).
        # Otherwise the run continues on the collective -- a wrong exchange is a wrong benchmark.
        with torch.inference_mode():
            peer_obj, shard.peer = shard.peer, None
            s_ = fresh_state()
            for _ in range(4):
                m.tree_round(s_)
            ref = s_.output_ids[0, :s_.emitted].clone()
            shard.peer = peer_obj
            s_ = fresh_state()
            s_.use_graphs = s_.use_graphs and not args.no_graphs
            for _ in range(4):
                m.tree_round(s_)
            got = s_.output_ids[0, :s_.emitted].clone()
            ok = got.numel() == ref.numel() and bool(torch.equal(got, ref)) and not shard.peer.status()[1]
            flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=device)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if not int(flag.item()):
                shard.peer.close()
                shard.peer = None
                exchange_note = "peer-store exchange disagreed with the collective on the 4-round cross-check: run continued on the collective"
                if rank == 0:
                    print("[bench] " + exchange_note, file=sys.stderr, flush=True)
            del s_

    def measure():
        """warm-up + the timed K rounds from a fresh decode state; rank 0 brackets every launch of every 10th round with events"""
        pool = EventPool(cfg.num_hidden_layers * args.steps) if timing else None
        gpool = GemmPool((4 * cfg.num_hidden_layers + 48) * (args.steps // SAMPLE + 1)) if timing else None
        xpool = EventPool(cfg.num_hidden_layers * (args.steps // SAMPLE + 1)) if timing and (world > 1 or args.shard_path) else None
        if pool is not None:
            for layer in m.model.layers:
                layer.self_attn.timing = pool.next
                layer.self_attn.xchg_timing = xpool.next if xpool is not None else None
            _ops.set_linear_timing(gpool.hook)
        with torch.inference_mode():
            st = fresh_state()
            graphs = st.use_graphs and not args.no_graphs
            st.use_graphs = graphs
            if graphs:
                m.prepare_tree_graphs(st)                # one HIP graph per accepted-token count, captured before the clock starts
            barrier()                                    # no rank polls for a peer that is still capturing
            for _ in range(args.warmup):
                m.tree_round(st)
            barrier()
            tok0 = e_last = st.emitted
            if pool is not None:
                pool.on = gpool.on = True
            t0 = time.time()
            for i in range(args.steps):
                e_last = st.emitted
                if gpool is not None:                    # launches are bracketed on every 10th / 20th round only: two event
                    pool.on = (i % SAMPLE == 0)          # records around each of ~200 launches cost ~2 ms per round, and
                    if xpool is not None:
                        xpool.on = pool.on
                    gpool.on = (i % GSAMPLE == 0)        # those rounds are inside the timed region
                    st.use_graphs = graphs and not pool.on   # the bracketed rounds are issued launch by launch, the others replayed
                m.tree_round(st)
            barrier()
            elapsed = time.time() - t0
            if pool is not None:
                pool.on = gpool.on = False
                if xpool is not None:
                    xpool.on = False
                _ops.set_linear_timing(None)
            tokens = st.emitted - tok0
        agree, detail = True, None
        if world > 1:                                    # the round is replicated: every rank must have emitted the same tokens
            chk = torch.tensor([tokens, int(st.output_ids[0, :st.emitted].sum())], dtype=torch.int64, device=device)
            lo = chk.clone()
            dist.all_reduce(lo, op=dist.ReduceOp.MIN)
            dist.all_reduce(chk, op=dist.ReduceOp.MAX)
            agree = bool(torch.equal(lo, chk))
            if not agree:
                detail = {"tokens_min_max": [int(lo[0]), int(chk[0])], "id_sum_min_max": [int(lo[1]), int(chk[1])]}
        return SimpleNamespace(elapsed=elapsed, tokens=tokens, st=st, graphs=graphs, pool=pool, gpool=gpool, xpool=xpool, agree=agree,
                               detail=detail, e_last=e_last)

    res = measure()
    if world > 1 and shard.peer is not None:
        # a wait that timed out (on any rank) or ranks that emitted different tokens void the run: measure again on the collective
        bad = torch.tensor([int(shard.peer.status()[1] or not res.agree)], dtype=torch.int32, device=device)
        dist.all_reduce(bad, op=dist.ReduceOp.MAX)
        if int(bad.item()):
            exchange_note = ("peer-store exchange failed during the timed rounds (timeout or rank disagreement): "
                             "measured again on the collective")
            if rank == 0:
                print("[bench] " + exchange_note, file=sys.stderr, flush=True)
            shard.peer.close()
            shard.peer = None
            res = measure()
    elapsed, tokens, st, graphs, pool, gpool, xpool = res.elapsed, res.tokens, res.st, res.graphs, res.pool, res.gpool, res.xpool
    t = torch.tensor([elapsed], dtype=torch.float64, device=device)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    tau = tokens / args.steps
    value = tokens / elapsed
    if args.dump_outputs and rank == 0:                  # the round is replicated: rank 0's outputs are every rank's
        dump_outputs(args.dump_outputs, st, res.e_last)

    out = {
        "metric": "accepted tokens/sec (tree speculative decode, temperature 0)", "value": round(value, 3),
        "unit": "accepted tokens/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak" if weak else "strong",
        "vs_baseline": None, "dtype": cfg.dtype, "data": "synthetic",
        "config": {"workload": (BASELINE_CONFIGS[args.config]["name"] + " -- " if args.config is not None else "") +
                               f"{args.model} dims + longspec draft layer, {L_total}-token synthetic prefix "
                               f"({Ls} rows of KV per GPU), tree_shape 4 16 16 16 16, temperature 0, batch 1"
                               + ("" if weak or args.model != "llama3-8b-262k" or L_total != 131072 else
                                  " [BASELINE.json metric config: Llama-3-8B @128k ctx]"),
                   "prefix_tokens": L_total, "kv_rows_per_gpu": Ls, "method": "tree",
                   "parallelism": "1 GPU" if world == 1 else
                   f"prefix KV sequence-sharded x{world}, lm_head " + ("replicated" if args.no_vocab_parallel else f"vocabulary-sharded x{world}")
                   + ", layer weights replicated"},
        "tau": round(tau, 3), "rounds_per_s": round(args.steps / elapsed, 3), "agreement": args.agreement,
        "hip_graphs": bool(graphs and st.graphs is not False),
        # boxes of the pool differ by ~2 % on the same binary (three same-box repeats agree to 0.3 %: profiles/r4_bench_repeat.json);
        # differences below this between two single runs are not a result
        "box_to_box_spread": 0.02,
    }
    if world > 1 or args.shard_path:
        out["backend"] = dist.get_backend()
        if out["backend"] == "nccl":
            out["rccl_ranks"] = dist.get_world_size()        # what RCCL itself saw
        out["exchange"] = ("peer stores into IPC-mapped mailboxes, fused into the two combine kernels of the call (csrc/xgmi.hip)" if shard.peer is not None
                           else "torch.distributed all-gather per attention call")
        if exchange_note:
            out["exchange_note"] = exchange_note
        if shard.peer is not None:
            done, timed_out = shard.peer.status()
            out["exchange_calls"], out["exchange_timed_out"] = done, timed_out
        if world > 1:
            out["ranks_agree"] = res.agree
            if res.detail:
                out["ranks_disagree"] = res.detail
    if timing:
        # ---- roofline of the kernel north_star names: the hybrid verification attention, stage 1 (this rank's KV shard).
        # achieved = SURVEY 8(d)'s algorithmic bytes of one call / the kernel's average duration, every launch of the timed
        # region's bracketed rounds measured with HIP events recorded by the C ABI on the launch stream.  `traffic` (PMC
        # HBM bytes per launch) cannot be observed inside this process: it is the figure of the separate rocprofv3 --pmc
        # passes of THIS command (tools/round_profile.sh; FETCH_SIZE / WRITE_SIZE, corrected as MI355X_MICROARCH.md
        # prescribes) committed under profiles/ -- quoted only when this run's launch moves the same algorithmic bytes
        # as the profiled one, null otherwise; `traffic_source` names the file.
        from longspec_amd import ops as _ops2
        mean_us = pool.mean_us()
        ab = algo_bytes_verify(Ls, H, Hkv)
        achieved = ab / (mean_us * 1e-6) / 1e9
        out["roofline"] = {"bound": "hbm", "achieved": round(achieved, 2), "peak": 8000.0, "unit": "GB/s",
                           "frac": round(achieved / 8000.0, 4), **committed_traffic("attn", ab),
                           "kernel": f"{_ops2.attn_kernel_name(H // Hkv * 74)} (hybrid tree-verification attention, stage 1: "
                                     f"prefix flash-decoding + tree part)",
                           "algorithmic_bytes_per_launch": ab, "avg_launch_us": round(mean_us, 2), "launches_timed": pool.i,
                           "mfma_tflops": round(4 * 74 * H * 128 * Ls / (mean_us * 1e-6) / 1e12, 1),
                           "mfma_frac_of_2500": round(4 * 74 * H * 128 * Ls / (mean_us * 1e-6) / 1e12 / 2500.0, 4),
                           # what the matrix pipe actually executes: the row block padded to whole 16-row tiles per S/O pair
                           # (Llama-3: 296 -> 320 rows) and the ones-tile that forms the soft-max row sums (a ninth V tile:
                           # 17 k-tiles of MFMAs per 32 keys instead of 16) -- VERDICT r3 weak 2
                           "mfma_frac_of_2500_incl_padding": round(
                               4 * issued_rows(74 * (H // Hkv)) * Hkv * 128 * Ls * (17.0 / 16.0) / (mean_us * 1e-6) / 1e12 / 2500.0, 4)}
        # Which roofline binds this call: algorithmic flops / algorithmic bytes against the chip's ridge (2.5 PFLOP/s dense 16-bit
        # MFMA / 8 TB/s = 312.5 flop/B).  Llama-3 (4 x 74 rows per kv head): 296 -> HBM, the object above; QwQ (5 x 74): 370 -> the
        # matrix pipe, reported beside it in the same form ("MFMA is the secondary bound ... at g*74 >= ~300 rows").
        flops = 4.0 * 74 * H * 128 * Ls
        out["roofline"]["flop_per_byte"] = round(flops / ab, 1)
        out["roofline"]["binding"] = "mfma" if flops / ab > 2500.0e12 / 8000.0e9 else "hbm"
        if out["roofline"]["binding"] == "mfma":
            tf = flops / (mean_us * 1e-6) / 1e12
            out["roofline_mfma"] = {"bound": "mfma", "achieved": round(tf, 1), "peak": 2500.0, "unit": "TFLOP/s",
                                    "frac": round(tf / 2500.0, 4), "traffic": None, "kernel": out["roofline"]["kernel"]}
        # ---- second kernel: the weight-streaming GEMM (ls_linear_fwd), the larger share of the round at short prefixes.
        # Algorithmic bytes of a launch = packed weight + x + y.
        gs = gpool.stats()
        g_ach = gs["bytes"] / (gs["us"] * 1e-6) / 1e9
        out["roofline_gemm"] = {"bound": "hbm", "achieved": round(g_ach, 2), "peak": 8000.0, "unit": "GB/s",
                                "frac": round(g_ach / 8000.0, 4), **committed_traffic("gemm", gs["bytes"] / gs["launches"]),
                                "kernel": "skinny_gemm_kernel (ls_linear_fwd: q|k|v, o_proj, gate|up+SiLU, down_proj, lm_head of the "
                                          "verify pass and the 5 draft passes)",
                                "algorithmic_bytes_per_launch": round(gs["bytes"] / gs["launches"]),
                                "avg_launch_us": round(gs["us"] / gs["launches"], 2), "launches_timed": gs["launches"],
                                "gemm_ms_per_round": round(gs["us"] / len(range(0, args.steps, GSAMPLE)) / 1e3, 3),
                                "launches_over_100MB_gbps": round(gs["big_gbps"], 1) if gs["big_gbps"] else None}
        out["attention_ms_per_round"] = round(mean_us * cfg.num_hidden_layers / 1e3, 3)
        mine = {"rank": rank, "attention_ms_per_round": out["attention_ms_per_round"],
                "gemm_ms_per_round": out["roofline_gemm"]["gemm_ms_per_round"],
                "exchange_us_per_call": round(xpool.mean_us(), 2) if xpool is not None and xpool.i else None,
                "ms_per_step": round(res.elapsed / args.steps * 1e3, 4)}
        if world > 1:
            # one line must diagnose a scaling run: stage-1 attention, exchange + merge (reduce/push + wait/merge kernels of a
            # call, or the collective) and GEMM time of EVERY rank
            allr = [None] * world
            dist.all_gather_object(allr, mine)
            out["per_rank"] = allr
        else:
            out["per_rank"] = [mine]
        out["exchange_us_per_call"] = mine["exchange_us_per_call"]
    if timing:
        # ---- the whole round against the HBM roofline: every weight streamed by the six passes (+ their
        # small x / y) as counted on the bracketed rounds, the prefix K/V of the 32 verification calls and of the 5 draft
        # cross-attention calls, the draft's 512-row window.  This rank's bytes over this rank's round time.
        n_sampled = len(range(0, args.steps, GSAMPLE))
        gemm_b = gs["bytes"] / n_sampled
        kv_row = 2 * Hkv * 128 * 2
        attn_b = cfg.num_hidden_layers * ab + 5 * (Ls * kv_row) + 5 * (512 * kv_row)
        round_b = gemm_b + attn_b
        r_ach = round_b / (elapsed / args.steps) / 1e9
        out["roofline_round"] = {"bound": "hbm", "achieved": round(r_ach, 2), "peak": 8000.0, "unit": "GB/s",
                                 "frac": round(r_ach / 8000.0, 4), "algorithmic_bytes_per_round": round(round_b),
                                 "of_which_weights": round(gemm_b), "of_which_kv": round(attn_b)}
    if args.full and rank == 0 and world == 1 and not args.no_vanilla:
        # ---- speed-up denominator: vanilla autoregressive decode on the same model and prefix ----------
        with torch.inference_mode():
            for layer in m.model.layers:
                layer.self_attn.timing = None
            out_v = torch.zeros((1, args.vanilla_steps + 8), dtype=torch.int64, device=device)
            out_v[:, 0] = first
            vs = m.begin_vanilla_decode(out_v, lens.clone(), lens.clone(), L_total)
            vs.use_graphs = vs.use_graphs and not args.no_graphs          # same treatment as the tree rounds
            graph_after, m.GRAPH_AFTER = m.GRAPH_AFTER, 2                 # capture now, not after GRAPH_AFTER tokens
            graph_tier, m.GRAPH_TIER = m.GRAPH_TIER, None                 # one capture sized for all --vanilla-steps: no tier edge
            try:                                                          # (and its re-capture) inside the timed steps
                for i in range(args.vanilla_steps + 4):                   # steps 1-2 eager, 3 captures, the rest replay
                    if i == 4:
                        torch.cuda.synchronize()
                        tv = time.time()
                    m.vanilla_step(vs)
                torch.cuda.synchronize()
                vanilla_tps = args.vanilla_steps / (time.time() - tv)
            finally:
                m.GRAPH_AFTER = graph_after
                m.GRAPH_TIER = graph_tier
            if vs.use_graphs and vs.graph_captures != 1:                  # the timed steps should be replays of ONE capture:
                out["vanilla_graph_captures"] = vs.graph_captures         # said in the line, not fatal behind a finished measurement
                print(f"[bench] warning: vanilla denominator ran with {vs.graph_captures} graph captures inside its timed steps "
                      f"(tokens/s understated)", file=sys.stderr, flush=True)
        out["vanilla_tokens_per_s"] = round(vanilla_tps, 3)
        out["speedup_vs_vanilla"] = round(value / vanilla_tps, 3)
        if not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(cfg, Ls, args.cpu_sample_calls, tau)
            if not args.no_cpu_round:
                out["cpu_baseline_round"] = cpu_baseline_round(TREE)
    if world > 1 or args.shard_path:
        if shard.peer is not None:
            shard.peer.close()
        dist.barrier()
        dist.destroy_process_group()
        # RCCL writes its version banner through C stdio, which a pipe buffers until exit: push it out now so that the
        # JSON line below is the LAST line of rank 0's stdout
        import ctypes
        ctypes.CDLL(None).fflush(None)
    if rank == 0:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
