"""The set-up cost of a guide on ONE box: ``Guide.from_byte_dfa`` on the host against the lift on the device, and the whole of
``Guide.from_regex`` for a record-like pattern.

    python tools/guide_lift_time.py [--states 16 128 512 1024] [--tokens 128256] [--repeat 3] [--out profiles/guide_lift.json]

The vocabulary: `tokens` random byte strings of 1-9 bytes over letters, digits, the space and the full stop.  The DFA: a counter
-- a digit advances the state, a letter stays, every other byte is dead.  Per S the host path is timed once (it takes seconds)
and the device path `repeat` times behind a warm-up call, the smallest kept; the device path's time is the whole call, uploads
of the step table and the vocabulary and the host's class numbering included, and is split into the three operators (each
between device synchronisations, which the product path does not have) and the rest: hash grouping, copies and numbering."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECORD = (r'\{"name": "[A-Za-z][a-z]{0,15}( [A-Za-z][a-z]{0,15}){0,2}", "age": (0|[1-9]\d{0,2}), '
          r'"email": "\w{1,12}@\w{1,12}\.(com|org|net)", "member": (true|false)\}')


def counter_dfa(S):
    import numpy as np
    nx = np.full((S, 256), -1, dtype=np.int64)
    for b in b"0123456789":
        nx[:S - 1, b] = np.arange(1, S)
    for b in range(128):
        if chr(b).isalpha():
            nx[:, b] = np.arange(S)
    return nx


def vocabulary(T, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    src = np.frombuffer(b'abcdefghijklmnopqrstuvwxyzABCDEFGH0123456789 .@{}":,', dtype=np.uint8)
    lens = rng.integers(1, 10, size=T)
    flat = src[rng.integers(0, src.size, size=int(lens.sum()))].tobytes()
    ends = np.cumsum(lens)
    return [flat[e - n:e] for e, n in zip(ends.tolist(), lens.tolist())]


class Split:
    """The three operators of ``ops`` timed between device synchronisations."""

    NAMES = ("guide_lift_hash", "guide_lift_cols", "guide_lift_check")

    def __init__(self, ops, torch):
        self.ops, self.torch, self.real, self.ms = ops, torch, {}, {}

    def __enter__(self):
        for name in self.NAMES:
            self.real[name] = getattr(self.ops, name)
            setattr(self.ops, name, self.timed(name))
        return self

    def __exit__(self, *exc):
        for name, fn in self.real.items():
            setattr(self.ops, name, fn)

    def timed(self, name):
        def call(*a, **k):
            self.torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = self.real[name](*a, **k)
            self.torch.cuda.synchronize()
            self.ms[name] = self.ms.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
            return out
        return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, nargs="+", default=[16, 128, 512, 1024])
    ap.add_argument("--tokens", type=int, default=128256)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from longspec_amd import Guide, ops, regex
    toks = vocabulary(a.tokens)
    result = {"tokens": a.tokens, "device": torch.cuda.get_device_name(0), "sizes": []}
    for S in a.states:
        nx = counter_dfa(S)
        t0 = time.perf_counter()
        host = Guide.from_byte_dfa(nx, toks)
        host_ms = (time.perf_counter() - t0) * 1e3
        dev = Guide.from_byte_dfa(nx, toks, device="cuda")            # warm-up: the library, the allocator
        assert dev == host, S
        whole = []
        for _ in range(a.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            Guide.from_byte_dfa(nx, toks, device="cuda")
            whole.append((time.perf_counter() - t0) * 1e3)
        with Split(ops, torch) as split:
            t0 = time.perf_counter()
            Guide.from_byte_dfa(nx, toks, device="cuda")
            split_whole = (time.perf_counter() - t0) * 1e3
        row = dict(S=S, classes=host.classes, host_ms=round(host_ms, 1), device_ms=round(min(whole), 2),
                   hash_ms=round(split.ms["guide_lift_hash"], 3), cols_ms=round(split.ms["guide_lift_cols"], 3),
                   check_ms=round(split.ms["guide_lift_check"], 3),
                   rest_ms=round(split_whole - sum(split.ms.values()), 2), ratio=round(host_ms / min(whole), 1))
        result["sizes"].append(row)
        print(json.dumps(row), flush=True)
    eos = a.tokens - 1
    t0 = time.perf_counter()
    dfa = regex.compile(RECORD)
    compile_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    host = Guide.from_regex(RECORD, toks, eos)
    host_ms = (time.perf_counter() - t0) * 1e3
    whole = []
    for _ in range(a.repeat + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = Guide.from_regex(RECORD, toks, eos, device="cuda")
        whole.append((time.perf_counter() - t0) * 1e3)
    assert dev == host
    row = dict(pattern=RECORD, byte_states=int(dfa.next.shape[0]), states=host.states, classes=host.classes,
               compile_ms=round(compile_ms, 1), from_regex_host_ms=round(host_ms, 1), from_regex_device_ms=round(min(whole[1:]), 1))
    result["record"] = row
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
