"""Replay a token sequence as if the target had produced it, through the prompt-lookup drafters: accepted tokens per round for
``branches`` 1 / 2 / 4 / 8 (and for a deeper chain).  Needs no model: a round accepts 1 + the longest common prefix of one of its
branches and what the sequence goes on with -- what ``lookup_generate`` does when the target's text is that sequence.

    python tools/lookup_replay.py FILE [FILE ...] [--prompt 6000] [--gen 1500] [--gamma 7] [--max-ngram 3] [--min-ngram 1]
                                  [--deep 15] [--kernel] [--json profiles/lookup_tree_replay.json]

A FILE is text, cut into word-level tokens (a run of word characters, a run of white space, or one other character), or a
``.npy`` / ``.pt`` of ids.  The first ``--prompt`` tokens are the prompt, the next ``--gen`` the generation.  The drafter is the
plain-Python definition (tests/lookup_oracle.py, tests/lookup_tree_oracle.py); ``--kernel`` drafts with ``ops.ngram_draft`` /
``ops.ngram_tree_draft`` on the GPU instead and must print the same table.  Word tokens are not the BPE tokens of a model: the
table ranks candidate rules and branch counts, it does not predict a model's acceptance."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BRANCHES = (1, 2, 4, 8)


def tokens_of(path):
    if path.endswith(".npy"):
        import numpy as np
        return [int(x) for x in np.load(path).reshape(-1)]
    if path.endswith(".pt"):
        import torch
        return [int(x) for x in torch.load(path).reshape(-1)]
    with open(path, encoding="utf-8", errors="replace") as f:
        words = re.findall(r"\w+|\s+|[^\w\s]", f.read())
    ids = {}
    return [ids.setdefault(w, len(ids)) for w in words]


def common(a, b):
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


class OracleDrafter:
    def slots(self, text, gamma, branches, mx, mn):
        import lookup_oracle
        import lookup_tree_oracle
        if branches == 1:
            return [lookup_oracle.draft(text, gamma, mx, mn)[0]]
        return lookup_tree_oracle.tree_draft(text, gamma, branches, mx, mn)[0]


class KernelDrafter:
    """The same question put to the device: the sequence sits in a prompt and an output buffer as in ``lookup_generate``."""

    def __init__(self, ids, prompt):
        import torch
        self.torch, self.P = torch, prompt
        dev = torch.device("cuda", 0)
        self.prompt = torch.tensor([ids[:prompt]], dtype=torch.int64, device=dev)
        self.out = torch.tensor([ids[prompt:] + [0] * 8], dtype=torch.int64, device=dev)
        self.il = torch.tensor([prompt], dtype=torch.int32, device=dev)
        self.bound = len(ids) + 8

    def slots(self, text, gamma, branches, mx, mn):
        from longspec_amd import ops
        torch, dev = self.torch, self.prompt.device
        w = len(text) - self.P
        if branches == 1:
            spec = torch.zeros((1, gamma + 1), dtype=torch.int64, device=dev)
            ops.ngram_draft(self.prompt, self.il, self.out, torch.tensor([len(text) - 1], dtype=torch.int32, device=dev), self.bound,
                            gamma, mx, mn, spec)
            return [spec[0, 1:].tolist()]
        F = 1 + branches * gamma
        spec = torch.zeros((1, F), dtype=torch.int64, device=dev)
        mask = torch.zeros((1, F, F), dtype=torch.int64, device=dev)
        ops.ngram_tree_draft(self.prompt, self.il, self.out, torch.tensor([w], dtype=torch.int32, device=dev), self.bound, gamma,
                             branches, mx, mn, spec, mask)
        return spec[0, 1:].view(gamma, branches).t().tolist()


def replay(ids, prompt, gen, gamma, branches, mx, mn, drafter):
    """(accepted tokens per round, rounds) over ids[prompt : prompt + gen] with ids[:prompt + 1] known at the start."""
    end = min(len(ids), prompt + gen)
    w, rounds = prompt + 1, 0                                          # the first generated token comes from the prefill
    while w < end:
        slots = drafter.slots(ids[:w], gamma, branches, mx, mn)
        w += 1 + max(common(s, ids[w:end]) for s in slots)
        rounds += 1
    return (min(w, end) - prompt - 1) / max(rounds, 1), rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="+")
    ap.add_argument("--prompt", type=int, default=6000)
    ap.add_argument("--gen", type=int, default=1500)
    ap.add_argument("--gamma", type=int, default=7)
    ap.add_argument("--max-ngram", type=int, default=3)
    ap.add_argument("--min-ngram", type=int, default=1)
    ap.add_argument("--deep", type=int, default=15, help="gamma of the deeper chain in the last column (0: none)")
    ap.add_argument("--kernel", action="store_true", help="draft with the HIP kernels (needs the GPU)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    out = {"what": f"accepted tokens per round when the text itself is replayed as the target's output: word-level ids, "
                   f"{args.prompt} prompt tokens, the next {args.gen} generated, gamma {args.gamma}, n-grams "
                   f"{args.min_ngram}..{args.max_ngram}; drafter: {'HIP kernels' if args.kernel else 'plain-Python definition'}",
           "texts": {}}
    print(f"{'text':28s}" + "".join(f"  B = {b:<4d}" for b in BRANCHES) + (f"  chain, gamma {args.deep}" if args.deep else ""))
    for path in args.files:
        ids = tokens_of(path)
        if len(ids) < args.prompt + 16:
            print(f"{os.path.basename(path):28s}  only {len(ids)} tokens: skipped")
            continue
        drafter = KernelDrafter(ids[:args.prompt + args.gen], args.prompt) if args.kernel else OracleDrafter()
        row = {"tokens": len(ids), "tokens_per_round": {}}
        for b in BRANCHES:
            row["tokens_per_round"][str(b)] = replay(ids, args.prompt, args.gen, args.gamma, b, args.max_ngram, args.min_ngram, drafter)[0]
        if args.deep:
            row["chain_deep"] = {"gamma": args.deep,
                                 "tokens_per_round": replay(ids, args.prompt, args.gen, args.deep, 1, args.max_ngram, args.min_ngram, drafter)[0]}
        out["texts"][os.path.basename(path)] = row
        print(f"{os.path.basename(path):28s}" + "".join(f"  {row['tokens_per_round'][str(b)]:<8.2f}" for b in BRANCHES)
              + (f"  {row['chain_deep']['tokens_per_round']:.2f}" if args.deep else ""), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
