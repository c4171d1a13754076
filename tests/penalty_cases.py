"""Case table of ``ops.penalize_rows``, shared by the GPU test (kernel against tests/penalty_oracle.py, bit for bit) and the
CPU test that every wrong variant of the oracle changes the expected output of some case.  A case: ``logits`` [b, R, V],
``state`` [b, V] int32, ``pen`` (a ``Penalties``), ``extra_ids`` [b, C] / ``extra_mask`` [b, R, C] or [R, C] (or None), all
on the CPU and never modified."""
import math

import numpy as np
import torch

import toy
from longspec_amd import Penalties

ALL = Penalties(repetition=1.3, presence=0.5, frequency=0.25)
SCALARS = {"rep": Penalties(repetition=1.3), "rep_below_1": Penalties(repetition=0.5), "pres": Penalties(presence=0.5),
           "freq": Penalties(frequency=0.25), "neg": Penalties(presence=-0.75, frequency=-0.125), "all": ALL,
           "none": Penalties()}
TREE = [4, 16, 16, 16, 16]


def _word(count, prompt):
    return int(np.array([(count & 0x7FFFFFFF) | (0x80000000 if prompt else 0)], dtype=np.uint32).view(np.int32)[0])


def random_state(b, V, g):
    """About V/6 generated tokens (counts 1..3) and V/6 prompt tokens per batch row, overlapping; never empty."""
    state = torch.zeros((b, V), dtype=torch.int32)
    n = max(2, V // 6)
    for z in range(b):
        gen = torch.randperm(V, generator=g)[:n]
        state[z, gen] = torch.randint(1, 4, (n,), generator=g, dtype=torch.int32)
        pr = torch.cat([torch.randperm(V, generator=g)[:n], gen[:max(1, n // 3)]])
        state[z, pr] = torch.from_numpy((state[z, pr].numpy().view(np.uint32) | np.uint32(0x80000000)).view(np.int32))
    return state


def random_logits(b, R, V, dtype, g):
    x = (torch.randn(b, R, V, generator=g) * 4.0).to(dtype)
    flat = x.view(-1)
    k = max(1, flat.numel() // 32)
    flat[torch.randperm(flat.numel(), generator=g)[:k]] = -math.inf
    return x


def random_extras(b, R, C, V, state, g, mask2d=False):
    """C ids per batch row: a third taken from the row's state tokens, duplicates, two outside the vocabulary; a random mask
    whose set entries are not all 1."""
    ids = torch.randint(0, V, (b, C), generator=g)
    for z in range(b):
        known = state[z].nonzero().view(-1)
        m = C // 3
        if m:
            ids[z, :m] = known[torch.randint(0, known.numel(), (m,), generator=g)]
        if C >= 4:
            ids[z, C - 1] = ids[z, C - 2]                      # a duplicate
        if C >= 8:
            ids[z, C // 2] = V + 3                             # outside the vocabulary, both ways
            ids[z, C // 2 + 1] = -2
    shape = (R, C) if mask2d else (b, R, C)
    mask = (torch.rand(shape, generator=g) < 0.4).to(torch.int64) * torch.randint(1, 9, shape, generator=g)
    return ids, mask


def make(name, b, R, V, dtype, C, pen, seed, mask2d=False, bias=None):
    g = torch.Generator().manual_seed(seed)
    state = random_state(b, V, g)
    case = dict(name=name, logits=random_logits(b, R, V, dtype, g), state=state, pen=pen, extra_ids=None, extra_mask=None)
    if C:
        case["extra_ids"], case["extra_mask"] = random_extras(b, R, C, V, state, g, mask2d)
    if bias:
        case["pen"] = Penalties(pen.repetition, pen.presence, pen.frequency, bias=bias)
    return case


def tree_case(dtype, V=8200, seed=11):
    """The real 4/16/16/16/16 tree: a seeded father assignment, masks as ``tree_grow`` builds them (a node's row = its father's
    row + itself, root column set), ``extra_ids = all_spec[:, 1:]``, ``extra_mask = tree_mask[:, :, 1:]`` -- the views the
    round passes.  One leaf's path holds a token the state counts (column 7), a prompt-only one (column 8), a new one (column
    8191) and that one again; other nodes hold columns 0, 8192, V - 1 and two ids outside the vocabulary, each under a set
    mask (its own row and its descendants') and under a zero mask (every other row)."""
    parents = toy.random_beam_tree(TREE, 9500 + seed)
    mask = torch.from_numpy(toy.tree_mask_from_parents(parents))[None].to(torch.int64).contiguous()
    Fn = mask.shape[1]
    g = torch.Generator().manual_seed(seed)
    state = random_state(1, V, g)
    state[0, 7], state[0, 8], state[0, 8191] = _word(2, False), _word(0, True), 0
    state[0, 0], state[0, 8192], state[0, V - 1] = _word(1, True), 0, _word(3, False)
    spec = torch.randint(0, V, (1, Fn), generator=g)
    leaf = Fn - 1
    path = []
    while leaf != 0:
        path.append(leaf)
        leaf = int(parents[leaf])
    path = path[::-1]                                          # levels 1 .. 5
    assert len(path) == 5
    for node, tok in zip(path, (7, 8, 8191, 8191, 8192)):
        spec[0, node] = tok
    others = [n for n in range(1, Fn) if n not in path]
    inner = [n for n in others if (parents == n).any()]        # nodes with descendants: their mask column is set in other rows
    spec[0, inner[0]], spec[0, inner[1]] = V + 3, -1
    spec[0, inner[2]], spec[0, others[-1]], spec[0, others[-2]] = 0, V - 1, 8192
    return dict(name=f"tree-{dtype}", logits=random_logits(1, Fn, V, dtype, g), state=state, pen=ALL, extra_ids=spec[:, 1:],
                extra_mask=mask[:, :, 1:])


def special_values_case(dtype, pen, name):
    """+-0, -inf, the largest finite value (overflows under repetition), subnormals, negative and positive logits, each at a
    generated token, a prompt-only token and an untouched one (V = 1032, R = 2)."""
    V, R = 1032, 2
    fin = torch.finfo(dtype)
    tiny_sub = fin.smallest_normal / 4
    vals = [0.0, -0.0, -math.inf, fin.max, -fin.max, tiny_sub, -tiny_sub, fin.smallest_normal, 2.5, -2.5, 1e-3, -1e-3, 7.0, -7.0]
    x = torch.zeros((1, R, V), dtype=dtype)
    state = torch.zeros((1, V), dtype=torch.int32)
    for i, v in enumerate(vals * 3):
        col = 5 + 3 * i
        x[0, :, col] = v
        kind = i // len(vals)
        state[0, col] = (_word(2, False), _word(0, True), 0)[kind]
    ids = torch.tensor([[5 + 3 * i for i in range(2 * len(vals), 3 * len(vals))]], dtype=torch.int64)      # row 1: the untouched ones, on its path
    mask = torch.zeros((1, R, ids.shape[1]), dtype=torch.int64)
    mask[0, 1] = 1
    return dict(name=f"{name}-{dtype}", logits=x, state=state, pen=pen, extra_ids=ids, extra_mask=mask)


def chain_case(dtype, b=3, gamma=4, V=1032, seed=5):
    """The chain's constant strictly-lower-triangular [gamma + 1, gamma] mask, one for all batch rows (batch stride 0)."""
    case = make(f"chain-{dtype}", b, gamma + 1, V, dtype, gamma, ALL, seed, mask2d=True)
    case["extra_mask"] = torch.ones((gamma + 1, gamma), dtype=torch.int64).tril(-1)
    case["extra_ids"][:, 1] = case["extra_ids"][:, 0]         # the same draft token twice
    return case


def small_case(dtype):
    """V = 8: every column hand-set."""
    x = torch.tensor([[[1.5, -1.5, 0.25, 3.0, -0.0, -math.inf, 2.0, -4.0]]], dtype=dtype)
    state = torch.tensor([[_word(1, False), _word(2, True), _word(0, True), 0, _word(5, False), _word(1, False), 0, 0]],
                         dtype=torch.int32)
    ids = torch.tensor([[3, 3, 7, 9]], dtype=torch.int64)
    return dict(name=f"v8-{dtype}", logits=x, state=state, pen=ALL, extra_ids=ids,
                extra_mask=torch.tensor([[[1, 2, 0, 1]]], dtype=torch.int64))


def _build():
    out = []
    seed = 100
    for dtype in (torch.float16, torch.bfloat16):
        out.append(small_case(dtype))
        for V in (1016, 1024, 1032, 8200):
            for R in (1, 5, 69):
                seed += 1
                out.append(make(f"V{V}-R{R}-{dtype}", 1, R, V, dtype, 12, ALL, seed))
        out.append(make(f"b3-V1032-R5-{dtype}", 3, 5, 1032, dtype, 12, ALL, seed + 50))
        out.append(make(f"b3-V8200-R69-{dtype}", 3, 69, 8200, dtype, 68, ALL, seed + 51))
        out.append(make(f"C0-{dtype}", 1, 5, 1032, dtype, 0, ALL, seed + 52))
        out.append(make(f"C1024-{dtype}", 1, 3, 1032, dtype, 1024, ALL, seed + 53))
        out.append(make(f"C300-{dtype}", 1, 3, 8200, dtype, 300, ALL, seed + 54))
        out.append(tree_case(dtype))
        out.append(chain_case(dtype))
        for key, pen in SCALARS.items():
            out.append(make(f"{key}-{dtype}", 1, 5, 1032, dtype, 12, pen, seed + 60))
            out.append(special_values_case(dtype, pen, f"special-{key}"))
        bias = {0: -math.inf, 7: 1.5, 8: -2.25, 1031: -math.inf, 500: 0.0, 16: 1e-3}
        out.append(make(f"bias-only-{dtype}", 1, 5, 1032, dtype, 12, Penalties(), seed + 61, bias=bias))
        out.append(make(f"bias-all-{dtype}", 1, 5, 1032, dtype, 12, ALL, seed + 62, bias=bias))
        out.append(special_values_case(dtype, Penalties(1.3, 0.5, 0.25, bias={5 + 3 * i: (-1.0, -math.inf)[i % 2] for i in range(42)}),
                                       "special-bias"))
    for V in (128256, 152064):                                  # the real vocabularies, 5 rows
        out.append(make(f"V{V}-R5-fp16", 1, 5, V, torch.float16, 68, ALL, V))
    out.append(make("V128256-R5-bf16", 1, 5, 128256, torch.bfloat16, 68, ALL, 77))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES
