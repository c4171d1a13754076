"""Word-stream oracle for ``ls_tree_verify_stochastic`` and the case table of its tests.

CPU only; nothing here imports ``longspec_amd``.  The kernel takes both random streams of the reference's walk pre-drawn:
raw 32-bit Mersenne-Twister words (what ``random.choice`` / ``random.random`` consume) and one Exponential(1) row (what
``torch.multinomial(p, 1)`` draws).  ``WordDraws`` is the ``draws`` object of ``oracle/ref_ops.py::verify_stochastic`` on exactly
those two arrays, so ``walk`` runs the oracle's own walk -- not a copy of it -- and reports what the kernel must return: the
accepted ids, their number and the number of words consumed.

``walk`` also reports how far every decision of the walk was from going the other way (``margins``).  The device rounds to
the activation type after every operation as torch does, but its ``expf`` and its summation order may differ from torch's
by one unit in the last place per rounded operation; an input whose decisions are all further away than that has ONE
correct answer, and the GPU tests compare exactly.  ``margin_bound`` is that rule; it is a condition on the inputs of
``CASES`` (tests/test_stochastic_oracle.py asserts it without a GPU), not a tolerance on the kernel.

``MUTANTS`` are wrong walks a kernel could plausibly implement; each must change the expected output of some case."""
from __future__ import annotations

import functools
import random

import numpy as np
import torch
from torch.overrides import TorchFunctionMode

import toy
from oracle import ref_ops

ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}
TT = 1024                    # threads of the kernel's workgroup: the stride of its vocabulary loops


class WordsExhausted(RuntimeError):
    """The walk asked for more Mersenne-Twister words than it was given (the kernel reports words_used = -1)."""


class ZeroDistribution(RuntimeError):
    """The final draw met an all-zero row: ``torch.multinomial`` raises there ("sum of probabilities <= 0")."""


class WordDraws:
    """``draws`` of ``ref_ops.verify_stochastic`` from given raw words and a given Exponential(1) row.

    choice(seq)     CPython's ``Random.choice``: ``seq[_randbelow(len(seq))]``, ``k = len.bit_length()``,
                    ``getrandbits(k)`` = one word ``>> (32 - k)``, redrawn while ``>= len``.
    random()        CPython's ``random_random``: ``((w0 >> 5) * 2**26 + (w1 >> 6)) / 2**53``.
    multinomial(p)  ATen's one-sample path: ``argmax(p / noise)`` in p's dtype, first maximum.

    Wrong variants (for the mutant test): ``last_max``, ``swap_shifts`` (random() from w0 >> 6 and w1 >> 5), ``no_redraw``
    (``getrandbits(k) % n`` instead of the redraw)."""

    def __init__(self, words, noise_row, last_max=False, swap_shifts=False, no_redraw=False):
        self.words = [int(w) & 0xFFFFFFFF for w in np.asarray(words).reshape(-1).tolist()]
        self.noise = noise_row
        self.used = 0
        self.last_max, self.swap_shifts, self.no_redraw = last_max, swap_shifts, no_redraw
        self.final = None            # (margin, top index) of the multinomial draw

    def _word(self):
        if self.used >= len(self.words):
            raise WordsExhausted(f"{len(self.words)} words were not enough")
        w = self.words[self.used]
        self.used += 1
        return w

    def choice(self, seq):
        n = len(seq)
        k = n.bit_length()
        r = self._word() >> (32 - k)
        if self.no_redraw:
            return seq[r % n]
        while r >= n:
            r = self._word() >> (32 - k)
        return seq[r]

    def random(self):
        if self.used + 2 > len(self.words):          # the kernel takes both words or none
            self.used = len(self.words)
            raise WordsExhausted(f"{len(self.words)} words were not enough")
        w0, w1 = self._word(), self._word()
        if self.swap_shifts:
            return ((w0 >> 6) * 67108864.0 + (w1 >> 5)) / 9007199254740992.0
        return ((w0 >> 5) * 67108864.0 + (w1 >> 6)) / 9007199254740992.0

    def multinomial(self, p_row):
        if not bool(p_row.sum() > 0):
            raise ZeroDistribution("invalid multinomial distribution (sum of probabilities <= 0)")
        v = p_row / self.noise.to(p_row.dtype)       # rounded to p's dtype
        V = v.numel()
        i = V - 1 - int(torch.argmax(v.flip(0))) if self.last_max else int(torch.argmax(v))
        top1 = float(v[i])
        rest = v.clone().double()
        rest[i] = -1.0
        top2 = float(rest.max()) if V > 1 else 0.0
        self.final = ((top1 - top2) / top1, i)
        return i


class _Watch(TorchFunctionMode):
    """Sees the oracle's own operands: every ``r <= ratio`` of the walk (both fp32 as compared), and counts the residual
    updates of the current row.  ``unnormalised``: the wrong walk that skips ``row / tot``."""

    def __init__(self, unnormalised=False):
        super().__init__()
        self.unnormalised = unnormalised
        self.n_res = 0
        self.margins = []

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = getattr(func, "__name__", "")
        if name in ("__le__", "le") and len(args) == 2 and all(torch.is_tensor(a) and a.dim() == 0 for a in args):
            r, ratio = float(args[0]), float(args[1])
            self.margins.append(dict(kind="accept", margin=abs(r - ratio) / max(ratio, 1e-30), n_res=self.n_res,
                                     r=r, ratio=ratio))
            self.n_res = 0 if r <= ratio else self.n_res + 1
        if (self.unnormalised and name in ("__truediv__", "div", "true_divide") and len(args) == 2
                and torch.is_tensor(args[0]) and args[0].dim() == 1 and torch.is_tensor(args[1]) and args[1].dim() == 0):
            return args[0]
        return func(*args, **kwargs)


def walk(spec, mask, logits, logp, T, words, noise, *, row=0, last_max=False, truncate=False, row0_words=False,
         row0_noise=False, swap_shifts=False, no_redraw=False, unnormalised=False, ignore_fs=False):
    """The reference's walk of ONE batch row on pre-drawn randomness.  spec [F] int64, mask [F,F], logits [F,V] in the
    activation type, logp [Fs,V] fp32, words [n] (or [b,n] with ``row``), noise [V] (or [b,V]).
    Returns (acc_ids [width], acc_num, words_used, margins); raises WordsExhausted / ZeroDistribution with the same
    fields as attributes (``.words_used``, ``.margins``).  The keyword flags are the wrong variants of ``MUTANTS``."""
    words = np.asarray(words)
    if words.ndim == 2:
        words = words[0 if row0_words else row]
    if noise.dim() == 2:
        noise = noise[0 if row0_noise else row]
    Fn, V = logits.shape
    Fs = logp.shape[0]
    if truncate and V - V % TT >= Fn:                # the strided loops stop at the last full stride
        V = V - V % TT
        logits, logp, noise = logits[:, :V], logp[:, :V], noise[:V]
    if ignore_fs:                                    # the draft row of cur is taken from min(cur, Fs-1)+1
        logp = logp[[min(min(c, Fs - 1) + 1, Fs - 1) for c in range(Fs)]]
    draws = WordDraws(words, noise, last_max=last_max, swap_shifts=swap_shifts, no_redraw=no_redraw)
    watch = _Watch(unnormalised)
    try:
        with watch:
            ids, num = ref_ops.verify_stochastic(spec[None], mask[None], logits[None].clone(), logp[None].clone(), T, draws)
    except (WordsExhausted, ZeroDistribution) as e:
        e.words_used, e.margins = draws.used, watch.margins
        raise
    margins = watch.margins + [dict(kind="final", margin=draws.final[0], n_res=watch.n_res, index=draws.final[1])]
    return ids[0], int(num[0]), draws.used, margins


def margin_bound(n_res, dtype):
    """One unit in the last place of the activation type per rounded operation the device may do differently (expf,
    summation order): the soft-max element and its sum, then one for the element and one for ``tot`` per residual update."""
    return 4 * (n_res + 1) * ULP[dtype]


# --------------------------------------------------------------------------- #
# the case table
# --------------------------------------------------------------------------- #
BIG = [4, 16, 16, 16, 16]
F16, BF16 = torch.float16, torch.bfloat16
N_WORDS = 384                # words handed to every case (a walk uses about three per child drawn)


def _case(name, kind, V, dtype, T, shapes, **kw):
    return dict(name=name, kind=kind, V=V, dtype=dtype, T=T, shapes=shapes, **kw)


# every case draws from seeds of its own: 100 * (its position in the table) + the bump listed here.  A bump is the smallest
# that makes the case meet margin_bound (`PYTHONPATH=. python tests/stochastic_oracle.py` lists them); it is chosen on the CPU, from the
# oracle alone, before any kernel sees the case.
_SEED_BUMP = {"sweep_V1024_bf16_T1.0": 1, "sweep_V2047_bf16_T0.5": 1, "strided_bf16": 1, "reject_all_64_2": 1}


def _cases():
    out = []
    dn = {F16: "f16", BF16: "bf16"}
    # vocabulary sweep: below / at / above one stride of the 1024 threads, ragged tails, several elements per thread
    for V in (1023, 1024, 1025, 2047, 4099, 33001):
        for dt in (F16, BF16):
            for T in (0.5, 1.0, 1.3):
                name = f"sweep_V{V}_{dn[dt]}_T{T}"
                out.append(_case(name, "random", V, dt, T, [BIG]))
    # production vocabularies
    out.append(_case("prod_V128256_f16", "random", 128256, F16, 0.8, [[4, 4]]))
    out.append(_case("prod_V152064_bf16", "random", 152064, BF16, 0.8, [[3]]))
    # first-maximum ties of the final draw: equal p / noise at `ties`, nothing larger.  EXEMPT from the final-draw margin
    # (it is 0 by construction: the row is uniform and the noise is 1 at `ties`, 2 elsewhere, so the tied values are the
    # same number whatever the soft-max rounds to); NOT exempt from the acceptance margins.
    # 5 and 1029 = 1024 + 5 are one thread's first and second element, 3000 is thread 952 (wave 14); the second case puts the
    # smallest index (70, wave 1) in a HIGHER thread than another tied one (1029 -> thread 5, wave 0; 2053 -> thread 5 again).
    out.append(_case("tie_5_1029_3000", "tie", 4099, F16, 1.0, [[1]], ties=(5, 1029, 3000), exempt_final=True))
    out.append(_case("tie_70_1029_2053_3000", "tie", 4099, BF16, 1.0, [[1]], ties=(70, 1029, 2053, 3000), exempt_final=True))
    # batch in one launch: three trees of equal F, separate word and noise rows
    out.append(_case("batch3_f16", "random", 2047, F16, 0.8, [BIG, BIG, BIG]))
    out.append(_case("batch3_bf16", "random", 1500, BF16, 1.0, [[4, 4]] * 3))
    # strides and Fs: views of larger buffers whose padding holds large finite values
    out.append(_case("strided_f16", "random", 1500, F16, 0.8, [BIG, BIG], strided=True))
    out.append(_case("strided_bf16", "random", 1025, BF16, 1.0, [[2, 2, 2]] * 2, strided=True))
    # child counts: every child of the root is rejected -> n draws, n residual updates, the word rejection of getrandbits
    for n in (1, 2, 3, 5, 16, 17, 64):
        for shape in ([n], [n, 2]):
            name = f"reject_all_{'_'.join(map(str, shape))}"
            out.append(_case(name, "reject_all", 1500, F16, 1.0, [shape]))
    for n in (2, 3, 5):
        name = f"reject_all_{n}_bf16"
        out.append(_case(name, "reject_all", 1100, BF16, 0.8, [[n]]))
    out.append(_case("accept_all_2x5", "accept_all", 1500, F16, 1.0, [[2, 2, 2, 2, 2]]))
    # depth limit: 13 accepted nodes + root + the final draw = 15 = the largest max_acc
    out.append(_case("chain13", "accept_all", 1500, F16, 1.0, [[1] * 13]))
    out.append(_case("chain13_bf16", "accept_all", 1100, BF16, 1.3, [[1] * 13]))
    out.append(_case("accept_all_3", "accept_all", 1500, F16, 0.8, [[3]]))      # the word-budget test walks this one too
    for i, c in enumerate(out):
        c["seed"] = 100 * i + _SEED_BUMP.get(c["name"], 0)
    return out


def build(case):
    """The inputs of a case on the CPU: dict(spec [b,F], mask [b,F,F], logits [b,F,V] (a view when strided), logp [b,Fs,V]
    fp32 (a view when strided), words [b,N_WORDS] uint32 numpy, noise [b,V], T, max_acc)."""
    return _build(case["name"])


@functools.lru_cache(maxsize=None)
def _build(name):
    case = BY_NAME[name]
    V, dt, seed, kind = case["V"], case["dtype"], case["seed"], case["kind"]
    shapes = case["shapes"]
    b = len(shapes)
    g = torch.Generator().manual_seed(77000 + seed)
    rng = random.Random(78000 + seed)
    masks = [torch.from_numpy(toy.tree_mask_from_parents(toy.random_beam_tree(s, 79000 + 10 * seed + z))).to(torch.int64)
             for z, s in enumerate(shapes)]
    Fn = masks[0].shape[0]
    assert all(m.shape[0] == Fn for m in masks) and V >= Fn
    strided = case.get("strided", False)
    Fs = Fn - shapes[0][-1] if strided else Fn       # strided: only the non-leaf levels have a draft row
    mask = torch.stack(masks)
    spec = torch.randint(2, V, (b, Fn), generator=g)
    lg = (torch.randn(b, Fn, V, generator=g) * 2.0)
    raw = torch.randn(b, Fs, V, generator=g) * 2.0
    noise = torch.empty(b, V, dtype=dt).exponential_(1, generator=g)
    kids = slice(1, Fn)                              # the vocabulary indices the acceptance ratios read: the node indices
    if kind == "reject_all":                         # target very low, draft very high at the child indices
        lg[:, :, kids] = -30.0
        raw[:, :, kids] = 8.0
    elif kind in ("accept_all", "tie"):
        lg[:, :, kids] = 12.0
        raw[:, :, kids] = -30.0
    if kind == "tie":                                # node 1 (the leaf the walk ends on): a uniform row
        lg[:, 1, :] = 0.0
        noise[:] = 2.0
        noise[:, list(case["ties"])] = 1.0
    assert bool((noise > 0).all())
    lg = lg.to(dt)
    lp = raw.log_softmax(dim=-1)
    if strided:
        a = 3
        big = torch.full((b, Fn + 5, V + 24), 30.0, dtype=dt)
        big[:, a - 1:a - 1 + Fn, :V] = lg
        lg = big[:, a - 1:a - 1 + Fn, :V]
        bigp = torch.full((b, Fs + 3, V + 16), 30.0, dtype=torch.float32)
        bigp[:, :Fs, :V] = lp
        lp = bigp[:, :Fs, :V]
    words = np.array([[rng.getrandbits(32) for _ in range(N_WORDS)] for _ in range(b)], dtype=np.uint32)
    max_acc = int(mask.sum(-1).max()) + 1
    return dict(spec=spec, mask=mask, logits=lg, logp=lp, words=words, noise=noise, T=case["T"], max_acc=max_acc, b=b)


def to_device(x, device, rows=None, n_words=None):
    """The tensors of ``build`` (rows ``rows`` of the batch, the first ``n_words`` words) on ``device``, in the argument order of
    ``ops.tree_verify_stochastic`` up to the noise.  Views stay views of a larger buffer: the buffer is moved, then sliced."""
    r = slice(None) if rows is None else rows

    def view(t):
        if t.is_contiguous():
            return t[r].to(device)
        base = t._base
        off = t.storage_offset()
        assert base is not None and base.is_contiguous()
        return torch.as_strided(base.to(device), t.shape, t.stride(), off)[r]

    words = x["words"][r, :n_words].copy()
    return (x["spec"][r].to(device), x["mask"][r].to(device), view(x["logits"]), view(x["logp"]), x["T"],
            torch.from_numpy(words.view(np.int32)).to(device), x["noise"][r].to(device))


def expected(case, **mutant):
    """[(acc_ids [max_acc], acc_num, words_used, margins)] per batch row of a case, from ``walk``."""
    if not mutant:
        return _expected(case["name"])
    x = build(case)
    return [walk(x["spec"][z], x["mask"][z], x["logits"][z], x["logp"][z], x["T"], x["words"], x["noise"], row=z, **mutant)
            for z in range(x["b"])]


@functools.lru_cache(maxsize=None)
def _expected(name):
    x = _build(name)
    return [walk(x["spec"][z], x["mask"][z], x["logits"][z], x["logp"][z], x["T"], x["words"], x["noise"], row=z)
            for z in range(x["b"])]


def violations(case):
    """The margins of a case that break margin_bound (the tie cases' final draw is exempt, as the table states)."""
    bad = []
    for z, (_, _, _, margins) in enumerate(expected(case)):
        for m in margins:
            if m["kind"] == "final" and case.get("exempt_final"):
                continue
            if not m["margin"] >= margin_bound(m["n_res"], case["dtype"]):
                bad.append((z, m))
    return bad


def zero_residual_inputs(V=1500, j=700, T=1.0, seed=5):
    """One-hot target and draft at the same index j (200 nats above the rest, so every other probability is exactly 0 in
    fp16 and in fp32), tree [3]: every child is rejected with ratio 0 and the residual row is all zero."""
    g = torch.Generator().manual_seed(77000 + seed)
    rng = random.Random(78000 + seed)
    mask = torch.from_numpy(toy.tree_mask_from_parents(toy.random_beam_tree([3], 79000 + seed))).to(torch.int64)[None]
    Fn = mask.shape[1]
    assert j >= Fn
    spec = torch.randint(2, V, (1, Fn), generator=g)
    lg = torch.full((1, Fn, V), -100.0)
    lg[:, :, j] = 100.0
    noise = torch.empty(1, V, dtype=F16).exponential_(1, generator=g)
    words = np.array([[rng.getrandbits(32) for _ in range(N_WORDS)]], dtype=np.uint32)
    return dict(spec=spec, mask=mask, logits=lg.to(F16), logp=lg.log_softmax(dim=-1), words=words, noise=noise, T=T,
                max_acc=3, b=1)


MUTANTS = {
    "last maximum instead of first": dict(last_max=True),
    "vocabulary truncated to V - V % 1024": dict(truncate=True),
    "row z reads row 0's words": dict(row0_words=True),
    "row z reads row 0's noise": dict(row0_noise=True),
    "random() from w0 >> 6 and w1 >> 5": dict(swap_shifts=True),
    "no redraw when getrandbits(k) >= n": dict(no_redraw=True),
    "residual not re-normalised": dict(unnormalised=True),
    "Fs ignored: draft row min(cur, Fs-1)+1": dict(ignore_fs=True),
}

CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


if __name__ == "__main__":                           # list, per case, the smallest seed that meets margin_bound
    for i, c in enumerate(CASES):
        for bump in range(100):
            c["seed"] = 100 * i + bump
            _build.cache_clear()
            _expected.cache_clear()
            try:
                if not violations(c):
                    break
            except (WordsExhausted, ZeroDistribution):
                continue
        if bump:
            print(f'    "{c["name"]}": {bump},')
