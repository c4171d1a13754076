"""Oracle of ``ops.penalize_rows`` / ``ops.token_state_add`` (``ls_penalize_rows`` / ``ls_token_state_add``): the formula of
``longspec_amd/penalties.py`` in torch fp32 on the CPU, from counts -- a ``bincount`` over (generated tokens + the row's selected
extras) -- and whole-tensor steps, plus an operator namespace that lets the host loops run penalised on the CPU.  Every step is
one IEEE fp32 operation in a fixed order, so the kernel has to agree bit for bit.  ``mutant=`` selects one of the wrong variants
the case tables must tell from the right one.  Lives under tests/: the product never imports it."""
import numpy as np
import torch

import sampling_oracle

MUTANTS = ("no_extras", "dup_once", "prompt_as_count", "rep_generated_only", "freq_first", "bias_first", "other_row_mask")


def history_counts(state, R, extra_ids=None, extra_mask=None, mutant=None):
    """(count [b, R, V] int64 of every token in each row's generated history, prompt [b, 1, V] bool)."""
    b, V = state.shape
    word = state.to(torch.int64) & 0xFFFFFFFF
    gen, prompt = word & 0x7FFFFFFF, (word >> 31).bool()
    if mutant == "prompt_as_count":
        gen = gen + prompt.to(torch.int64)
    count = gen[:, None, :].repeat(1, R, 1)
    if extra_ids is not None and extra_ids.shape[-1] > 0 and mutant != "no_extras":
        mask = extra_mask if extra_mask.dim() == 3 else extra_mask[None].expand(b, -1, -1)
        for z in range(b):
            ids = extra_ids[z].to(torch.int64)
            inside = (ids >= 0) & (ids < V)
            for r in range(R):
                row = (r + 1) % R if mutant == "other_row_mask" else r
                chosen = ids[(mask[z, row] != 0) & inside]
                extra = torch.bincount(chosen, minlength=V)
                if mutant == "dup_once":
                    extra = extra.clamp(max=1)
                count[z, r] += extra
    return count, prompt[:, None, :]


def penalize_rows(logits, state, penalties, extra_ids=None, extra_mask=None, mutant=None, bias=None):
    """``longspec_amd.ops.penalize_rows`` on CPU tensors."""
    shape = logits.shape
    x = (logits if logits.dim() == 3 else logits.unsqueeze(1)).to(torch.float32).clone()
    b, R, V = x.shape
    count, prompt = history_counts(state, R, extra_ids, extra_mask, mutant)
    seen = count > 0
    full = lambda v: torch.full_like(x, float(np.float32(v)))        # an fp32 operand per element: no scalar shortcut
    rep, pres, freq = full(penalties.repetition), full(penalties.presence), full(penalties.frequency)
    bias = penalties.bias_table(V, "cpu") if bias is None else bias

    def repetition(x):
        touched = seen if mutant == "rep_generated_only" else seen | prompt
        return torch.where(touched, torch.where(x > 0, x / rep, x * rep), x)

    def presence_frequency(x):
        t = freq * count.to(torch.float32)
        return torch.where(seen, (x - t) - pres, x)

    def add_bias(x):
        return x + bias.view(1, 1, V) if bias is not None else x

    if mutant == "freq_first":
        x = add_bias(repetition(presence_frequency(x)))
    elif mutant == "bias_first":
        x = presence_frequency(repetition(add_bias(x)))
    else:
        x = add_bias(presence_frequency(repetition(x)))
    return x.to(logits.dtype).view(shape)


def token_state_add_np(state, ids, num=None, prompt=False):
    """numpy: state [b, V] int32 (returned updated, the input untouched), ids [b, n] int64, num [b] or None."""
    word = state.astype(np.int64) & 0xFFFFFFFF
    b, V = word.shape
    ids = np.asarray(ids).reshape(b, -1)
    for z in range(b):
        row = ids[z, :ids.shape[1] if num is None else max(0, min(int(num[z]), ids.shape[1]))]
        row = row[(row >= 0) & (row < V)]
        if prompt:
            word[z, np.unique(row)] |= 0x80000000
        else:
            word[z] += np.bincount(row, minlength=V)
    return (word & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def token_state_add(state, ids, num=None, prompt=False):
    """``longspec_amd.ops.token_state_add`` on CPU tensors (in place)."""
    b = state.shape[0]
    new = token_state_add_np(state.numpy(), ids.reshape(b, -1).numpy(), None if num is None else num.reshape(-1).numpy(), prompt)
    state.copy_(torch.from_numpy(new.copy()))


def state_of(prompt, text, V):
    """The state word table [1, V] a loop must hold after writing ``text`` behind ``prompt`` (1-D int64 tensors)."""
    word = torch.bincount(text, minlength=V).to(torch.int64)
    word[prompt.unique()] |= 0x80000000
    return torch.from_numpy((word.numpy() & 0xFFFFFFFF).astype(np.uint32).view(np.int32).copy())[None]


class Ops:
    """``sampling_oracle.ops`` plus the two penalty operators: the operator namespace of the penalised host-logic tests."""

    def __getattr__(self, name):
        return getattr(sampling_oracle.ops, name)

    penalize_rows = staticmethod(penalize_rows)
    token_state_add = staticmethod(token_state_add)


ops = Ops()
