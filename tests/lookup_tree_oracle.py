"""Oracle of ``ops.ngram_tree_draft`` (``ls_ngram_tree_draft``): the tree drafter's definition of ``longspec_amd/lookup.py`` in
plain Python, and an operator namespace layered on ``lookup_oracle.ops`` that lets ``lookup_generate(branches=B)`` run on the
CPU.  Lives under tests/: the product never imports it."""
import lookup_oracle

TOP = 8                                # LS_NGRAM_TOP


def candidates(text, max_ngram, min_ngram):
    """Every candidate end as (m, e), best first: the key (m, e) descending."""
    L = len(text)
    found = []
    for e in range(1, L):
        m = 0
        while m < min(max_ngram, e) and text[e - 1 - m] == text[L - 1 - m]:
            m += 1
        if m >= max(min_ngram, 1):
            found.append((m, e))
    return sorted(found, reverse=True)


def continuation(text, e, gamma):
    L = len(text)
    return [text[e + i % (L - e)] for i in range(gamma)]


def tree_draft(text, gamma, branches, max_ngram, min_ngram):
    """(slots [branches][gamma], info [branches] of (n, e), nb)."""
    kept = []
    for m, e in candidates(text, max_ngram, min_ngram)[:TOP]:
        c = continuation(text, e, gamma)
        if len(kept) < branches and all(c != k[0] for k in kept):
            kept.append((c, (m, e)))
    nb = len(kept)
    if nb == 0:
        first = [text[-1] if text else 0] * gamma
        return [list(first) for _ in range(branches)], [(0, -1)] * branches, 0
    slots = [list(k[0]) for k in kept] + [list(kept[0][0]) for _ in range(branches - nb)]
    return slots, [k[1] for k in kept] + [(0, -1)] * (branches - nb), nb


def node(d, j, branches):
    """Index of branch j's node at depth d = 1..gamma: level-major, the root is node 0."""
    return 1 + (d - 1) * branches + j


def tree_layout(slots, gamma, branches):
    """(all_spec[1:], mask rows 1..) of the static tree: lists of F - 1 ids and of F - 1 rows of F ints."""
    F = 1 + branches * gamma
    spec = [0] * F
    mask = [[0] * F for _ in range(F)]
    for j in range(branches):
        for d in range(1, gamma + 1):
            r = node(d, j, branches)
            spec[r] = slots[j][d - 1]
            mask[r][0] = 1
            for dd in range(1, d + 1):
                mask[r][node(dd, j, branches)] = 1
    return spec[1:], mask[1:]


def text_of(prompt_ids, input_len, output_ids, written, z):
    il = min(max(int(input_len[z]), 0), prompt_ids.shape[1])
    w = min(max(int(written[z]), 0), output_ids.shape[1])
    return prompt_ids[z, :il].tolist() + output_ids[z, :w].tolist()


def ngram_tree_draft(prompt_ids, input_len, output_ids, written, len_bound, gamma, branches, max_ngram, min_ngram, all_spec,
                     tree_mask, info=None, hist=None, hist_nb=None):
    """``longspec_amd.ops.ngram_tree_draft`` on CPU tensors (in place, exact; ``len_bound`` must bound every text)."""
    import torch
    b = output_ids.shape[0]
    if info is None:
        info = torch.empty((b, branches, 2), dtype=torch.int32)
    for z in range(b):
        text = text_of(prompt_ids, input_len, output_ids, written, z)
        assert len(text) <= len_bound, "the host's bound is no bound"
        slots, ne, nb = tree_draft(text, gamma, branches, max_ngram, min_ngram)
        spec, rows = tree_layout(slots, gamma, branches)
        all_spec[z, 1:] = torch.tensor(spec, dtype=torch.int64)
        tree_mask[z, 1:] = torch.tensor(rows, dtype=torch.int64)
        info[z] = torch.tensor(ne, dtype=torch.int32)
        if hist is not None:
            hist[z, ne[0][0]] += 1
        if hist_nb is not None:
            hist_nb[z, nb] += 1
    return info


class Ops:
    """``lookup_oracle.ops`` plus the tree drafter: the operator namespace of the tree lookup host-logic tests."""

    def __getattr__(self, name):
        return getattr(lookup_oracle.ops, name)

    ngram_tree_draft = staticmethod(ngram_tree_draft)


ops = Ops()
