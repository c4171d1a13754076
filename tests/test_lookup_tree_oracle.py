"""Cases that pin tests/lookup_tree_oracle.py, the plain-Python definition of the tree drafter of prompt-lookup speculation
(``longspec_amd/lookup.py``).  Every input goes through the oracle AND through a brute force written independently here (all
windows compared as tuples, no early exits, the tree built from ancestor sets); both must satisfy the same checks, and the
expectations of the hand cases were worked out from the definition, not from either."""
import numpy as np
import pytest
import torch

import lookup_oracle as lo
import lookup_tree_oracle as lt


def brute(text, gamma, B, mx, mn):
    """(slots, info, nb, all_spec[1:], mask rows 1..) straight from the definition's sentences."""
    L = len(text)
    keys = []
    for e in range(1, L):
        ms = [k for k in range(1, min(mx, e) + 1) if tuple(text[e - k:e]) == tuple(text[L - k:L])]
        if ms and max(ms) >= mn:
            keys.append((max(ms), e))
    keys.sort(key=lambda me: (-me[0], -me[1]))
    seen, kept = set(), []
    for m, e in keys[:8]:
        cont = tuple((text[e:] * gamma)[:gamma])              # T[e:] repeated: the periodic extension
        if cont not in seen and len(kept) < B:
            seen.add(cont)
            kept.append((cont, m, e))
    nb = len(kept)
    if nb:
        slots = [list(kept[j][0]) if j < nb else list(kept[0][0]) for j in range(B)]
        info = [(kept[j][1], kept[j][2]) if j < nb else (0, -1) for j in range(B)]
    else:
        slots, info = [[text[-1] if L else 0] * gamma for _ in range(B)], [(0, -1)] * B
    # the tree from ancestor sets: nodes in level order, the ancestors of (d, j) are (1..d, j) and the root
    order = [(0, 0)] + [(d, j) for d in range(1, gamma + 1) for j in range(B)]
    spec = [slots[j][d - 1] for d, j in order[1:]]
    rows = [[int((dd, jj) == (0, 0) or (jj == j and 1 <= dd <= d)) for dd, jj in order] for d, j in order[1:]]
    return slots, info, nb, spec, rows


def both(text, gamma, B, mx, mn):
    """The oracle's and the brute force's answer, checked for the properties every answer has; returns the oracle's."""
    slots, info, nb = lt.tree_draft(text, gamma, B, mx, mn)
    spec, rows = lt.tree_layout(slots, gamma, B)
    for s, i, n, sp, rw in ((slots, info, nb, spec, rows), brute(text, gamma, B, mx, mn)):
        assert (s, list(i), n, sp, rw) == (slots, list(info), nb, spec, rows)
        assert len(s) == B and all(len(x) == gamma for x in s) and 0 <= n <= B
        if text:
            d, n0, e0 = lo.draft(text, gamma, mx, mn)
            assert s[0] == d and tuple(i[0]) == (n0, e0), "slot 0 is the chain's draft"
        assert len({tuple(x) for x in s[:n]}) == n, "kept continuations are pairwise distinct"
        assert [tuple(k) for k in i[:n]] == sorted((tuple(k) for k in i[:n]), reverse=True), "... and in key order"
        assert all(x == s[0] for x in s[n:]) and all(tuple(k) == (0, -1) for k in i[n:]), "padding slots copy slot 0"
        assert all(k[0] >= mn for k in i[:n])
        F = 1 + B * gamma
        assert len(sp) == F - 1 and len(rw) == F - 1 and all(len(r) == F for r in rw)
        for j in range(B):
            for d in range(1, gamma + 1):
                r = 1 + (d - 1) * B + j                                   # level-major
                assert sp[r - 1] == s[j][d - 1]
                assert sum(rw[r - 1]) == d + 1 and rw[r - 1][0] == 1 and all(rw[r - 1][1 + (dd - 1) * B + j] for dd in range(1, d + 1))
    return slots, info, nb


def test_the_cap_of_eight_candidates():
    # the suffix 5 occurs nine times before: the oldest is followed by 7, the eight later ones by 6
    text = [5, 7] + [5, 6] * 8 + [5]
    slots, info, nb = both(text, 1, 4, 1, 1)
    assert nb == 1 and slots == [[6]] * 4 and info[0] == (1, 17)
    # with seven later ones the oldest is among the eight and is new
    slots, info, nb = both([5, 7] + [5, 6] * 7 + [5], 1, 4, 1, 1)
    assert nb == 2 and slots == [[6], [7], [6], [6]] and info == [(1, 15), (1, 1), (0, -1), (0, -1)]


def test_distinct_continuations_in_key_order_and_the_stop_at_B():
    #       0  1  2  3  4  5  6  7  8  9 10 11 12 13
    text = [1, 2, 7, 9, 2, 8, 1, 2, 7, 3, 2, 6, 1, 2]
    # (1, 2) ends at 2 and 8 (both followed by 7 ...), the lone 2 at 5 and 11
    slots, info, nb = both(text, 2, 4, 2, 1)
    assert info == [(2, 8), (2, 2), (1, 11), (1, 5)] and nb == 4
    assert slots == [[7, 3], [7, 9], [6, 1], [8, 1]]
    slots, info, nb = both(text, 1, 4, 2, 1)                           # one token deep the two 7s are the same draft
    assert nb == 3 and info == [(2, 8), (1, 11), (1, 5), (0, -1)] and slots == [[7], [6], [8], [7]]
    slots, info, nb = both(text, 2, 2, 2, 1)
    assert nb == 2 and info == [(2, 8), (2, 2)]
    assert both(text, 2, 3, 2, 2)[2] == 2                              # min_ngram = 2 leaves the two long ones


def test_a_periodic_text_has_one_continuation():
    for gamma in (1, 4, 15):
        slots, info, nb = both([1, 2, 3] * 5, gamma, 8, 3, 1)
        assert nb == 1 and slots[0] == ([1, 2, 3] * 5)[:gamma] and info[0] == (3, 12)


def test_all_equal_and_the_shortest_texts():
    slots, info, nb = both([4] * 10, 3, 2, 8, 1)
    assert nb == 1 and slots == [[4, 4, 4]] * 2 and info == [(8, 9), (0, -1)]
    assert both([9], 3, 2, 3, 1) == ([[9, 9, 9]] * 2, [(0, -1)] * 2, 0)
    assert both([], 2, 3, 3, 1) == ([[0, 0]] * 3, [(0, -1)] * 3, 0)
    assert both([6, 6], 2, 2, 8, 1) == ([[6, 6]] * 2, [(1, 1), (0, -1)], 1)
    assert both([6, 7], 2, 2, 8, 1) == ([[7, 7]] * 2, [(0, -1)] * 2, 0)


@pytest.mark.parametrize("gamma,B,mx,mn", [(1, 2, 1, 1), (4, 4, 3, 1), (8, 8, 2, 1), (15, 4, 8, 2), (7, 3, 3, 1)])
def test_random_texts_over_few_ids(gamma, B, mx, mn):
    rng = np.random.default_rng(gamma * 10 + B)
    full = 0
    for L in (2, 3, 9, 40, 200):
        for ids in (2, 4):
            full += both(rng.integers(0, ids, L).tolist(), gamma, B, mx, mn)[2] == B
    assert full >= 1


def test_the_operator_reads_only_the_text_and_keeps_the_root():
    prompt = torch.tensor([[1, 2, 3, 77, 77], [4, 4, 4, 4, 4]])                     # row 0: two columns of padding
    out = torch.tensor([[9, 1, 2, 5, 1, 2, 3, 55], [4, 4, 0, 0, 0, 0, 0, 0]])      # row 0: a stale id behind w = 7
    input_len = torch.tensor([3, 5], dtype=torch.int32)
    written = torch.tensor([7, 1], dtype=torch.int32)
    g, B = 2, 2
    F = 1 + g * B
    spec = torch.full((2, F), -7)
    mask = torch.full((2, F, F), -3)
    hist = torch.zeros((2, 4), dtype=torch.int64)
    hist_nb = torch.zeros((2, B + 1), dtype=torch.int64)
    info = lt.ngram_tree_draft(prompt, input_len, out, written, 16, g, B, 3, 1, spec, mask, hist=hist, hist_nb=hist_nb)
    # row 0: T = 1 2 3 9 1 2 5 1 2 3: (1, 2, 3) ends at 3 -> 9 1; the lone 3 nowhere else; (2, 3)... only e = 3 matches at all
    # row 1: T = 4 4 4 4 4 4: every end drafts 4 4
    assert info.tolist() == [[[3, 3], [0, -1]], [[3, 5], [0, -1]]]
    assert spec.tolist() == [[-7, 9, 9, 1, 1], [-7, 4, 4, 4, 4]]
    assert (mask[:, 0] == -3).all()
    assert mask[0, 1:].tolist() == [[1, 1, 0, 0, 0], [1, 0, 1, 0, 0], [1, 1, 0, 1, 0], [1, 0, 1, 0, 1]]
    assert hist.tolist() == [[0, 0, 0, 1]] * 2 and hist_nb.tolist() == [[0, 1, 0]] * 2
    with pytest.raises(AssertionError):
        lt.ngram_tree_draft(prompt, input_len, out, written, 9, g, B, 3, 1, spec, mask)


def test_the_namespace_is_layered_on_the_lookup_oracle():
    assert lt.ops.ngram_draft is lo.ops.ngram_draft and lt.ops.stop_scan is lo.ops.stop_scan
    assert not hasattr(lo.ops, "ngram_tree_draft")
