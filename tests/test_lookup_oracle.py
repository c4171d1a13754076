"""Hand-written cases that pin tests/lookup_oracle.py, the plain-Python definition of the prompt-lookup drafter
(``longspec_amd/lookup.py``): the expectations below were worked out by hand from the definition, not from the code."""
import pytest
import torch

import lookup_oracle as lo


def test_longest_beats_recent():
    #       0  1  2  3  4  5  6  7  8  9 10
    text = [1, 2, 3, 9, 7, 3, 8, 6, 1, 2, 3]
    # suffix (1, 2, 3): the end e = 3 matches three tokens, the later e = 6 only one
    assert lo.draft(text, 4, 3, 1) == ([9, 7, 3, 8], 3, 3)
    # with max_ngram = 1 both match one token and the most recent wins
    assert lo.draft(text, 4, 1, 1) == ([8, 6, 1, 2], 1, 6)


def test_most_recent_among_equals():
    #       0  1  2  3  4  5  6  7  8
    text = [5, 6, 1, 5, 6, 2, 4, 5, 6]
    assert lo.draft(text, 3, 2, 1) == ([2, 4, 5], 2, 5)
    assert lo.draft(text, 3, 8, 2) == ([2, 4, 5], 2, 5)


def test_overlap_with_the_suffix():
    #       0  1  2  3  4
    text = [7, 3, 3, 3, 3]
    # e = 4: T[1:4] == T[2:5], the occurrence overlaps the suffix; the draft wraps with period 1
    assert lo.draft(text, 5, 3, 1) == ([3, 3, 3, 3, 3], 3, 4)
    # e = 4 is limited by max_ngram only: with 8 it matches T[1:4] (three 3s; T[0] = 7 stops it)
    assert lo.match(text, 8, 1) == (3, 4)


def test_period_one_and_two_wrap_to_full_depth():
    assert lo.draft([4, 9, 9], 15, 3, 1) == ([9] * 15, 1, 2)                       # e = L - 1
    text = [8, 1, 2, 1, 2]                                                          # e = L - 2 = 3: T[1:3] == T[3:5]
    d, n, e = lo.draft(text, 15, 2, 1)
    assert (n, e) == (2, 3) and d == [1, 2] * 7 + [1]
    # a longer context prefers the same end here: (1, 2, 1, 2) does not occur earlier, (2, 1, 2)... T[0:3] = 8, 1, 2 no
    assert lo.match(text, 8, 1) == (2, 3)


def test_only_matches_shorter_than_min_ngram():
    text = [1, 2, 5, 3, 2]                                                          # one earlier 2, preceded by 1 != 3
    assert lo.draft(text, 4, 3, 1) == ([5, 3, 2, 5], 1, 2)
    assert lo.draft(text, 4, 3, 2) == ([2, 2, 2, 2], 0, -1)


def test_all_distinct_and_the_shortest_text():
    assert lo.draft(list(range(10, 30)), 3, 3, 1) == ([29, 29, 29], 0, -1)
    assert lo.draft([6, 6], 2, 8, 1) == ([6, 6], 1, 1)                              # L = 2: the one end, one token of context
    assert lo.draft([6, 7], 2, 8, 1) == ([7, 7], 0, -1)


def test_ids_are_compared_in_64_bits():
    a, b = 5, 5 + (1 << 32)
    assert lo.draft([a, 1, b], 1, 1, 1) == ([b], 0, -1)
    assert lo.draft([b, 1, b], 1, 1, 1) == ([1], 1, 1)


def test_the_operator_reads_only_the_text_and_keeps_column_0():
    prompt = torch.tensor([[1, 2, 3, 77, 77], [4, 4, 4, 4, 4]])                     # row 0: two columns of padding
    out = torch.tensor([[9, 1, 2, 3, 55, 0], [4, 4, 0, 0, 0, 0]])                   # row 0: stale ids behind w = 4
    input_len = torch.tensor([3, 5], dtype=torch.int32)
    cache_lens = torch.tensor([6, 5], dtype=torch.int32)                            # w = 4 and 1
    spec = torch.full((2, 4), -7)
    hist = torch.zeros((2, 4), dtype=torch.int64)
    info = lo.ngram_draft(prompt, input_len, out, cache_lens, 16, 3, 3, 1, spec, hist=hist)
    # row 0: T = 1 2 3 9 1 2 3, the suffix (1, 2, 3) ends at e = 3 -> 9 1 2; row 1: T = 4 4 4 4 4 4, e = 5, period 1
    assert spec.tolist() == [[-7, 9, 1, 2], [-7, 4, 4, 4]]
    assert info.tolist() == [[3, 3], [3, 5]] and hist.tolist() == [[0, 0, 0, 1], [0, 0, 0, 1]]
    with pytest.raises(AssertionError):
        lo.ngram_draft(prompt, input_len, out, cache_lens, 6, 3, 3, 1, spec)
