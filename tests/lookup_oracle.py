"""Oracle of ``ops.ngram_draft`` (``ls_ngram_draft``): the definition of ``longspec_amd/lookup.py`` in plain Python, and an
operator namespace layered on ``stop_oracle.ops`` that lets ``lookup_generate`` run on the CPU.  Lives under tests/: the product
never imports it."""
import stop_oracle


def match(text, max_ngram, min_ngram):
    """(n, e) of the winner over ``text`` (a list of ints): the largest m(e), then the largest e; (0, -1) without a candidate."""
    L = len(text)
    best = (0, -1)
    for e in range(1, L):
        if text[e - 1] != text[L - 1]:
            continue
        m = max(k for k in range(1, min(max_ngram, e) + 1) if text[e - k:e] == text[L - k:L])
        if m >= min_ngram and (m, e) > best:
            best = (m, e)
    return best


def draft(text, gamma, max_ngram, min_ngram):
    """(d [gamma], n, e)."""
    L = len(text)
    n, e = match(text, max_ngram, min_ngram)
    if n == 0:
        return [text[L - 1]] * gamma, 0, -1
    return [text[e + i % (L - e)] for i in range(gamma)], n, e


def text_of(prompt_ids, input_len, output_ids, cache_lens, z):
    il = int(input_len[z])
    w = int(cache_lens[z]) - il + 1
    return prompt_ids[z, :il].tolist() + output_ids[z, :w].tolist()


def ngram_draft(prompt_ids, input_len, output_ids, cache_lens, len_bound, gamma, max_ngram, min_ngram, spec_buffer, info=None,
                hist=None):
    """``longspec_amd.ops.ngram_draft`` on CPU tensors (in place, exact; ``len_bound`` must bound every text)."""
    import torch
    b = output_ids.shape[0]
    if info is None:
        info = torch.empty((b, 2), dtype=torch.int32)
    for z in range(b):
        text = text_of(prompt_ids, input_len, output_ids, cache_lens, z)
        assert len(text) <= len_bound, "the host's bound is no bound"
        d, n, e = draft(text, gamma, max_ngram, min_ngram)
        spec_buffer[z, 1:] = torch.tensor(d, dtype=torch.int64)
        info[z, 0], info[z, 1] = n, e
        if hist is not None:
            hist[z, n] += 1
    return info


class Ops:
    """``stop_oracle.ops`` plus the drafter: the operator namespace of the lookup host-logic tests."""

    def __getattr__(self, name):
        return getattr(stop_oracle.ops, name)

    ngram_draft = staticmethod(ngram_draft)


ops = Ops()
