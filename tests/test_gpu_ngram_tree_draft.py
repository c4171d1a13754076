"""``ops.ngram_tree_draft`` (``ls_ngram_tree_draft``, csrc/lookup_tree.hip) against tests/lookup_tree_oracle.py, bit for bit:
``all_spec``, ``tree_mask``, ``info``, ``hist`` and ``hist_nb``; column 0 of ``all_spec`` and row 0 of the mask are never touched,
everything else is rewritten by every call.  Text lengths sit around the chunk of candidate ends."""
import numpy as np
import pytest
import torch

import lookup_tree_oracle as lt

pytestmark = pytest.mark.gpu
KEEP = -12345                        # what column 0 of all_spec and row 0 of the mask hold
JUNK = -777                          # what the rest holds before a call
SHAPES = [(1, 2), (4, 4), (8, 8), (15, 4)]           # (gamma, branches)
# seeds of the random texts, chosen with the oracle on the CPU so that the big texts fill every branch
SEEDS = {(1, 2): 1, (4, 4): 1, (8, 8): 1, (15, 4): 1}


def chunk():
    from longspec_amd import ops
    return ops.NGRAM_CHUNK


def run_both(prompt, input_len, out, written, bound, g, B, mx, mn, hist=None, hist_nb=None):
    """The kernel and the oracle on the same (CPU) inputs: asserts equality, returns (all_spec, info, nb per row, hist, hist_nb)."""
    from longspec_amd import ops
    b, F = out.shape[0], 1 + B * g
    il = torch.tensor(input_len, dtype=torch.int32)
    wr = torch.tensor(written, dtype=torch.int32)

    def fresh(dev):
        spec = torch.full((b, F), JUNK, dtype=torch.int64, device=dev)
        mask = torch.full((b, F, F), JUNK, dtype=torch.int64, device=dev)
        spec[:, 0], mask[:, 0] = KEEP, KEEP
        return spec, mask

    spec_c, mask_c = fresh("cpu")
    hist_c = torch.zeros((b, mx + 1), dtype=torch.int64) if hist is None else hist.cpu().clone()
    nb_c = torch.zeros((b, B + 1), dtype=torch.int64) if hist_nb is None else hist_nb.cpu().clone()
    before = nb_c.clone()
    info_c = lt.ngram_tree_draft(prompt, il, out, wr, bound, g, B, mx, mn, spec_c, mask_c, hist=hist_c, hist_nb=nb_c)
    spec_d, mask_d = fresh("cuda")
    hist_d = torch.zeros((b, mx + 1), dtype=torch.int64, device="cuda") if hist is None else hist
    nb_d = torch.zeros((b, B + 1), dtype=torch.int64, device="cuda") if hist_nb is None else hist_nb
    info_d = ops.ngram_tree_draft(prompt.cuda(), il.cuda(), out.cuda(), wr.cuda(), bound, g, B, mx, mn, spec_d, mask_d, hist=hist_d,
                                  hist_nb=nb_d)
    assert info_d.dtype == torch.int32 and info_d.cpu().tolist() == info_c.tolist(), (info_d.cpu().tolist(), info_c.tolist())
    assert spec_d.cpu().tolist() == spec_c.tolist()
    assert torch.equal(mask_d.cpu(), mask_c)
    assert (spec_d[:, 0] == KEEP).all() and (mask_d[:, 0] == KEEP).all() and not (spec_c[:, 1:] == JUNK).any()
    assert set(mask_c[:, 1:].flatten().tolist()) <= {0, 1}
    assert hist_d.cpu().tolist() == hist_c.tolist() and nb_d.cpu().tolist() == nb_c.tolist()
    return spec_c, info_c, (nb_c - before).argmax(dim=1).tolist(), hist_d, nb_d


def split(text, il, pad_p=0, pad_o=8, fill_p=0, fill_o=0):
    """(prompt [1, il + pad_p], input_len, out [1, w + pad_o], written) of one text: the first arguments of `run_both`."""
    L = len(text)
    prompt = torch.full((1, il + pad_p), fill_p, dtype=torch.int64)
    out = torch.full((1, L - il + pad_o), fill_o, dtype=torch.int64)
    prompt[0, :il] = torch.tensor(text[:il], dtype=torch.int64)
    out[0, :L - il] = torch.tensor(text[il:], dtype=torch.int64)
    return prompt, [il], out, [L - il]


def lengths():
    C = chunk()
    return [2, 3, 9, C - 1, C, C + 1, 2 * C + 7]


def random_cases(g, B):
    rng = np.random.default_rng(SEEDS[g, B])
    return [(rng.integers(0, 4, L).tolist(), il) for L in lengths() for il in sorted({1, L // 2, L - 1})]


@pytest.mark.parametrize("g,B", SHAPES)
@pytest.mark.parametrize("mx,mn", [(3, 1), (8, 2)])
def test_random_text_over_four_ids(g, B, mx, mn):
    C = chunk()
    cases = random_cases(g, B)
    full = crowded = 0
    for text, il in cases:
        _, _, nb, _, _ = run_both(*split(text, il, pad_p=3), len(text) + 5, g, B, mx, mn)
        full += nb[0] == B
        cands = [e for m, e in lt.candidates(text, mx, mn)]
        crowded += max((sum(c * C <= e < (c + 1) * C for e in cands) for c in range(len(text) // C + 1)), default=0) > lt.TOP
    print(f"gamma {g}, {B} branches, n-grams {mn}..{mx}: {full} of {len(cases)} texts fill every branch, {crowded} have a chunk with "
          f"more than {lt.TOP} candidates")
    assert 2 * full >= len(cases) and crowded >= 1


def planted(L, seed=0):
    """All-distinct ids up to 152 063."""
    return (152_063 - np.random.default_rng(seed).permutation(L)).tolist()


@pytest.mark.parametrize("g,B", [(4, 4), (4, 8), (4, 2), (15, 4)])
def test_ten_occurrences_across_a_chunk_border_with_four_continuations(g, B):
    C = chunk()
    L = 2 * C + 40
    text = planted(L)
    step = 3 + g + 1
    ends = [C + 1 - 4 * step + step * k for k in range(10)]            # k = 4 ends at C + 1: its three tokens straddle the border
    assert ends[0] > 16 and ends[-1] + g < L - 8 and ends[4] == C + 1
    conts = [[200_000 + 100 * c + i for i in range(g)] for c in range(4)]
    for k, e in enumerate(ends):
        text[e - 3:e] = text[L - 3:]
        text[e:e + g] = conts[k % 4]
    for il in (20, C - 1, C + 3, L - 2):                               # the prompt/output boundary on either side, and inside one
        spec, info, nb, _, _ = run_both(*split(text, il), L, g, B, 8, 1)
        # the eight most recent ends are taken (k = 9 .. 2); walking down, k = 9, 8, 7, 6 are the four new continuations
        want = [(3, ends[k]) for k in (9, 8, 7, 6)][:B]
        assert nb == [min(B, 4)] and [tuple(x) for x in info[0, :nb[0]].tolist()] == want
        slots = spec[0, 1:].view(g, B).t().tolist()
        assert slots[:nb[0]] == [conts[k % 4] for k in (9, 8, 7, 6)][:B] and all(s == slots[0] for s in slots[nb[0]:])


def test_the_ninth_candidate_is_not_looked_at():
    C = chunk()
    L = C + 300
    text = planted(L)
    ends = [C - 40 + 10 * k for k in range(9)]                         # the oldest of nine alone goes on differently
    for k, e in enumerate(ends):
        text[e - 2:e] = text[L - 2:]
        text[e] = 300_000 + (k == 0)
    assert run_both(*split(text, 50), L, 1, 4, 2, 2)[2] == [1]
    text[ends[8] - 1] = 7                                              # eight are left: the oldest is in, and new
    spec, info, nb, _, _ = run_both(*split(text, 50), L, 1, 4, 2, 2)
    assert nb == [2] and info[0].tolist() == [[2, ends[7]], [2, ends[0]], [0, -1], [0, -1]]
    assert spec[0, 1:].tolist() == [300_000, 300_001, 300_000, 300_000]


@pytest.mark.parametrize("g,B", SHAPES)
def test_periodic_all_equal_and_tiny_texts(g, B):
    C = chunk()
    for L in (7, C + 5):
        spec, info, nb, _, _ = run_both(*split(([1, 2, 3] * L)[:L], 2), L, g, B, 3, 1)
        assert nb == [1] and info[0, 0].tolist() == [3, L - 3]
        spec, info, nb, _, _ = run_both(*split([4] * L, L - 1), L, g, B, 8, 1)
        assert nb == [1] and info[0, 0].tolist() == [min(8, L - 1), L - 1] and set(spec[0, 1:].tolist()) == {4}
    text = planted(C + 9)
    spec, info, nb, _, _ = run_both(*split(text, 7), len(text), g, B, 3, 1)      # all distinct: no candidate
    assert nb == [0] and info[0].tolist() == [[0, -1]] * B and set(spec[0, 1:].tolist()) == {text[-1]}
    prompt, il, out, wr = split([9, 5], 1)
    assert run_both(prompt, il, out, [0], 4, g, B, 3, 1)[2] == [0]               # L = 1: nothing is written yet
    assert run_both(prompt, [0], out, [0], 4, g, B, 3, 1)[0][0, 1:].tolist() == [0] * (B * g)   # L = 0


def test_batch_rows_padded_prompts_and_strided_output():
    C = chunk()
    rng = np.random.default_rng(3)
    g, B = 4, 4
    Ls, ils = [C + 30, 40, 2 * C + 1], [C - 5, 11, 300]
    P, W = max(ils) + 16, max(L - il for L, il in zip(Ls, ils)) + 32
    wide = torch.zeros((3, W + 24), dtype=torch.int64)
    out = wide[:, 8:8 + W]                                              # a column slice of a wider buffer: strided rows
    prompt = torch.zeros((3, P), dtype=torch.int64)
    for z, (L, il) in enumerate(zip(Ls, ils)):
        text = rng.integers(0, 6, L).tolist()
        prompt[z, :il] = torch.tensor(text[:il])
        out[z, :L - il] = torch.tensor(text[il:])
        decoy = torch.tensor(text[-8:] + [151_999])                     # the suffix, then a marker: longer than any true match
        prompt[z, il + 2:il + 11] = decoy
        out[z, L - il + 3:L - il + 12] = decoy
        wide[z, :8] = decoy[1:]
    wr = [L - il for L, il in zip(Ls, ils)]
    spec, info, nb, _, _ = run_both(prompt, ils, out, wr, max(Ls), g, B, 8, 1)
    assert 151_999 not in spec.flatten().tolist() and min(nb) >= 2
    from longspec_amd import ops
    wide_d = wide.cuda()
    out_d = wide_d[:, 8:8 + W]
    F = 1 + g * B
    spec_d = torch.full((3, F), KEEP, dtype=torch.int64, device="cuda")
    mask_d = torch.full((3, F, F), KEEP, dtype=torch.int64, device="cuda")
    info_d = ops.ngram_tree_draft(prompt.cuda(), torch.tensor(ils, dtype=torch.int32).cuda(), out_d,
                                  torch.tensor(wr, dtype=torch.int32).cuda(), max(Ls), g, B, 8, 1, spec_d, mask_d)
    assert not out_d.is_contiguous() and info_d.cpu().tolist() == info.tolist() and spec_d[:, 1:].cpu().tolist() == spec[:, 1:].tolist()
    for z in range(3):                                                  # each row alone gives the same bits
        sz, iz, _, _, _ = run_both(prompt[z:z + 1], ils[z:z + 1], out[z:z + 1].contiguous(), wr[z:z + 1], Ls[z], g, B, 8, 1)
        assert sz[0].tolist() == spec[z].tolist() and iz[0].tolist() == info[z].tolist()


def test_histograms_accumulate_over_calls():
    text = planted(60)
    text[59] = text[10]
    text[40] = text[10]                                                 # two ends, two continuations
    hist = torch.zeros((1, 4), dtype=torch.int64, device="cuda")
    hist_nb = torch.zeros((1, 4), dtype=torch.int64, device="cuda")
    for k in range(2):
        _, _, _, hist, hist_nb = run_both(*split(text, 5), 60, 2, 3, 3, 1, hist=hist, hist_nb=hist_nb)
    assert hist.cpu().tolist() == [[0, 2, 0, 0]] and hist_nb.cpu().tolist() == [[0, 0, 2, 0]]
    _, _, _, hist, hist_nb = run_both(*split(planted(60), 5), 60, 2, 3, 3, 1, hist=hist, hist_nb=hist_nb)
    assert hist.cpu().tolist() == [[1, 2, 0, 0]] and hist_nb.cpu().tolist() == [[1, 0, 2, 0]]


@pytest.mark.parametrize("g,B", SHAPES)
def test_slot_0_is_what_ngram_draft_drafts(g, B):
    from longspec_amd import ops
    for text, il in random_cases(g, B):
        prompt, ilv, out, wr = split(text, il, pad_p=2)
        F = 1 + g * B
        spec = torch.zeros((1, F), dtype=torch.int64, device="cuda")
        mask = torch.zeros((1, F, F), dtype=torch.int64, device="cuda")
        ilt = torch.tensor(ilv, dtype=torch.int32).cuda()
        info = ops.ngram_tree_draft(prompt.cuda(), ilt, out.cuda(), torch.tensor(wr, dtype=torch.int32).cuda(), len(text), g, B, 3, 1,
                                    spec, mask)
        chain = torch.zeros((1, g + 1), dtype=torch.int64, device="cuda")
        cl = torch.tensor([len(text) - 1], dtype=torch.int32).cuda()     # the chain's w = cache_lens - input_len + 1
        cinfo = ops.ngram_draft(prompt.cuda(), ilt, out.cuda(), cl, len(text), g, 3, 1, chain)
        assert spec[0, 1:].view(g, B)[:, 0].tolist() == chain[0, 1:].tolist() and info[0, 0].tolist() == cinfo[0].tolist()


def test_a_captured_call_replays_on_the_text_as_it_stands():
    from longspec_amd import ops
    C = chunk()
    rng = np.random.default_rng(17)
    il, W, g, B, mx, mn = C - 20, 96, 7, 4, 3, 1
    F = 1 + g * B
    full = rng.integers(0, 5, il + W).tolist()
    prompt = torch.tensor([full[:il]], dtype=torch.int64).cuda()
    out = torch.zeros((1, W), dtype=torch.int64, device="cuda")
    ilt = torch.tensor([il], dtype=torch.int32).cuda()
    wr = torch.tensor([1], dtype=torch.int32).cuda()
    out[0, 0] = full[il]
    spec = torch.full((1, F), KEEP, dtype=torch.int64, device="cuda")
    mask = torch.full((1, F, F), KEEP, dtype=torch.int64, device="cuda")
    hist = torch.zeros((1, mx + 1), dtype=torch.int64, device="cuda")
    hist_nb = torch.zeros((1, B + 1), dtype=torch.int64, device="cuda")
    info = torch.zeros((1, B, 2), dtype=torch.int32, device="cuda")
    bound = il + W

    def call():
        ops.ngram_tree_draft(prompt, ilt, out, wr, bound, g, B, mx, mn, spec, mask, info=info, hist=hist, hist_nb=hist_nb)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):                                     # warm-up on the capture stream: its workspace
        call()
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        call()
    keep = {t.data_ptr() for t in ops.workspace_tensors()}
    assert {b.data_ptr() for b in ops._ngram_tree_ws._buf.values()} <= keep and ops._ngram_tree_ws._buf
    want_hist, want_nb = [0] * (mx + 1), [0] * (B + 1)
    slots, ne, nb = lt.tree_draft(full[:il + 1], g, B, mx, mn)
    want_hist[ne[0][0]] += 1
    want_nb[nb] += 1
    w = 1
    for add in (30, 40):                                                # the text grows across the chunk boundary
        out[0, w:w + add] = torch.tensor(full[il + w:il + w + add], device="cuda")
        out[0, w + add:w + add + 3] = 151_999                           # stale ids behind w
        w += add
        wr.fill_(w)
        mask[:, 1:] = JUNK                                              # what tree_commit does to the mask, and worse
        spec[:, 1:] = JUNK
        graph.replay()
        slots, ne, nb = lt.tree_draft(full[:il + w], g, B, mx, mn)
        rows_spec, rows_mask = lt.tree_layout(slots, g, B)
        want_hist[ne[0][0]] += 1
        want_nb[nb] += 1
        assert info.cpu().tolist() == [[list(x) for x in ne]] and spec.cpu().tolist() == [[KEEP] + rows_spec]
        assert mask[0, 1:].cpu().tolist() == rows_mask and (mask[0, 0] == KEEP).all()
        assert hist.cpu().tolist() == [want_hist] and hist_nb.cpu().tolist() == [want_nb]
