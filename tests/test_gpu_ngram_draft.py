"""``ops.ngram_draft`` (``ls_ngram_draft``, csrc/lookup.hip) against tests/lookup_oracle.py, bit for bit: ``spec_buffer``,
``info`` and ``hist``; column 0 of ``spec_buffer`` is never touched.  Text lengths sit around the chunk of candidate ends."""
import numpy as np
import pytest
import torch

import lookup_oracle as lo

pytestmark = pytest.mark.gpu
MARK = 151_999                       # the id decoys are followed by: it must never be drafted
KEEP = -12345                        # what column 0 of spec_buffer holds


def chunk():
    from longspec_amd import ops
    return ops.NGRAM_CHUNK


def run_both(prompt, input_len, out, cache_lens, bound, g, mx, mn, hist=None):
    """The kernel and the oracle on the same (CPU) inputs: asserts equality, returns (draft rows, info, hist)."""
    from longspec_amd import ops
    b = out.shape[0]
    il = torch.tensor(input_len, dtype=torch.int32)
    cl = torch.tensor(cache_lens, dtype=torch.int32)
    spec_c = torch.full((b, g + 1), KEEP, dtype=torch.int64)
    hist_c = torch.zeros((b, mx + 1), dtype=torch.int64) if hist is None else hist.cpu().clone()
    info_c = lo.ngram_draft(prompt, il, out, cl, bound, g, mx, mn, spec_c, hist=hist_c)
    spec_d = torch.full((b, g + 1), KEEP, dtype=torch.int64, device="cuda")
    hist_d = torch.zeros((b, mx + 1), dtype=torch.int64, device="cuda") if hist is None else hist
    out_d = out.cuda() if not out.is_cuda else out
    info_d = ops.ngram_draft(prompt.cuda(), il.cuda(), out_d, cl.cuda(), bound, g, mx, mn, spec_d, hist=hist_d)
    assert info_d.dtype == torch.int32 and info_d.cpu().tolist() == info_c.tolist(), (info_d.cpu().tolist(), info_c.tolist())
    assert spec_d.cpu().tolist() == spec_c.tolist()
    assert (spec_d[:, 0] == KEEP).all()
    assert hist_d.cpu().tolist() == hist_c.tolist()
    return spec_c[:, 1:], info_c, hist_d


def split(text, il, pad_p=0, pad_o=8, fill_p=0, fill_o=0):
    """(prompt [1, il + pad_p], input_len, out [1, w + pad_o], cache_lens) of one text: the first arguments of `run_both`."""
    L = len(text)
    prompt = torch.full((1, il + pad_p), fill_p, dtype=torch.int64)
    out = torch.full((1, L - il + pad_o), fill_o, dtype=torch.int64)
    prompt[0, :il] = torch.tensor(text[:il], dtype=torch.int64)
    out[0, :L - il] = torch.tensor(text[il:], dtype=torch.int64)
    return prompt, [il], out, [L - 1]


def lengths():
    C = chunk()
    return [2, 3, 9, C - 1, C, C + 1, 2 * C + 7]


@pytest.mark.parametrize("g,mx,mn", [(1, 1, 1), (4, 3, 1), (7, 2, 2), (15, 8, 1), (15, 8, 8)])
def test_random_text_over_four_ids(g, mx, mn):
    rng = np.random.default_rng(g * 100 + mx * 10 + mn)
    matched = 0
    for L in lengths():
        for il in sorted({1, L // 2, L - 1}):
            text = rng.integers(0, 4, L).tolist()
            _, info, _ = run_both(*split(text, il, pad_p=3), L + 5, g, mx, mn)
            matched += int(info[0, 0] > 0)
    assert matched >= (10 if mn < 8 else 0)


def planted(L, seed=0):
    """All-distinct ids up to 152 063."""
    return (152_063 - np.random.default_rng(seed).permutation(L)).tolist()


def test_the_winner_straddles_the_prompt_output_boundary_and_a_chunk_boundary():
    C = chunk()
    L = 2 * C + 40
    # the occurrence T[at : at + 4]: two tokens in the prompt and two in the output; its end in chunk 1 and its front in chunk
    # 0; the same at the second boundary, in the output
    for at, il in ((300, 302), (C - 2, 50), (2 * C - 1, C + 7)):
        text = planted(L, at)
        text[L - 4:] = text[at:at + 4]
        d, info, _ = run_both(*split(text, il), L, 6, 8, 1)
        assert info.tolist() == [[4, at + 4]] and d[0].tolist() == text[at + 4:at + 10]
        assert run_both(*split(text, il), L, 6, 3, 2)[1].tolist() == [[3, at + 4]]


@pytest.mark.parametrize("back", [1, 2])
def test_an_occurrence_that_ends_at_the_end_of_the_text_wraps(back):
    C = chunk()
    for L in (5, C + 3):
        text = planted(L)
        text[L - back:] = text[L - 2 * back:L - back]                   # period `back`: e = L - back
        d, info, _ = run_both(*split(text, 2), L, 15, 8, 1)
        assert info.tolist() == [[back, L - back]]
        assert d[0].tolist() == (text[L - back:] * 15)[:15]


def test_a_longer_older_match_beats_a_shorter_newer_one():
    C = chunk()
    L = C + 200
    text = planted(L)
    text[L - 3:] = text[20:23]                                          # three tokens match at e = 23
    text[C + 50] = text[L - 1]                                          # one token at e = C + 51
    assert run_both(*split(text, 100), L, 4, 3, 1)[1].tolist() == [[3, 23]]
    assert run_both(*split(text, 100), L, 4, 1, 1)[1].tolist() == [[1, C + 51]]


def test_nothing_of_min_ngram_and_all_distinct():
    L = chunk() + 9
    text = planted(L)
    d, info, _ = run_both(*split(text, 7), L, 5, 3, 1)
    assert info.tolist() == [[0, -1]] and d[0].tolist() == [text[-1]] * 5
    text[40] = text[L - 1]                                              # a one-token match only
    assert run_both(*split(text, 7), L, 5, 3, 2)[1].tolist() == [[0, -1]]
    assert run_both(*split(text, 7), L, 5, 3, 1)[1].tolist() == [[1, 41]]


def test_ids_that_differ_above_bit_31_do_not_match():
    L = 70
    text = planted(L)
    text[10] = text[L - 1] + (1 << 32)
    text[30] = text[L - 1] + (1 << 40)
    assert run_both(*split(text, 5), L, 3, 2, 1)[1].tolist() == [[0, -1]]
    text[50] = text[L - 1]
    text[49], text[L - 2] = 7, 7 + (1 << 33)                           # the second token differs above bit 31 only
    assert run_both(*split(text, 5), L, 3, 2, 1)[1].tolist() == [[1, 51]]


def test_batch_rows_strided_output_and_decoys():
    C = chunk()
    rng = np.random.default_rng(3)
    Ls, ils = [C + 30, 40, 2 * C + 1], [C - 5, 11, 300]
    P, W = max(ils) + 16, max(L - il for L, il in zip(Ls, ils)) + 32
    wide = torch.zeros((3, W + 24), dtype=torch.int64)
    out = wide[:, 8:8 + W]                                              # a column slice of a wider buffer: strided rows
    prompt = torch.zeros((3, P), dtype=torch.int64)
    texts = []
    for z, (L, il) in enumerate(zip(Ls, ils)):
        text = rng.integers(0, 6, L).tolist()
        texts.append(text)
        prompt[z, :il] = torch.tensor(text[:il])
        out[z, :L - il] = torch.tensor(text[il:])
        decoy = torch.tensor(text[-8:] + [MARK])                        # the suffix, then the marker: longer than any true match
        prompt[z, il + 2:il + 11] = decoy
        out[z, L - il + 3:L - il + 12] = decoy
        wide[z, :8] = decoy[1:]
    assert not out.is_contiguous()
    cl = [L - 1 for L in Ls]
    d, info, _ = run_both(prompt, ils, out, cl, max(Ls), 15, 8, 1)
    assert MARK not in d.flatten().tolist() and (info[:, 0] > 0).all()
    from longspec_amd import ops
    wide_d = wide.cuda()
    out_d = wide_d[:, 8:8 + W]
    spec = torch.full((3, 16), KEEP, dtype=torch.int64, device="cuda")
    info_d = ops.ngram_draft(prompt.cuda(), torch.tensor(ils, dtype=torch.int32).cuda(), out_d,
                             torch.tensor(cl, dtype=torch.int32).cuda(), max(Ls), 15, 8, 1, spec)
    assert not out_d.is_contiguous() and info_d.cpu().tolist() == info.tolist() and spec[:, 1:].cpu().tolist() == d.tolist()
    for z in range(3):                                                  # each row alone gives the same bits
        dz, iz, _ = run_both(prompt[z:z + 1], ils[z:z + 1], out[z:z + 1].contiguous(), cl[z:z + 1], Ls[z], 15, 8, 1)
        assert dz[0].tolist() == d[z].tolist() and iz[0].tolist() == info[z].tolist()


def test_a_128k_text_with_one_planted_8_gram():
    L, il = 131_072 + 77, 131_072
    rng = np.random.default_rng(11)
    text = rng.integers(0, 50_000, L)
    text[L - 8:] = 60_000 + np.arange(8)                                # ids no other position holds
    text[1000:1008] = text[L - 8:]
    d, info, hist = run_both(*split(text.tolist(), il), L + 4096, 15, 8, 1)        # the host bound 4096 above L
    assert info.tolist() == [[8, 1008]] and d[0].tolist() == text[1008:1023].tolist()
    assert hist.cpu().tolist() == [[0] * 8 + [1]]


def test_hist_accumulates_over_calls():
    text = planted(50)
    text[49] = text[10]
    hist = torch.zeros((1, 4), dtype=torch.int64, device="cuda")
    for k in range(3):
        _, _, hist = run_both(*split(text, 5), 50, 2, 3, 1, hist=hist)
    assert hist.cpu().tolist() == [[0, 3, 0, 0]]
    _, _, hist = run_both(*split(planted(50), 5), 50, 2, 3, 1, hist=hist)
    assert hist.cpu().tolist() == [[1, 3, 0, 0]]


def test_a_captured_call_replays_on_the_text_as_it_stands():
    from longspec_amd import ops
    C = chunk()
    rng = np.random.default_rng(17)
    il, W, g, mx, mn = C - 20, 96, 7, 3, 1
    full = rng.integers(0, 5, il + W).tolist()
    prompt = torch.tensor([full[:il]], dtype=torch.int64).cuda()
    out = torch.zeros((1, W), dtype=torch.int64, device="cuda")
    ilt = torch.tensor([il], dtype=torch.int32).cuda()
    cl = torch.tensor([il], dtype=torch.int32).cuda()                   # w = 1
    out[0, 0] = full[il]
    spec = torch.full((1, g + 1), KEEP, dtype=torch.int64, device="cuda")
    hist = torch.zeros((1, mx + 1), dtype=torch.int64, device="cuda")
    info = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    bound = il + W
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):                                     # warm-up on the capture stream: its workspace
        ops.ngram_draft(prompt, ilt, out, cl, bound, g, mx, mn, spec, info=info, hist=hist)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        ops.ngram_draft(prompt, ilt, out, cl, bound, g, mx, mn, spec, info=info, hist=hist)
    want_hist = [0] * (mx + 1)
    want_hist[lo.match(full[:il + 1], mx, mn)[0]] += 1
    w = 1
    for add in (5, 30, 40):                                             # the text grows across the chunk boundary
        out[0, w:w + add] = torch.tensor(full[il + w:il + w + add], device="cuda")
        out[0, w + add:w + add + 3] = MARK                              # stale ids behind w
        w += add
        cl.fill_(il + w - 1)
        graph.replay()
        d, n, e = lo.draft(full[:il + w], g, mx, mn)
        want_hist[n] += 1
        assert info.cpu().tolist() == [[n, e]] and spec.cpu().tolist() == [[KEEP] + d]
        assert hist.cpu().tolist() == [want_hist]
