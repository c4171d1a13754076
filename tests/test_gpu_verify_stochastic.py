"""``ls_tree_verify_stochastic`` called directly (``ops.tree_verify_stochastic``), one launch per case, against the word-stream
oracle (tests/stochastic_oracle.py): vocabularies beyond one stride of the 1024 threads, ragged tails, production
vocabularies, batch rows in one launch, strided views and Fs < F, every child count's word rejection, the depth limit, the
word budget and the all-zero residual.  ``acc_ids``, ``acc_num`` and ``words_used`` are compared EXACTLY: every case of the table
meets the margin condition asserted in tests/test_stochastic_oracle.py, so it has one correct answer."""
import random

import numpy as np
import pytest
import torch

import stochastic_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from longspec_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def launch(ops, x, rows=None, n_words=None, max_acc=None):
    """One launch on (rows of) the inputs of ``stochastic_oracle.build`` -> (acc_ids, acc_num, words_used) on the CPU."""
    spec, mask, logits, logp, T, words, noise = so.to_device(x, DEV, rows, n_words)
    ids, num, used = ops.tree_verify_stochastic(spec, mask, logits, logp, T, words, noise, max_acc or x["max_acc"])
    return ids.cpu(), num.cpu(), used.cpu()


def check_rows(got, want, what):
    ids, num, used = got
    for z, (w_ids, w_num, w_used, _) in enumerate(want):
        assert int(used[z]) == w_used, f"{what} row {z}: words_used {int(used[z])}, the oracle consumed {w_used}"
        assert int(num[z]) == w_num, f"{what} row {z}: acc_num {int(num[z])}, oracle {w_num}"
        assert torch.equal(ids[z], w_ids), f"{what} row {z}: acc_ids {ids[z].tolist()}, oracle {w_ids.tolist()}"


@pytest.mark.parametrize("c", so.CASES, ids=lambda c: c["name"])
def test_case_matches_the_oracle(ops, c):
    x = so.build(c)
    want = so.expected(c)
    got = launch(ops, x)
    check_rows(got, want, c["name"])
    if x["b"] > 1:                                  # a row of a batched launch == the same row launched alone
        for z in range(x["b"]):
            one = launch(ops, x, rows=slice(z, z + 1))
            check_rows(one, want[z:z + 1], f"{c['name']} alone")
            assert torch.equal(one[0][0], got[0][z]) and int(one[1][0]) == int(got[1][z]) and int(one[2][0]) == int(got[2][z])


def test_depth_limit(ops):
    """13 accepted nodes + the root + the final draw fill max_acc = 15, the largest the entry point takes."""
    from longspec_amd import _C
    c = so.BY_NAME["chain13"]
    x = so.build(c)
    assert x["max_acc"] == 15
    ids, num, used = launch(ops, x)
    (w_ids, w_num, _, _), = so.expected(c)
    assert int(num[0]) == 15 and torch.equal(ids[0], w_ids) and torch.equal(ids[0, :14], x["spec"][0])
    with pytest.raises(_C.LongSpecHipError, match=r"code -1.*max_acc=16"):      # LS_ERR_INVALID_ARG, before any launch
        launch(ops, x, max_acc=16)


def test_vocabulary_smaller_than_the_tree_is_rejected(ops):
    """The acceptance ratio reads vocabulary index s = the child's node index: V < F is LS_ERR_INVALID_ARG (no launch)."""
    from longspec_amd import _C
    Fn, V = 69, 64
    x = so.build(so.BY_NAME["sweep_V1023_f16_T1.0"])
    spec, mask = x["spec"].to(DEV), x["mask"].to(DEV)
    assert spec.shape[1] == Fn
    logits = torch.zeros((1, Fn, V), dtype=torch.float16, device=DEV)
    logp = torch.zeros((1, Fn, V), dtype=torch.float32, device=DEV)
    words = torch.zeros((1, 16), dtype=torch.int32, device=DEV)
    noise = torch.ones((1, V), dtype=torch.float16, device=DEV)
    with pytest.raises(_C.LongSpecHipError, match=r"code -1.*V=64.*F=69"):
        ops.tree_verify_stochastic(spec, mask, logits, logp, 1.0, words, noise, x["max_acc"])


def test_word_budget(ops):
    """n_words == what the walk consumes: exact, and reported; one word fewer: words_used = -1."""
    for name in ("reject_all_5_2", "sweep_V1025_f16_T1.3", "chain13"):
        c = so.BY_NAME[name]
        x = so.build(c)
        want = so.expected(c)
        u = want[0][2]
        assert u >= 4
        check_rows(launch(ops, x, n_words=u), want, f"{name} with n_words = {u}")
        assert int(launch(ops, x, n_words=u - 1)[2][0]) == -1
    # a 3-child root: getrandbits(2) = 3 is redrawn, so the first draw takes 3 words or 4
    c = so.BY_NAME["accept_all_3"]
    base = so.build(c)
    args = (base["spec"][0], base["mask"][0], base["logits"][0], base["logp"][0], base["T"])
    for words, u in (([0x40000000, 0x12345678, 0x9ABCDEF0, 0], 3), ([0xC0000000, 0x40000000, 0x12345678, 0x9ABCDEF0], 4)):
        x = dict(base, words=np.array([words], dtype=np.uint32))
        want = so.walk(*args, words[:u], base["noise"][0])
        assert want[2] == u and want[1] == 3
        check_rows(launch(ops, x, n_words=u), [want], f"3-child root, n_words = {u}")
        check_rows(launch(ops, x, n_words=4), [want], "3-child root, n_words = 4")
        if u == 4:
            with pytest.raises(so.WordsExhausted):
                so.walk(*args, words[:3], base["noise"][0])
            assert int(launch(ops, x, n_words=3)[2][0]) == -1


def test_wrapper_raises_and_keeps_pythons_generator(ops, monkeypatch):
    """ops.verify_stochastic with too few pre-drawn words: RuntimeError, and ``random`` is where it was before the call."""
    monkeypatch.setattr(ops, "MT_WORDS", 3)
    c = so.BY_NAME["reject_all_3"]                  # the first child is rejected: more than one draw is needed
    x = so.build(c)
    assert so.expected(c)[0][2] > 3
    spec, mask, logits, logp, T, _, _ = so.to_device(x, DEV)
    random.seed(4321)
    state = random.getstate()
    with pytest.raises(RuntimeError, match="exhausted"):
        ops.verify_stochastic(spec, mask, logits, logp, T)
    assert random.getstate() == state


def test_zero_residual(ops):
    """One-hot target and draft at the same index: every child is rejected with ratio 0, the residual is all zero and is
    left un-normalised.  The reference's torch.multinomial raises on that row; the device returns some valid index."""
    x = so.zero_residual_inputs()
    with pytest.raises(so.ZeroDistribution) as e:
        so.walk(x["spec"][0], x["mask"][0], x["logits"][0], x["logp"][0], x["T"], x["words"][0], x["noise"][0])
    ids, num, used = launch(ops, x)
    assert int(num[0]) == 2 and int(ids[0, 0]) == int(x["spec"][0, 0])
    assert 0 <= int(ids[0, 1]) < x["logits"].shape[-1] and int(ids[0, 2]) == 0
    assert int(used[0]) == e.value.words_used
