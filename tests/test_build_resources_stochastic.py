"""The kernels added for the graph-replayed temperature > 0 round (the log-prob store of topk.hip, the stochastic commit of
tree.hip) must not use a scratch segment: the compiler's resource report of the product build, checked without a GPU."""
import json
import os


def _usage(src):
    from longspec_amd import build
    build.build(verbose=False)
    with open(os.path.join(build.LIBDIR, src + ".usage.json")) as f:
        return json.load(f)


def _clean(u, n):
    assert u[n]["VGPRs Spill"] == 0 and u[n]["SGPRs Spill"] == 0 and u[n]["ScratchSize [bytes/lane]"] == 0, (n, u[n])


def test_logp_store_kernels_have_no_scratch():
    u = _usage("topk")
    store = [n for n in u if "logp_store_kernel" in n]
    assert len(store) == 2, store                          # fp16 and bf16
    for n in store:
        _clean(u, n)
    # the chunk and merge kernels share their row statistics with it: they must not have started to spill either
    shared = [n for n in u if "topk_chunk_kernel" in n or "topk_merge_kernel" in n]
    assert len(shared) == 2 + 4, shared
    for n in shared:
        _clean(u, n)


def test_stochastic_commit_kernel_has_no_scratch():
    u = _usage("tree")
    commit = [n for n in u if "tree_commit_stochastic_kernel" in n]
    assert len(commit) == 1, commit
    _clean(u, commit[0])
