"""The kernels of csrc/logprob.hip (``ls_token_logprobs``, ``ls_logprob_commit``) run inside every round and vanilla step under
``logprobs=``: none of them may use a scratch segment or spill.  The compiler's resource report of the product build, checked
without a GPU."""
import json
import os


def _usage(src):
    from longspec_amd import build
    build.build(verbose=False)
    with open(os.path.join(build.LIBDIR, src + ".usage.json")) as f:
        return json.load(f)


def test_logprob_kernels_have_no_scratch_and_no_spills():
    u = _usage("logprob")
    want = {"logprob_chunk_kernel": 4, "logprob_row_kernel": 1, "logprob_commit_kernel": 1}     # (fp16, bf16) x (n == 0, n > 0)
    for stem, count in want.items():
        names = [n for n in u if stem in n]
        assert len(names) == count, (stem, names)
        for n in names:
            assert u[n]["VGPRs Spill"] == 0 and u[n]["SGPRs Spill"] == 0 and u[n]["ScratchSize [bytes/lane]"] == 0, (n, u[n])
    assert sum(want.values()) == len(u), sorted(u)


def test_logprob_source_is_part_of_the_build():
    from longspec_amd import build
    assert "logprob.hip" in build.SOURCES
