"""The kernels of csrc/sample.hip (``ls_sample_rows``) run once per verification pass and once per vanilla step: none of them
may use a scratch segment or spill.  The compiler's resource report of the product build, checked without a GPU."""
import json
import os


def _usage(src):
    from longspec_amd import build
    build.build(verbose=False)
    with open(os.path.join(build.LIBDIR, src + ".usage.json")) as f:
        return json.load(f)


def test_sample_kernels_have_no_scratch_and_no_spills():
    u = _usage("sample")
    want = {"sample_hist_kernel": 2, "sample_key_kernel": 2, "sample_select_kernel": 1, "sample_merge_kernel": 1}   # fp16 and bf16
    for stem, count in want.items():
        names = [n for n in u if stem in n]
        assert len(names) == count, (stem, names)
        for n in names:
            assert u[n]["VGPRs Spill"] == 0 and u[n]["SGPRs Spill"] == 0 and u[n]["ScratchSize [bytes/lane]"] == 0, (n, u[n])
    assert sum(want.values()) == len(u), sorted(u)
