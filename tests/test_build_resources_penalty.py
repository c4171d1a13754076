"""The kernels of csrc/penalty.hip (``ls_penalize_rows``, ``ls_token_state_add``) run inside every penalised verification pass
and vanilla step: none of them may use a scratch segment or spill.  The compiler's resource report of the product build,
checked without a GPU."""
import json
import os


def _usage(src):
    from longspec_amd import build
    build.build(verbose=False)
    with open(os.path.join(build.LIBDIR, src + ".usage.json")) as f:
        return json.load(f)


def test_penalty_kernels_have_no_scratch_and_no_spills():
    u = _usage("penalty")
    want = {"penalize_rows_kernel": 2, "token_state_add_kernel": 1}          # fp16 and bf16
    for stem, count in want.items():
        names = [n for n in u if stem in n]
        assert len(names) == count, (stem, names)
        for n in names:
            assert u[n]["VGPRs Spill"] == 0 and u[n]["SGPRs Spill"] == 0 and u[n]["ScratchSize [bytes/lane]"] == 0, (n, u[n])
    assert sum(want.values()) == len(u), sorted(u)


def test_penalty_source_is_part_of_the_build():
    from longspec_amd import build
    assert "penalty.hip" in build.SOURCES
