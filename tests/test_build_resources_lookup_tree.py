"""The kernels of csrc/lookup_tree.hip (``ls_ngram_tree_draft``) run in front of every round of ``lookup_generate(branches=B)``:
neither may use a scratch segment or spill, and the object holds exactly the kernels the source defines.  The compiler's
resource report of the product build, checked without a GPU."""
import json
import os
import re


def _usage(src):
    from longspec_amd import build
    build.build(verbose=False)
    with open(os.path.join(build.LIBDIR, src + ".usage.json")) as f:
        return json.load(f)


def test_lookup_tree_kernels_have_no_scratch_and_no_spills():
    from longspec_amd import build
    u = _usage("lookup_tree")
    defined = re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(os.path.join(build.CSRC, "lookup_tree.hip")).read())
    assert sorted(defined) == ["ngram_tree_draft_kernel", "ngram_tree_match_kernel"]
    for stem in defined:
        names = [n for n in u if stem in n]
        assert len(names) == 1, (stem, names)
        for n in names:
            assert u[n]["VGPRs Spill"] == 0 and u[n]["SGPRs Spill"] == 0 and u[n]["ScratchSize [bytes/lane]"] == 0, (n, u[n])
    assert len(defined) == len(u), sorted(u)


def test_lookup_tree_source_is_part_of_the_build():
    from longspec_amd import build
    assert "lookup_tree.hip" in build.SOURCES
    assert os.path.join(build.CSRC, "lookup_text.h") in build.HEADERS      # both drafters are rebuilt when it changes


def test_constants_match_the_header():
    from conftest import ROOT
    from longspec_amd import lookup, ops
    txt = open(os.path.join(ROOT, "include", "longspec_hip.h")).read()
    top = int(re.search(r"#define LS_NGRAM_TOP (\d+)", txt).group(1))
    assert top == ops.NGRAM_TOP == lookup.NGRAM_TOP == 8
    assert lookup.MAX_ROWS == ops.LINEAR_MAX_ROWS and lookup.MAX_GAMMA == ops.NGRAM_MAX_GAMMA and lookup.MAX_NGRAM == ops.NGRAM_MAX_N
    import lookup_tree_oracle
    assert lookup_tree_oracle.TOP == top
