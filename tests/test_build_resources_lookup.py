"""The kernels of csrc/lookup.hip (``ls_ngram_draft``) run in front of every round of ``lookup_generate``: neither may use a
scratch segment or spill, and the object holds exactly the kernels the source defines.  The compiler's resource report of the
product build, checked without a GPU."""
import json
import os
import re


def _usage(src):
    from longspec_amd import build
    build.build(verbose=False)
    with open(os.path.join(build.LIBDIR, src + ".usage.json")) as f:
        return json.load(f)


def test_lookup_kernels_have_no_scratch_and_no_spills():
    from longspec_amd import build
    u = _usage("lookup")
    defined = re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(os.path.join(build.CSRC, "lookup.hip")).read())
    assert sorted(defined) == ["ngram_draft_kernel", "ngram_match_kernel"]
    for stem in defined:
        names = [n for n in u if stem in n]
        assert len(names) == 1, (stem, names)
        for n in names:
            assert u[n]["VGPRs Spill"] == 0 and u[n]["SGPRs Spill"] == 0 and u[n]["ScratchSize [bytes/lane]"] == 0, (n, u[n])
    assert len(defined) == len(u), sorted(u)


def test_lookup_source_is_part_of_the_build():
    from longspec_amd import build
    assert "lookup.hip" in build.SOURCES


def test_chunk_constant_matches_the_header():
    from conftest import ROOT
    from longspec_amd import ops
    txt = open(os.path.join(ROOT, "include", "longspec_hip.h")).read()
    assert int(re.search(r"#define LS_NGRAM_CHUNK (\d+)", txt).group(1)) == ops.NGRAM_CHUNK
