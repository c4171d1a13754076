"""The kernel of csrc/dry.hip (``ls_dry_rows``) runs twice inside every round and vanilla step under ``dry=``: it may not use a
scratch segment or spill.  The compiler's resource report of the product build, checked without a GPU."""
import json
import os
import re


def _usage(src):
    from longspec_amd import build
    build.build(verbose=False)
    with open(os.path.join(build.LIBDIR, src + ".usage.json")) as f:
        return json.load(f)


def test_dry_kernels_have_no_scratch_and_no_spills():
    u = _usage("dry")
    want = {"dry_rows_kernel": 1}                                         # one body, launched twice
    for stem, count in want.items():
        names = [n for n in u if stem in n]
        assert len(names) == count, (stem, names)
        for n in names:
            assert u[n]["VGPRs Spill"] == 0 and u[n]["SGPRs Spill"] == 0 and u[n]["ScratchSize [bytes/lane]"] == 0, (n, u[n])
    assert sum(want.values()) == len(u), sorted(u)


def test_dry_source_is_part_of_the_build_and_the_library_exports_the_operator():
    from longspec_amd import _C, build
    assert "dry.hip" in build.SOURCES
    assert "ls_dry_rows" in _C.SYMBOLS and len(_C.SYMBOLS["ls_dry_rows"][1]) == 24


def test_the_layout_constants_agree():
    from longspec_amd import dry, ops
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    txt = open(os.path.join(root, "include", "longspec_hip.h")).read()
    macro = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
    assert macro("LS_DRY_TABLE_WORDS") == dry.TABLE_WORDS == ops.DRY_TABLE_WORDS
    assert macro("LS_DRY_MAX_MATCH") == dry.MAX_MATCH == ops.DRY_MAX_MATCH == 32
    assert dry.PEN_OFF == 4 and dry.BREAK_OFF == 4 + dry.MAX_MATCH + 1 and dry.MAX_BREAKERS == 64
    # the kernel's own copy of the layout is tied to the header by a static_assert; its chunk and path limits are the ban's
    src = open(os.path.join(root, "longspec_amd", "csrc", "dry.hip")).read()
    assert "static_assert(DR_WORDS == LS_DRY_TABLE_WORDS" in src and "DR_CHUNK = LS_BAN_CHUNK" in src
    assert "DR_MAX = LS_DRY_MAX_MATCH" in src and "DR_MAX_EXTRA = LS_BAN_MAX_EXTRA" in src
