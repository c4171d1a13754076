"""The kernels of csrc/guide.hip (``ls_guide_rows`` / ``ls_guide_advance``) run inside every round and vanilla step under
``guide=``: they may not use a scratch segment or spill.  The compiler's resource report of the product build, checked without a
GPU."""
import json
import os


def _usage(src):
    from longspec_amd import build
    build.build(verbose=False)
    with open(os.path.join(build.LIBDIR, src + ".usage.json")) as f:
        return json.load(f)


def test_guide_kernels_have_no_scratch_and_no_spills():
    u = _usage("guide")
    want = {"guide_rows_kernel": 1, "guide_advance_kernel": 1}
    for stem, count in want.items():
        names = [n for n in u if stem in n]
        assert len(names) == count, (stem, names)
        for n in names:
            assert u[n]["VGPRs Spill"] == 0 and u[n]["SGPRs Spill"] == 0 and u[n]["ScratchSize [bytes/lane]"] == 0, (n, u[n])
    assert sum(want.values()) == len(u), sorted(u)


def test_guide_source_is_part_of_the_build():
    from longspec_amd import build
    assert "guide.hip" in build.SOURCES


def test_the_layout_constants_agree():
    import re
    from longspec_amd import guide, ops
    here = os.path.dirname(os.path.abspath(__file__))
    txt = open(os.path.join(os.path.dirname(here), "include", "longspec_hip.h")).read()
    macro = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
    assert macro("LS_GUIDE_HEADER_WORDS") == guide.HEADER_WORDS == ops.GUIDE_HEADER_WORDS
    assert macro("LS_GUIDE_MAX_CLASSES") == guide.MAX_CLASSES and macro("LS_GUIDE_MAX_CELLS") == guide.MAX_CELLS
    assert macro("LS_GUIDE_NO_CLASS") == guide.NO_CLASS
    assert macro("LS_GUIDE_MAX_EXTRA") == ops.GUIDE_MAX_EXTRA and macro("LS_GUIDE_SLICE") == ops.GUIDE_SLICE
    assert ops.GUIDE_SLICE % 8 == 0 and guide.MAX_CLASSES % 64 == 0
