"""The kernels of csrc/watermark.hip: ``ls_watermark_rows`` runs inside every round and vanilla step under ``watermark=`` and
``ls_watermark_score`` over whole documents; neither may use a scratch segment or spill.  The compiler's resource report of the
product build, checked without a GPU."""
import json
import os
import re


def _usage(src):
    from longspec_amd import build
    build.build(verbose=False)
    with open(os.path.join(build.LIBDIR, src + ".usage.json")) as f:
        return json.load(f)


def test_watermark_kernels_have_no_scratch_and_no_spills():
    u = _usage("watermark")
    want = {"watermark_rows_kernel": 1, "watermark_score_kernel": 1}
    for stem, count in want.items():
        names = [n for n in u if stem in n]
        assert len(names) == count, (stem, names)
        for n in names:
            assert u[n]["VGPRs Spill"] == 0 and u[n]["SGPRs Spill"] == 0 and u[n]["ScratchSize [bytes/lane]"] == 0, (n, u[n])
    assert sum(want.values()) == len(u), sorted(u)


def test_watermark_source_is_part_of_the_build_and_the_library_exports_the_operators():
    from longspec_amd import _C, build
    assert "watermark.hip" in build.SOURCES
    assert "ls_watermark_rows" in _C.SYMBOLS and len(_C.SYMBOLS["ls_watermark_rows"][1]) == 22
    assert _C.SYMBOLS["ls_watermark_rows"][1] == _C.SYMBOLS["ls_ban_rows"][1]          # the arguments of ls_ban_rows
    assert "ls_watermark_score" in _C.SYMBOLS and len(_C.SYMBOLS["ls_watermark_score"][1]) == 11


def test_the_layout_constants_agree():
    from longspec_amd import ops, watermark
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    txt = open(os.path.join(root, "include", "longspec_hip.h")).read()
    macro = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
    assert macro("LS_WATERMARK_TABLE_WORDS") == watermark.TABLE_WORDS == ops.WATERMARK_TABLE_WORDS == 8
    assert macro("LS_WATERMARK_MAX_CONTEXT") == watermark.MAX_CONTEXT == ops.WATERMARK_MAX_CONTEXT == 8
    # the kernel's own copies are tied to the header by static_asserts; its path limit is the ban's
    src = open(os.path.join(root, "longspec_amd", "csrc", "watermark.hip")).read()
    assert "static_assert(WM_WORDS == LS_WATERMARK_TABLE_WORDS" in src and "static_assert(WM_MAX_CTX == LS_WATERMARK_MAX_CONTEXT" in src
    assert "WM_MAX_EXTRA = LS_BAN_MAX_EXTRA" in src
    for name, value in (("M1", 0x9E3779B97F4A7C15), ("M2", 0xBF58476D1CE4E5B9), ("M3", 0x94D049BB133111EB)):
        assert getattr(watermark, name) == value and f"WM_{name} = {value:#018X}".replace("0X", "0x") in src
