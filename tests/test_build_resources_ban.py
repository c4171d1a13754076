"""The kernel of csrc/ban.hip (``ls_ban_rows``) runs inside every round and vanilla step under ``ban=``: it may not use a scratch
segment or spill.  The compiler's resource report of the product build, checked without a GPU."""
import json
import os


def _usage(src):
    from longspec_amd import build
    build.build(verbose=False)
    with open(os.path.join(build.LIBDIR, src + ".usage.json")) as f:
        return json.load(f)


def test_ban_kernels_have_no_scratch_and_no_spills():
    u = _usage("ban")
    want = {"ban_rows_kernel": 1}
    for stem, count in want.items():
        names = [n for n in u if stem in n]
        assert len(names) == count, (stem, names)
        for n in names:
            assert u[n]["VGPRs Spill"] == 0 and u[n]["SGPRs Spill"] == 0 and u[n]["ScratchSize [bytes/lane]"] == 0, (n, u[n])
    assert sum(want.values()) == len(u), sorted(u)


def test_ban_source_is_part_of_the_build():
    from longspec_amd import build
    assert "ban.hip" in build.SOURCES


def test_the_layout_constants_agree():
    import re
    from longspec_amd import ban, ops
    here = os.path.dirname(os.path.abspath(__file__))
    txt = open(os.path.join(os.path.dirname(here), "include", "longspec_hip.h")).read()
    macro = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
    assert macro("LS_BAN_TABLE_WORDS") == ban.TABLE_WORDS == ops.BAN_TABLE_WORDS
    assert macro("LS_BAN_CHUNK") == ops.BAN_CHUNK and macro("LS_BAN_MAX_EXTRA") == ops.BAN_MAX_EXTRA
