"""The kernels of csrc/stop.hip (``ls_stop_scan``, ``ls_stop_ban_rows``) run inside every round and vanilla step under ``stop=``:
neither may use a scratch segment or spill.  The compiler's resource report of the product build, checked without a GPU."""
import json
import os


def _usage(src):
    from longspec_amd import build
    build.build(verbose=False)
    with open(os.path.join(build.LIBDIR, src + ".usage.json")) as f:
        return json.load(f)


def test_stop_kernels_have_no_scratch_and_no_spills():
    u = _usage("stop")
    want = {"stop_scan_kernel": 1, "stop_ban_rows_kernel": 1}
    for stem, count in want.items():
        names = [n for n in u if stem in n]
        assert len(names) == count, (stem, names)
        for n in names:
            assert u[n]["VGPRs Spill"] == 0 and u[n]["SGPRs Spill"] == 0 and u[n]["ScratchSize [bytes/lane]"] == 0, (n, u[n])
    assert sum(want.values()) == len(u), sorted(u)


def test_stop_source_is_part_of_the_build():
    from longspec_amd import build
    assert "stop.hip" in build.SOURCES
