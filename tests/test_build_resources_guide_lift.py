"""The kernels of csrc/guide_lift.hip (``ls_guide_lift_hash`` / ``_cols`` / ``_check``) walk tokens x states gathers per request:
they may not use a scratch segment or spill.  The compiler's resource report of the product build, checked without a GPU."""
import json
import os
import re


def test_guide_lift_kernels_have_no_scratch_and_no_spills():
    from longspec_amd import build
    build.build(verbose=False)
    with open(os.path.join(build.LIBDIR, "guide_lift.usage.json")) as f:
        u = json.load(f)
    names = [n for n in u if "guide_lift_kernel" in n]
    assert len(names) == 6 and len(u) == 6, sorted(u)                # three modes, one and four slices of 64 states per pass
    for n in names:
        assert u[n]["VGPRs Spill"] == 0 and u[n]["SGPRs Spill"] == 0 and u[n]["ScratchSize [bytes/lane]"] == 0, (n, u[n])
        assert u[n]["Occupancy [waves/SIMD]"] == 8, (n, u[n])        # a latency-bound gather chain: it lives on resident waves


def test_guide_lift_source_is_part_of_the_build():
    from longspec_amd import build
    assert "guide_lift.hip" in build.SOURCES


def test_the_state_limit_agrees():
    from longspec_amd import guide, ops
    here = os.path.dirname(os.path.abspath(__file__))
    txt = open(os.path.join(os.path.dirname(here), "include", "longspec_hip.h")).read()
    macro = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))
    assert macro("LS_GUIDE_LIFT_MAX_STATES") == ops.GUIDE_LIFT_MAX_STATES == guide.LIFT_MAX_STATES == 16384
    assert macro("LS_GUIDE_MAX_CLASSES") == ops.GUIDE_MAX_CLASSES == guide.MAX_CLASSES
    assert ops.GUIDE_LIFT_MAX_STATES < 2 ** 15                       # a state, the dead one included, is a non-negative int16
