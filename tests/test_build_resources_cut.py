"""The kernels of csrc/sample_cut.hip (top_n_sigma / xtc of ``ls_sample_rows_cut``) run once per verification pass and once per
vanilla step, as those of sample.hip: none may use a scratch segment or spill, and the file holds exactly these.  Plus the
layout of ``ls_sample_cut``: the ctypes mirror and the header agree.  Checked without a GPU."""
import ctypes
import json
import os
import re

from conftest import ROOT


def _usage(src):
    from longspec_amd import build
    build.build(verbose=False)
    with open(os.path.join(build.LIBDIR, src + ".usage.json")) as f:
        return json.load(f)


def test_cut_kernels_have_no_scratch_and_no_spills():
    from longspec_amd import build
    assert "sample_cut.hip" in build.SOURCES
    u = _usage("sample_cut")
    want = {"sample_sigma_part_kernel": 2, "sample_sigma_finish_kernel": 1, "sample_xtc_sum_kernel": 2, "sample_xtc_cut_kernel": 1,
            "sample_xtc_find_kernel": 2, "sample_xtc_store_kernel": 1}                              # 2: fp16 and bf16
    for stem, count in want.items():
        names = [n for n in u if stem in n]
        assert len(names) == count, (stem, names)
        for n in names:
            assert u[n]["VGPRs Spill"] == 0 and u[n]["SGPRs Spill"] == 0 and u[n]["ScratchSize [bytes/lane]"] == 0, (n, u[n])
    assert sum(want.values()) == len(u), sorted(u)


def test_sample_cut_layout_matches_header():
    """Field order and size of the ctypes mirror == ls_sample_cut."""
    from longspec_amd import _C
    txt = open(os.path.join(ROOT, "include", "longspec_hip.h")).read()
    body = txt[txt.index("typedef struct ls_sample_cut {"):txt.index("} ls_sample_cut;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for stmt in body.split("{", 1)[1].split(";"):
        tail = stmt.strip()
        if not tail:
            continue
        for kw in ("int32_t", "float"):
            tail = tail.replace(kw, " ")
        fields += [f.strip() for f in tail.split(",") if f.strip()]
    assert fields == [f[0] for f in _C.SampleCut._fields_] == ["top_n_sigma", "xtc_probability", "xtc_threshold", "reserved"]
    assert ctypes.sizeof(_C.SampleCut) == 16
    assert [getattr(_C.SampleCut, f).offset for f in fields] == [0, 4, 8, 12]
    assert _C.SampleCut.reserved.size == 4


def test_the_old_descriptor_is_untouched():
    from longspec_amd import _C
    assert ctypes.sizeof(_C.SampleDesc) == 120
