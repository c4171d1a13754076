"""The kernels of csrc/sample_band.hip (min_p / typical_p of ``ls_sample_rows_ex``) run once per verification pass and once per
vanilla step, as those of sample.hip: none may use a scratch segment or spill, and the file holds exactly these.  Plus the
layout of ``ls_sample_desc``: the ctypes mirror and the header agree.  Checked without a GPU."""
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


def test_band_kernels_have_no_scratch_and_no_spills():
    u = _usage("sample_band")
    want = {"sample_count_kernel": 1, "sample_minp_kernel": 1, "sample_band_kernel": 1}          # dtype is an argument
    for stem, count in want.items():
        names = [n for n in u if stem in n]
        assert len(names) == count, (stem, names)
        for n in names:
            assert u[n]["VGPRs Spill"] == 0 and u[n]["SGPRs Spill"] == 0 and u[n]["ScratchSize [bytes/lane]"] == 0, (n, u[n])
    assert sum(want.values()) == len(u), sorted(u)


def test_sample_desc_layout_matches_header():
    """Field order and size of the ctypes mirror == ls_sample_desc."""
    from longspec_amd import _C
    txt = open(os.path.join(ROOT, "include", "longspec_hip.h")).read()
    body = txt[txt.index("typedef struct ls_sample_desc {"):txt.index("} ls_sample_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for stmt in body.split("{", 1)[1].split(";"):
        tail = stmt.strip()
        if not tail:
            continue
        for kw in ("const", "void", "uint64_t", "int32_t", "int64_t", "float", "*"):
            tail = tail.replace(kw, " ")
        fields += [f.strip() for f in tail.split(",") if f.strip()]
    assert fields == [f[0] for f in _C.SampleDesc._fields_]
    assert ctypes.sizeof(_C.SampleDesc) == 9 * 8 + 2 * 8 + 4 * 4 + 4 * 4
    assert _C.SampleDesc.ld.offset == 72 and _C.SampleDesc.rows.offset == 88 and _C.SampleDesc.typical_p.offset == 116
