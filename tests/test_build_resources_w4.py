"""The kernels of the 4-bit-weight path must not spill either: the compiler's resource report of the product build
(``_lib/gemm_w4.usage.json``, written by longspec_amd.build) is checked without a GPU."""
import json
import os


def _usage(src):
    from longspec_amd import build
    build.build(verbose=False)
    with open(os.path.join(build.LIBDIR, src + ".usage.json")) as f:
        return json.load(f)


def test_w4_kernels_have_no_scratch():
    u = _usage("gemm_w4")
    gemm = [n for n in u if "skinny_gemm_w4_kernel" in n]
    assert len(gemm) == 2 * (3 * 3 + 2), gemm            # 2 dtypes x (3 epilogues x MT {1, 2, 5} at 4 tiles + 2 epilogues at 8 tiles)
    assert any("quantize_blocks_kernel" in n for n in u) and any("pack_w4_kernel" in n for n in u)
    for n in u:
        assert u[n]["VGPRs Spill"] == 0 and u[n]["SGPRs Spill"] == 0 and u[n]["ScratchSize [bytes/lane]"] == 0, (n, u[n])
    for n in gemm:                                       # M <= 32: at least two workgroups per CU, as the other two formats (this build: three)
        if "Li1ELi4E" in n or "Li2ELi4E" in n:
            assert u[n]["Occupancy [waves/SIMD]"] >= 2, (n, u[n])
