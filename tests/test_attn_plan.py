"""The attention launch plan (``plan_attn`` in csrc/attn.hip) as its three planning entry points show it --
``ls_attn_kernel_name``, ``ls_attn_num_parts``, ``ls_attn_workspace_bytes`` -- against ``tests/golden/attn_plan.json``, and
the argument errors ``ls_attn_fwd`` must report before it launches anything.  No GPU: planning is host arithmetic, and
without a device the library plans for 256 CUs, which is also the MI355X's count.

The table was recorded from the library built at the commit BEFORE the plan was gathered into one function
(``python tests/test_attn_plan.py --record``, with ``LONGSPEC_HIP_LIB`` naming that build and the default ``LS_ATTN_KERNEL``);
re-record it only from a commit whose dispatch is known good, never to make a failure go away."""
import ctypes as C
import json
import os

import pytest

from conftest import GOLDEN
from test_gpu_attn_dispatch import DRAFT_MN, VERIFY_TABLE

from longspec_amd import _C
from longspec_amd._C import LS_NEW_DRAFT, LS_NEW_FLASH, LS_NEW_NONE, LS_NEW_TARGET

TABLE = os.path.join(GOLDEN, "attn_plan.json")
LS_ERR_INVALID_ARG, LS_ERR_WORKSPACE = -1, -3
FIELDS = ("b", "sq", "H", "Hkv", "new_mode", "n_new", "causal", "window_left", "n_app", "kv_len_hint", "n_splits")
HINTS = [0, 1, 63, 64, 65, 4095, 4096, 16384, 16421, 131051, 131072]
# With 8 kv heads and b = 1 a call without a new-key block aims at 256 / 8 = 32 splits; 32768 / 32 and 65536 / 32 rows are
# multiples of 512 rows, so pick_splits' odd-stride loop gives one split up (test_odd_stride_hints_drop_a_split).
ODD_STRIDE_HINTS = [32768, 65536]
SHORT_HINTS = [0, 300, 4095, 4096, 131072]


def desc(b, sq, H, Hkv, new_mode, n_new, causal, window_left, n_app, kv_len_hint, n_splits, q_pad=0, q=1):
    """A descriptor with non-null placeholders for the tensors: planning dereferences none of them."""
    d = _C.AttnDesc()
    d.q = q
    d.k_cache = d.v_cache = d.cache_seqlens = 1
    d.b, d.sq, d.H, d.Hkv, d.dtype = b, sq, H, Hkv, _C.LS_F16
    d.new_mode, d.n_new, d.causal, d.window_left, d.n_app = new_mode, n_new, causal, window_left, n_app
    d.kv_len_hint, d.n_splits = kv_len_hint, n_splits
    if new_mode != LS_NEW_NONE:
        d.k_new = d.v_new = d.mask_bits = 1
        d.mask_words = (n_new + 31) // 32
        d.scatter_new = 1
    d.softmax_scale = 128 ** -0.5
    d.q_stride_h = d.kc_stride_h = d.kn_stride_h = d.out_stride_h = 128
    d.q_stride_s = H * 128 + q_pad
    d.out_stride_s = H * 128
    d.kc_stride_s = d.kn_stride_s = Hkv * 128
    return d


# the call forms of ops.py: (new_mode, n_new from sq, causal, window_left, n_app from sq)
def verify(sq):
    return (LS_NEW_TARGET, sq, 0, -1, 0)


def plain(sq):
    return (LS_NEW_NONE, 0, 0, -1, 0)


def causal(sq):
    return (LS_NEW_NONE, 0, 1, -1, 0)


def window(sq):
    return (LS_NEW_NONE, 0, 1, 512, 0)


def append_chunk(sq):
    return (LS_NEW_FLASH, sq, 1, -1, sq)


def append_window(sq):
    return (LS_NEW_FLASH, sq, 1, 512, sq)


def grid():
    """The descriptor grid, as tuples in FIELDS order: every (H, Hkv, R) of the dispatch test's tables in the call forms it
    is used with, crossed with the hints, and thinned crosses with batch, a forced split count and 1 / 8 kv heads."""
    rows = [(H, Hkv, R) for H, Hkv, R, *_ in VERIFY_TABLE]
    extra = [(g * Hkv, Hkv, R) for Hkv in (1, 8) for g in (1, 4, 5) for R in (1, 16, 74, 80, 97, 192, 193)]
    out = []

    def add(b, sq, H, Hkv, form, hint, n_splits):
        out.append((b, sq, H, Hkv) + form(sq) + (hint, n_splits))

    for H, Hkv, R in rows:
        for form in (verify, plain):
            for hint in HINTS + ODD_STRIDE_HINTS:
                add(1, R, H, Hkv, form, hint, 0)
        for form in (causal, window, append_chunk, append_window):
            for hint in SHORT_HINTS:
                add(1, R, H, Hkv, form, hint, 0)
    for H, Hkv, R in extra:
        for form in (verify, plain, append_chunk):
            for hint in (65, 4096, 16421, 131051) + tuple(ODD_STRIDE_HINTS):
                add(1, R, H, Hkv, form, hint, 0)
    for H, Hkv, R in rows[::4] + extra[::3]:
        for form in (verify, plain, window, append_chunk):
            for hint in (64, 4096, 131072):
                for b, n_splits in ((3, 0), (1, 3), (3, 3)):
                    add(b, R, H, Hkv, form, hint, n_splits)
    for M, N in DRAFT_MN:                       # the draft tree step: M query rows, N new keys
        for H, Hkv in ((2, 2), (4, 1), (32, 8)):
            for hint in (0, 5, 511, 512, 513, 2000, 4096):
                for b in (1, 3):
                    out.append((b, M, H, Hkv, LS_NEW_DRAFT, N, 0, -1, 0, hint, 0))
    out = list(dict.fromkeys(out))              # the two row lists overlap
    assert len(out) <= 5000, len(out)
    return out


def invalid_descs():
    """Descriptors every entry point must refuse."""
    ok = (1, 74, 8, 2) + verify(74) + (4096, 0)
    return {"stride not a multiple of 8": desc(*ok, q_pad=4),
            "n_new = 257": desc(1, 257, 4, 4, *verify(257), 300, 0),
            "null q": desc(*ok, q=None)}


def plan_of(lib, d):
    return [lib.ls_attn_kernel_name(C.byref(d)).decode(), lib.ls_attn_num_parts(C.byref(d)),
            lib.ls_attn_workspace_bytes(C.byref(d))]


def workspace_errors(lib):
    """(what, return code, message) of ls_attn_fwd with a short and with a null workspace: it returns before any launch."""
    d = desc(1, 74, 8, 2, *verify(74), 4096, 0)
    need = lib.ls_attn_workspace_bytes(C.byref(d))
    buf = C.create_string_buffer(64)
    got = []
    for what, ws, nbytes in (("short", C.addressof(buf), need - 1), ("null", None, need)):
        rc = lib.ls_attn_fwd(C.byref(d), ws, nbytes, None)
        got.append([what, rc, lib.ls_last_error().decode()])
    return got


@pytest.fixture(scope="module")
def lib():
    from longspec_amd.build import build
    build(verbose=False)
    return _C.load()


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


def test_grid_holds_what_it_must():
    g = grid()
    col = {f: {r[i] for r in g} for i, f in enumerate(FIELDS)}
    assert col["b"] == {1, 3} and col["n_splits"] == {0, 3} and {1, 8} <= col["Hkv"]
    assert set(HINTS + ODD_STRIDE_HINTS) <= col["kv_len_hint"]
    assert {192, 193} <= col["n_new"]
    forms = {r[4:9] for r in g}
    for H, Hkv, R, *_ in VERIFY_TABLE:
        for form in (verify, plain, causal, window, append_chunk):
            assert form(R) in forms and (1, R, H, Hkv) + form(R) + (4096, 0) in g


def test_plan_matches_the_recorded_table(lib, table):
    g = grid()
    assert table["fields"] == list(FIELDS) + ["kernel", "n_parts", "workspace_bytes"]
    assert [tuple(r[:len(FIELDS)]) for r in table["records"]] == g, "the grid moved: the table no longer describes it"
    wrong = []
    for r in table["records"]:
        got = plan_of(lib, desc(*r[:len(FIELDS)]))
        if got != [table["kernels"][r[-3]], r[-2], r[-1]]:
            wrong.append((r, got))
    assert not wrong, f"{len(wrong)} of {len(g)} plans differ, first: {wrong[:3]}"
    assert {table["kernels"][r[-3]] for r in table["records"]} == {"attn_partial_kernel", "attn_partial_ws_kernel"}


def test_odd_stride_hints_drop_a_split(table):
    """H = Hkv = 8, one query row (class "1": two key slices per split), no new-key block: 31 splits, not 32."""
    for hint in ODD_STRIDE_HINTS:
        (r,) = [r for r in table["records"] if tuple(r[:len(FIELDS)]) == (1, 1, 8, 8) + plain(1) + (hint, 0)]
        assert r[-2] == 31 * 2


def test_invalid_descriptors(lib):
    for what, d in invalid_descs().items():
        assert plan_of(lib, d) == ["invalid", LS_ERR_INVALID_ARG, 0], what
    assert lib.ls_attn_kernel_name(None).decode() == "invalid" and lib.ls_attn_workspace_bytes(None) == 0


def test_workspace_errors_keep_code_and_text(lib, table):
    got = workspace_errors(lib)
    assert got == table["workspace_errors"]
    assert [g[1] for g in got] == [LS_ERR_WORKSPACE] * 2 and all("workspace" in g[2] and "bytes" in g[2] for g in got)


def test_output_errors_come_before_any_launch(lib):
    """``out == NULL``, and ``lse`` in LS_NEW_TARGET mode: LS_ERR_INVALID_ARG with the messages these checks have always
    had.  They sit in front of stage 1 (this test has no device to launch on), where they used to follow it."""
    d = desc(1, 74, 8, 2, *verify(74), 4096, 0)
    need = lib.ls_attn_workspace_bytes(C.byref(d))
    ws = C.create_string_buffer(64)            # never touched: both calls return before a launch
    assert lib.ls_attn_fwd(C.byref(d), C.addressof(ws), need, None) == LS_ERR_INVALID_ARG
    assert lib.ls_last_error().decode() == "out is null"
    d.out = d.lse = 1
    assert lib.ls_attn_fwd(C.byref(d), C.addressof(ws), need, None) == LS_ERR_INVALID_ARG
    assert lib.ls_last_error().decode() == "no lse output in LS_NEW_TARGET mode"


def record():
    from longspec_amd.build import build
    if not os.environ.get("LONGSPEC_HIP_LIB"):
        build(verbose=False)
    lib = _C.load()
    kernels = ["attn_partial_kernel", "attn_partial_ws_kernel", "invalid"]
    records = []
    for r in grid():
        name, parts, nbytes = plan_of(lib, desc(*r))
        records.append(list(r) + [kernels.index(name), parts, nbytes])
    table = {"library": "recorded from the build of the commit before plan_attn() (one plan per descriptor)",
             "fields": list(FIELDS) + ["kernel", "n_parts", "workspace_bytes"], "kernels": kernels,
             "workspace_errors": workspace_errors(lib)}
    with open(TABLE, "w") as f:
        f.write(json.dumps(table)[:-1] + ', "records": [\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in records)
                + "\n]}\n")
    print(f"{len(records)} records from {_C.LIB_PATH} -> {TABLE} ({os.path.getsize(TABLE)} bytes)")


if __name__ == "__main__":
    import sys
    if "--record" in sys.argv:
        record()
