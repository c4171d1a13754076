"""The lift of a byte DFA to a vocabulary on the device (``ls_guide_lift_hash`` / ``_cols`` / ``_check`` behind
``ops.guide_lift``, ``Guide.from_byte_dfa(device=)`` and ``Guide.from_regex(device=)``) against the host path, exactly: the
lane-packing and multi-slice boundaries of S, one to several thousand tokens, tokens of 0, 1 and 300 bytes, dead tokens,
duplicates, a dead vocabulary, too many behaviours, forced hash collisions, the operators against a Python walk between guard
words, the real vocabulary size once, and two loops end to end under a ``from_regex`` guide."""
import functools
import re

import numpy as np
import pytest
import torch

from longspec_amd import Guide, regex
from test_guide_regex import toy_vocab

pytestmark = pytest.mark.gpu
DEV = "cuda"
LIVE = b"abcdefgh"                # the bytes the random DFAs move on; every other byte is dead


@pytest.fixture(scope="module")
def ops():
    from longspec_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def random_dfa(S, seed, dead=0.25):
    rng = np.random.default_rng(seed)
    nx = np.full((S, 256), -1, dtype=np.int64)
    for b in LIVE:
        col = rng.integers(0, S, size=S)
        col[rng.random(S) < dead] = -1
        nx[:, b] = col
    return nx


def random_tokens(T, seed):
    """T byte strings: one byte, 300 bytes and none among them (where T allows), tokens with a dead byte, short tokens over a
    small alphabet (many duplicates) and exact copies."""
    rng = np.random.default_rng(seed)
    toks = []
    while len(toks) < T:
        kind = rng.random()
        if kind < 0.1:
            toks.append(bytes(rng.choice(list(LIVE + b"\xff"), size=int(rng.integers(1, 5))).tolist()))
        elif kind < 0.2 and toks:
            toks.append(toks[int(rng.integers(0, len(toks)))])
        else:
            toks.append(bytes(rng.choice(list(LIVE[:3 + int(rng.integers(0, 6))]), size=int(rng.integers(1, 10))).tolist()))
    if T >= 8:
        toks[1], toks[3], toks[T - 1] = b"", bytes(rng.choice(list(LIVE), size=300).tolist()), b"\xff"
        toks[5] = b"a"
    return toks


def steps_of(nx, toks):
    """The operands of the operators on the device: (step, blob, offsets)."""
    S = nx.shape[0]
    step = np.full((256, S + 1), S, dtype=np.int16)
    step[:, :S] = np.where(nx < 0, S, nx).T
    offsets = np.zeros(len(toks) + 1, dtype=np.int32)
    np.cumsum([len(t) for t in toks], out=offsets[1:])
    blob = np.frombuffer(b"".join(toks), dtype=np.uint8).copy()
    return torch.from_numpy(step).to(DEV), torch.from_numpy(blob).to(DEV), torch.from_numpy(offsets).to(DEV)


def vector_of(nx, tok):
    out = []
    for s in range(nx.shape[0]):
        for b in tok:
            s = int(nx[s, b])
            if s < 0:
                break
        out.append(s if tok else -1)
    return out


@pytest.mark.parametrize("T", [1, 255, 2000, 4097])
@pytest.mark.parametrize("S", [1, 2, 16, 17, 63, 64, 65, 130, 1000])
def test_the_device_lift_equals_the_host_lift(ops, S, T):
    nx, toks = random_dfa(S, S), random_tokens(T, S + T)
    want = Guide.from_byte_dfa(nx, toks, start=S // 2)
    got = Guide.from_byte_dfa(nx, toks, start=S // 2, device=DEV)
    assert got == want and got.next.dtype == want.next.dtype and got.token_class.dtype == want.token_class.dtype
    if T >= 8:
        assert want.token_class[1] == -1 and want.token_class[T - 1] == -1 and (want.classes > 1 or S == 1)


def test_a_dead_vocabulary_and_a_dead_dfa(ops):
    nx = random_dfa(9, 1)
    for toks in ([b"\xff"] * 70, [b""], [b"", b"\xffa", b"a\xff"]):
        want = Guide.from_byte_dfa(nx, toks)
        assert want.next.shape == (9, 1) and (want.next == -1).all() and (want.token_class == -1).all()
        assert Guide.from_byte_dfa(nx, toks, device=DEV) == want
    dead = np.full((5, 256), -1)
    assert Guide.from_byte_dfa(dead, random_tokens(100, 2), device=DEV) == Guide.from_byte_dfa(dead, random_tokens(100, 2))
    assert Guide.from_byte_dfa(dead, [], device=DEV) == Guide.from_byte_dfa(dead, [])          # (no token: nothing to launch)


def test_too_many_behaviours(ops):
    rng = np.random.default_rng(3)
    nx = rng.integers(0, 32, size=(32, 256))
    toks = [bytes([a, b]) for a in range(256) for b in range(256)]
    with pytest.raises(ValueError, match="distinct behaviours"):
        Guide.from_byte_dfa(nx, toks, device=DEV)


@pytest.mark.parametrize("bits", [0, 3])
def test_forced_collisions_are_regrouped_exactly(ops, monkeypatch, bits):
    nx, toks = random_dfa(65, 11), random_tokens(2000, 12)
    want = Guide.from_byte_dfa(nx, toks)
    stats = {}
    monkeypatch.setattr(ops, "guide_lift", functools.partial(ops.guide_lift, _hash_bits=bits, _stats=stats))
    assert Guide.from_byte_dfa(nx, toks, device=DEV) == want
    print(f"_hash_bits={bits}: {stats['groups']} hash groups, {stats['mismatches']} tokens differ from their representative, "
          f"{want.classes} classes")
    assert stats["groups"] <= 2 ** bits and stats["mismatches"] > 0 and want.classes > 2 ** bits


def test_the_full_hash_finds_every_class(ops, monkeypatch):
    nx, toks = random_dfa(65, 11), random_tokens(2000, 12)
    stats = {}
    monkeypatch.setattr(ops, "guide_lift", functools.partial(ops.guide_lift, _stats=stats))
    g = Guide.from_byte_dfa(nx, toks, device=DEV)
    assert stats == dict(groups=g.classes, mismatches=0)


@pytest.mark.parametrize("S", [5, 64, 70, 300])
def test_cols_against_a_python_walk_between_guard_words(ops, S):
    nx, toks = random_dfa(S, S + 1, dead=0.1), random_tokens(120, S)
    step, blob, offsets = steps_of(nx, toks)
    ids = [0, 1, 3, 5, 119, 7, 7, -1, 120, 2 ** 31 - 1, -2 ** 31] + list(range(20, 46))
    n, guard, mark = len(ids), 64, -123456789
    buf = torch.full((guard + n * S + guard,), mark, dtype=torch.int32, device=DEV)
    out = buf[guard:guard + n * S].view(n, S)
    assert ops.guide_lift_cols(step, blob, offsets, torch.tensor(ids, dtype=torch.int32, device=DEV), out=out) is out
    torch.cuda.synchronize()
    want = [vector_of(nx, toks[t]) if 0 <= t < 120 else [-1] * S for t in ids]
    assert out.cpu().tolist() == want
    assert (buf[:guard] == mark).all() and (buf[guard + n * S:] == mark).all()
    fresh = ops.guide_lift_cols(step, blob, offsets, torch.tensor(ids, dtype=torch.int32, device=DEV))
    assert fresh.cpu().tolist() == want


@pytest.mark.parametrize("S", [5, 64, 70, 300])
def test_hash_and_check_flag_exactly_what_differs(ops, S):
    nx, toks = random_dfa(S, S + 2, dead=0.1), random_tokens(500, S)
    T = len(toks)
    step, blob, offsets = steps_of(nx, toks)
    g = Guide.from_byte_dfa(nx, toks)
    vec = {t: tuple(vector_of(nx, toks[t])) for t in range(T)}
    hashes, alive = ops.guide_lift_hash(step, blob, offsets)
    torch.cuda.synchronize()
    assert hashes.shape == (T, 2) and alive.cpu().tolist() == [int(c >= 0) for c in g.token_class]
    by_hash = {}
    for t, h in enumerate(map(tuple, hashes.cpu().tolist())):                 # equal vectors: equal hashes; and here no collision
        assert by_hash.setdefault(h, vec[t]) == vec[t], t
    assert len(by_hash) == len(set(vec.values()))
    assert len({h[0] for h in by_hash}) == len(by_hash) == len({h[1] for h in by_hash})       # each hash tells them apart alone
    # check: the true grouping is clean between guard bytes; planted wrong groups are flagged, and nothing else
    reps = torch.from_numpy(np.ascontiguousarray(g.next.T).astype(np.int32)).to(DEV)
    group = torch.from_numpy(g.token_class.astype(np.int32)).to(DEV)
    assert ops.guide_lift_check(step, blob, offsets, reps, group).cpu().tolist() == [0] * T
    rng = np.random.default_rng(S)
    live = np.flatnonzero(g.token_class >= 0)
    planted = sorted(rng.choice(live, size=23, replace=False).tolist())
    wrong = g.token_class.copy()
    wrong[planted] = (wrong[planted] + 1 + rng.integers(0, g.classes - 1, size=23)) % g.classes
    wrong[planted[0]] = g.classes                                              # a group the representatives do not have
    got = ops.guide_lift_check(step, blob, offsets, reps, torch.from_numpy(wrong.astype(np.int32)).to(DEV))
    assert got.nonzero().view(-1).cpu().tolist() == planted
    # one differing state is enough
    near = reps.clone()
    c = int(g.token_class[planted[1]])
    near[c, S - 1] = near[c, S - 1] + 1
    got = ops.guide_lift_check(step, blob, offsets, near, group)
    assert got.nonzero().view(-1).cpu().tolist() == np.flatnonzero(g.token_class == c).tolist()


def test_argument_checks(ops):
    from longspec_amd import _C
    nx, toks = random_dfa(6, 1), random_tokens(40, 1)
    step, blob, offsets = steps_of(nx, toks)
    T, S = 40, 6
    hashes, alive = ops.guide_lift_hash(step, blob, offsets)
    ids = torch.arange(4, dtype=torch.int32, device=DEV)
    cols = ops.guide_lift_cols(step, blob, offsets, ids)
    group = torch.zeros(T, dtype=torch.int32, device=DEV)
    mism = ops.guide_lift_check(step, blob, offsets, cols, group)
    lib, p = _C.load(), lambda t: t.data_ptr()
    base = dict(step=p(step), blob=p(blob), offsets=p(offsets), nbytes=blob.numel(), T=T, S=S)
    front = lambda o: [o[k] for k in ("step", "blob", "offsets", "nbytes", "T", "S")]
    for bad in (dict(step=None), dict(blob=None), dict(offsets=None), dict(S=0), dict(S=ops.GUIDE_LIFT_MAX_STATES + 1), dict(T=0),
                dict(nbytes=-1)):
        o = dict(base, **bad)
        assert lib.ls_guide_lift_hash(*front(o), p(hashes), p(alive), None) == _C.LS_ERR_INVALID_ARG, bad
        assert lib.ls_guide_lift_cols(*front(o), p(ids), 4, p(cols), None) == _C.LS_ERR_INVALID_ARG, bad
        assert lib.ls_guide_lift_check(*front(o), p(cols), 4, p(group), p(mism), None) == _C.LS_ERR_INVALID_ARG, bad
    assert lib.ls_guide_lift_hash(*front(base), None, p(alive), None) == _C.LS_ERR_INVALID_ARG
    assert lib.ls_guide_lift_hash(*front(base), p(hashes), None, None) == _C.LS_ERR_INVALID_ARG
    assert lib.ls_guide_lift_cols(*front(base), None, 4, p(cols), None) == _C.LS_ERR_INVALID_ARG
    assert lib.ls_guide_lift_cols(*front(base), p(ids), 0, p(cols), None) == _C.LS_ERR_INVALID_ARG
    assert lib.ls_guide_lift_cols(*front(base), p(ids), 4, None, None) == _C.LS_ERR_INVALID_ARG
    assert lib.ls_guide_lift_check(*front(base), None, 4, p(group), p(mism), None) == _C.LS_ERR_INVALID_ARG
    assert lib.ls_guide_lift_check(*front(base), p(cols), 0, p(group), p(mism), None) == _C.LS_ERR_INVALID_ARG
    assert lib.ls_guide_lift_check(*front(base), p(cols), 4, None, p(mism), None) == _C.LS_ERR_INVALID_ARG
    assert lib.ls_guide_lift_check(*front(base), p(cols), 4, p(group), None, None) == _C.LS_ERR_INVALID_ARG
    for bad in (dict(step=step.int()), dict(step=step[:, :0]), dict(step=step.cpu()), dict(step=step.t()), dict(blob=blob.int()),
                dict(offsets=offsets.long()), dict(offsets=offsets[:1])):
        kw = dict(dict(step=step, blob=blob, offsets=offsets), **bad)
        with pytest.raises((TypeError, RuntimeError)):
            ops.guide_lift(**kw)
    with pytest.raises(TypeError):
        ops.guide_lift_cols(step, blob, offsets, ids.long())
    with pytest.raises(TypeError):
        ops.guide_lift_cols(step, blob, offsets, ids, out=cols[:, :5])
    with pytest.raises(TypeError):
        ops.guide_lift_check(step, blob, offsets, cols, group[:5])
    # offsets that do not lie in the blob: the token counts as empty, nothing beyond the blob is read
    broken = offsets.clone()
    broken[3], broken[4] = 2 ** 30, -5
    _, alive2 = ops.guide_lift_hash(step, blob, broken)
    assert alive2[2:4].tolist() == [0, 0] and alive2[5:].tolist() == alive[5:].tolist()


def counter_dfa(S):
    """Digits advance the state (the last one has no digit left), letters stay, every other byte is dead."""
    nx = np.full((S, 256), -1, dtype=np.int64)
    for b in b"0123456789":
        nx[:S - 1, b] = np.arange(1, S)
    for b in range(256):
        if chr(b).isalpha() and b < 128:
            nx[:, b] = np.arange(S)
    return nx


def counter_vocab(T, seed=0):
    rng = np.random.default_rng(seed)
    src = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGH0123456789 .", dtype=np.uint8)
    lens = rng.integers(1, 10, size=T)
    flat = src[rng.integers(0, src.size, size=int(lens.sum()))].tobytes()
    ends = np.cumsum(lens)
    return [flat[e - n:e] for e, n in zip(ends.tolist(), lens.tolist())]


def test_the_real_vocabulary_size(ops):
    nx, toks = counter_dfa(128), counter_vocab(128256)
    want = Guide.from_byte_dfa(nx, toks)
    assert Guide.from_byte_dfa(nx, toks, device=DEV) == want and want.classes >= 9          # a class per number of digits


@pytest.mark.parametrize("p", [r"-?(0|[1-9]\d*)(\.\d+)?([eE][+-]?\d+)?", r"\w+@\w+\.(com|org)", "[é€a]+"])
def test_from_regex_on_the_device_equals_the_host(ops, p):
    toks, eos = toy_vocab()
    want = Guide.from_regex(p, toks, eos)
    assert Guide.from_regex(p, toks, eos, device=DEV) == want
    assert Guide.from_regex(p, toks, eos, device=torch.device("cuda", 0)) == want


# ---- end to end ------------------------------------------------------------------------------------------------------
PATTERN = r"[a-h]{1,6}( [a-h]{1,6}){0,5}\."


def toy_token_bytes(V, eos):
    """Byte strings for the V ids of the toy models: one to three bytes over letters, the space, the full stop and digits, every
    single byte of the pattern's alphabet among them; id 0 and the end-of-sequence id hold nothing."""
    rng = np.random.default_rng(5)
    src = list(b"abcdefgh" * 3 + b"   ..0123")
    toks = [bytes(rng.choice(src, size=int(rng.integers(1, 4))).tolist()) for _ in range(V)]
    for i, b in enumerate(b"abcdefgh ."):
        toks[10 + 37 * i] = bytes([b])
    toks[0] = b""
    if 0 <= eos < V:
        toks[eos] = b""
    return toks


def test_vanilla_and_tree_under_a_regex_guide_replayed_from_graphs(ops):
    import sampled_runs as sr
    import test_gpu_generate_guide as gg
    import test_gpu_generate_lookup as gk
    import test_host_generate_guide as hg
    family, name = "llama", "mixed"
    run, m = gk.model_of(family, name)
    tol = sr.TOL[run["dtype"]]
    eos, V = hg.eos_of(run, m), run["cfg"].vocab_size
    toks = toy_token_bytes(V, eos)
    guide = Guide.from_regex(PATTERN, toks, eos, device=DEV)
    assert guide == Guide.from_regex(PATTERN, toks, eos)
    dfa, want = regex.compile(PATTERN), re.compile(PATTERN, re.ASCII)
    ref, rows = gg.device_vanilla(family, name, guide, eos)
    plain, _ = gk.vanilla(family, name)
    assert ref != plain[:len(ref)], "the guide must bite"
    texts = {"the device's vanilla run": ref}
    for loop in ("vanilla", "tree"):
        g = gg.glide_loop(family, name, loop, guide, graphs=True)
        assert g.st.replayer.captures > 0 and not g.st.replayer.disabled, loop
        text = gg.cut(g.out[:min(g.n, gg.GEN)], eos)
        gg.explained(text, ref, rows, tol, (name, loop, "replayed"))
        texts[loop] = text
    ended = 0
    for what, text in texts.items():
        body = text[:-1] if text and text[-1] == eos else text
        assert eos not in body, what
        s = 0
        for c, t in enumerate(body):                                            # the bytes keep the byte DFA alive at every column
            assert toks[t], (what, c)
            for b in toks[t]:
                s = int(dfa.next[s, b])
                assert s >= 0, (what, c, t)
        if text and text[-1] == eos:
            data = b"".join(toks[t] for t in body)
            assert dfa.accepting[s] and want.fullmatch(data.decode("utf-8")), (what, data)
            ended += 1
    assert ended == len(texts), "the pattern bounds the text below the generated length: every run ends"
