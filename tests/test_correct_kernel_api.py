"""rsgpu_set_correct_kernel on the CPU (include/rsgpu.h): the choices of the
wrapper and of the header agree, the symbol is exported and bound, a null
context is an argument error; the damage the GPU suite plans
(tests/correct_fused_cases.py, tests/correct_cases.py) gives, on the model
alone, one-row and two-row corrections and columns left alone in every block,
so that the GPU comparison cannot pass on trivial input; and the pair search
of k_rs_bs_correct (csrc/rs_pairs.h, through the test-hooks library) agrees
with the model's brute force over all pairs (tests/correct_model.py) in count,
rows and values.

A column that two different pairs explain: none is planted here, because the
compiled codes have none.  Two pairs explaining one column make at most four
columns of [C | I] dependent; with C's entries 2^(p r) any four data columns
are a Vandermonde matrix, three data columns stay independent on the three
consecutive coordinates that one missing coordinate leaves when e >= 7, two
data columns are not proportional on two consecutive coordinates, and a data
column has no zero entry.  The bounded search that goes with the argument:
correct_model.explaining_pairs, which tries every pair of rows and every
(x, y), on each planned and drawn two-row column of the five codes below (a
few hundred columns, every kind of pair) found the planted pair and no
other."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import correct_cases as cc
import correct_fused_cases as fc
import correct_model as cm
import rsgpu
import scrub_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rsgpu.h")


def test_the_wrapper_s_choices():
    assert rsgpu.CORRECT_KERNELS == {"auto": 0, "two_pass": 1, "fused": 2}
    assert "CORRECT_KERNELS" in rsgpu.__all__
    assert "rsgpu_set_correct_kernel" in rsgpu.EXPORTED_SYMBOLS
    assert callable(rsgpu.Context.set_correct_kernel)


def test_the_header_s_constants():
    txt = open(HEADER).read()
    got = dict(re.findall(r"^#define RSGPU_CORRECT_(AUTO|TWO_PASS|FUSED)\s+(\d+)\s*$", txt, re.M))
    assert {k.lower(): int(v) for k, v in got.items()} == rsgpu.CORRECT_KERNELS
    assert re.search(r"^int rsgpu_set_correct_kernel\(rsgpu_ctx \*ctx, int kernel\);", txt, re.M)


def test_the_symbol_is_exported_and_bound():
    fn = rsgpu.lib().rsgpu_set_correct_kernel
    assert fn.restype is C.c_int and fn.argtypes == [C.c_void_p, C.c_int]


def test_null_context_is_an_argument_error():
    for kernel in (0, 1, 2, 3, -1):
        assert rsgpu.lib().rsgpu_set_correct_kernel(None, kernel) == -1


def syndrome(c, hits):
    """The syndrome column of a column damaged as `hits`: sum of x h_r."""
    e, k = c.shape
    s = np.zeros(e, np.uint8)
    for r, x in hits:
        if r < k:
            s ^= sm.gf_mul(c[:, r], np.uint8(x))
        else:
            s[r - k] ^= x
    return s


def fixes(c, entries):
    """Per planned column the number of rows the model corrects (0: left alone)."""
    return [len(cm.verdict(c, syndrome(c, hits), 2)) for _, _, hits in entries]


@pytest.mark.parametrize("k,e", fc.T2_CODES, ids=str)
def test_the_planned_damage_is_not_trivial(k, e):
    """Both plans at L = 4160, blocks 0..2: at least 9 two-row corrections, a
    one-row correction and a column left alone per block; correct_cases.plan
    gives 3, 14 and 2 of them."""
    c = sm.rs_matrix(k, e)
    for b in range(3):
        n = fixes(c, fc.plan(k, e, 4160, b))
        assert n.count(2) >= 9 and n.count(1) >= 1 and n.count(0) >= 1, (b, n)
        kinds = {kind for kind, _, _ in fc.plan(k, e, 4160, b)}
        assert set(fc.PAIR_KINDS) | {"one", "one-parity", "three", "three-mixed"} <= kinds
        n = fixes(c, cc.plan(k, e, 4160, b))
        assert (n.count(1), n.count(2), n.count(0)) == (3, 14, 2), (b, n)


def test_the_plan_s_positions():
    """Every position the fused kernel's cold path distinguishes is planned."""
    for L in (32, 2080, 4160):
        cols = [c for _, c, _ in fc.plan(64, 32, L, 0)]
        assert len(cols) == len(set(cols)) and all(0 <= c < L for c in cols) and L - 1 in cols
    plan = fc.plan(64, 32, 4160, 0)
    pending = {c for kind, c, _ in plan if kind in fc.PAIR_KINDS}
    one = {c for kind, c, _ in plan if kind.startswith("one")}
    where = lambda c: (c // 2048, c % 2048 // 32, c % 32 // 8, c % 8)  # noqa: E731  tile, lane, pass, byte
    for pas in range(4):
        assert any(where(c)[:3:2] == (0, pas) for c in pending) and any(where(c)[:3:2] == (0, pas) for c in one)
    assert any(c + 1 in pending and c % 8 < 7 for c in pending), "adjacent bytes"
    assert any(where(c)[:3] == where(d)[:3] for c in pending for d in one), "one 8-byte group"
    for nw in (2, 4):
        per_pass = [{(8 * where(c)[1] + where(c)[3]) % (64 * nw) // 64 for c in pending if where(c)[::2] == (0, pas)}
                    for pas in range(4)]
        assert any(len(w) == nw for w in per_pass), ("waves", nw)
    for nw in (1, 2, 4):
        assert any(c + 32 * 8 * nw in pending and where(c)[0] == where(c + 32 * 8 * nw)[0] for c in pending), nw
    assert {0, 2047, 2048, 4096, 4159} <= pending and 4128 in pending


_hook = None


def pair_search(k, e, s):
    global _hook
    if _hook is None:
        _hook = rsgpu.testhooks().rsgpu_internal_rs_pair_search
        _hook.restype = C.c_int
        _hook.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    s = np.ascontiguousarray(s, np.uint8)
    out = np.full(4, -1, np.int32)
    n = _hook(k, e, s.ctypes.data, out.ctypes.data)
    return n, tuple(int(v) for v in out)


def drawn(k, e, n, seed):
    """n damaged columns: one, two and three rows, every kind of pair."""
    rng = np.random.default_rng(seed)
    kinds = ("one", "one-parity", "three", "three-mixed") + fc.PAIR_KINDS * 2
    return [(kinds[i % len(kinds)], i, fc.hits_of(kinds[i % len(kinds)], k, e, rng)) for i in range(n)]


@pytest.mark.parametrize("k,e", fc.T2_CODES, ids=str)
def test_the_pair_search_is_the_model_s(k, e):
    c = sm.rs_matrix(k, e)
    assert pair_search(k, 2, np.zeros(2, np.uint8))[0] == -1 and pair_search(256, e, np.zeros(e, np.uint8))[0] == -1
    entries = fc.plan(k, e, 4160, 0) + cc.plan(k, e, 4160, 1) + drawn(k, e, 64, 9 * k + e)
    two = 0
    for kind, _, hits in entries:
        s = syndrome(c, hits)
        pairs = cm.explaining_pairs(c, s)
        want = len({(a, b) for a, b, _, _ in pairs})
        got, out = pair_search(k, e, s)
        assert got == min(want, 2), (kind, hits, pairs, got, out)
        if want == 1:
            assert out == pairs[0], (kind, hits, pairs, out)
            two += 1
        if kind in fc.PAIR_KINDS or kind.startswith("data+") or kind.startswith("parity"):
            # the planted pair and no other (the module's docstring)
            assert [(a, x) for a, b, x, y in pairs] + [(b, y) for a, b, x, y in pairs] == sorted(hits), (kind, hits, pairs)
    assert two >= 60
