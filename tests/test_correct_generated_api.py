"""The correction fused into the generated scrub (k_rs_jit_correct,
k_rs_jitw_correct; include/rsgpu.h rsgpu_set_correct_kernel) on the CPU: the
damage the GPU suite plans by position in the generated tile
(tests/correct_generated_cases.py) covers every position the cold path
distinguishes and gives, on the model alone, two-row and one-row corrections
and columns left alone in every block, so that the GPU comparison cannot pass
on trivial input; the pair search the kernels run per lane (csrc/rs_pairs.h
pair_search_lane, through the test-hooks library) agrees with the model's
brute force over all pairs (tests/correct_model.py) in count, rows and values,
for matrices read from memory, matrices with columns that two pairs explain and
more than 64 data rows; and the opt-in adds no constant."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import correct_cases as cc
import correct_fused_cases as fc
import correct_generated_cases as gc
import correct_model as cm
import rsgpu
import scrub_model as sm
from test_correct_kernel_api import drawn, fixes, syndrome

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rsgpu.h")

# every matrix of the GPU suite's t = 2 cases, and the wide ones of its bands
MATRICES = gc.T2_SHAPES + [(65, 6, "cauchy"), (129, 7, "cauchy")]


def matrix(k, e, kind):
    return sm.rs_matrix(k, e) if kind == "rs" else sm.cauchy_matrix(k, e)


def test_the_plan_s_positions():
    """Every position the generated kernels' cold path distinguishes is planned."""
    for L in (32, 2112, gc.L0):
        cols = [c for _, c, _ in gc.plan(14, 32, L, 0)]
        assert len(cols) == len(set(cols)) and all(0 <= c < L for c in cols) and L - 1 in cols
    L = gc.L0
    plan = gc.plan(14, 32, L, 0)
    pending = {c for kind, c, _ in plan if kind in fc.PAIR_KINDS}
    one = {c for kind, c, _ in plan if kind.startswith("one")}
    three = {c for kind, c, _ in plan if kind.startswith("three")}
    where = gc.where
    for pas in range(8):
        assert any(where(c)[:3:2] == (0, pas) for c in pending) and any(where(c)[:3:2] == (0, pas) for c in one)
    assert any(c + 1 in pending and c % 4 < 3 for c in pending), "adjacent bytes"
    assert any(where(c)[:3] == where(d)[:3] for c in pending for d in one), "one dword"
    # a pass with a pending column in every wave's share: wave = lane mod 16 NV div 16
    for nv in (1, 2, 4):
        per_pass = [{where(c)[1] % (16 * nv) // 16 for c in pending if where(c)[::2] == (0, pas)} for pas in range(8)]
        assert any(len(w) == nv for w in per_pass), ("waves", nv)
    # two trips of one thread: columns c and c + 64 NV of a pass, 32 * 16 NV bytes apart
    for nv in (1, 2):
        assert any(c + 32 * 16 * nv in pending and where(c)[0] == where(c + 32 * 16 * nv)[0] for c in pending), nv
    assert {0, 2047, 2048} <= pending
    t0 = (L - 1) // 2048 * 2048
    assert t0 == 3 * 2048 and {t0, L - 32, L - 1} <= pending and t0 + 6 in one and len(three) == 3
    # TPW = 3: workgroup 0's three tiles are dirty, the last workgroup owns tiles past the row end
    assert {where(c)[0] for c in pending | one} == {0, 1, 2, 3} and (L + 2047) // 2048 == 4


@pytest.mark.parametrize("k,e,kind", gc.T2_SHAPES + gc.BAND_SHAPES[:2], ids=str)
def test_the_planned_damage_is_not_trivial(k, e, kind):
    """The tile plan at L0, blocks 0..2: at least 9 two-row corrections, a
    one-row correction and a column left alone per block, on the model alone;
    correct_fused_cases.plan and correct_cases.plan likewise."""
    c = matrix(k, e, kind)
    for b in range(3):
        n = fixes(c, gc.plan(k, e, gc.L0, b))
        assert n.count(2) >= 9 and n.count(1) >= 1 and n.count(0) >= 1, (b, n)
        kinds = {kd for kd, _, _ in gc.plan(k, e, gc.L0, b)}
        assert set(fc.PAIR_KINDS) | {"one", "one-parity", "three", "three-mixed"} <= kinds
        n = fixes(c, fc.plan(k, e, 4160, b))
        assert n.count(2) >= 9 and n.count(1) >= 1 and n.count(0) >= 1, (b, n)
        n = fixes(c, cc.plan(k, e, 4160, b))
        assert (n.count(1), n.count(2), n.count(0)) == (3, 14, 2), (b, n)


_hook = None


def pair_search(c, s, k=None, e=None):
    global _hook
    if _hook is None:
        _hook = rsgpu.testhooks().rsgpu_internal_pair_search
        _hook.restype = C.c_int
        _hook.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    c = np.ascontiguousarray(c, np.uint8)
    s = np.ascontiguousarray(s, np.uint8)
    out = np.full(4, -1, np.int32)
    n = _hook(c.shape[1] if k is None else k, c.shape[0] if e is None else e, c.ctypes.data, s.ctypes.data,
              out.ctypes.data)
    return n, tuple(int(v) for v in out)


def agrees(c, hits, kind=""):
    """The hook on the column damaged as `hits` against the model's pairs;
    the number of distinct pairs the model finds."""
    s = syndrome(c, hits)
    pairs = cm.explaining_pairs(c, s)
    want = len({(a, b) for a, b, _, _ in pairs})
    got, out = pair_search(c, s)
    assert got == min(want, 2), (kind, hits, pairs, got, out)
    if want == 1:
        assert out == pairs[0], (kind, hits, pairs, out)
    return want


@pytest.mark.parametrize("k,e,kind", MATRICES, ids=str)
def test_the_pair_search_is_the_model_s(k, e, kind):
    """Planned and drawn columns of every matrix: one, two and three damaged
    rows, every kind of pair."""
    c = matrix(k, e, kind)
    entries = gc.plan(k, e, gc.L0, 0) + cc.plan(k, e, 4160, 1) + drawn(k, e, 64, 9 * k + e)
    unique = sum(agrees(c, hits, kd) == 1 for kd, _, hits in entries)
    assert unique >= 60


def test_argument_errors():
    c = sm.cauchy_matrix(10, 5)
    assert pair_search(c, np.zeros(5, np.uint8), e=2)[0] == -1
    assert pair_search(c, np.zeros(5, np.uint8), k=256)[0] == -1
    assert pair_search(c, np.zeros(5, np.uint8), e=65)[0] == -1
    assert pair_search(c, np.zeros(5, np.uint8), k=0)[0] == -1


@pytest.mark.parametrize("make,columns,two", [
    (cc.dependent_matrix, cc.AMBIGUOUS + cc.UNIQUE, len(cc.AMBIGUOUS)),
    (cc.dependent_wide_matrix, cc.AMBIGUOUS_WIDE + cc.UNIQUE_WIDE, len(cc.AMBIGUOUS_WIDE))], ids=["(12, 6)", "(129, 7)"])
def test_two_matching_pairs_return_two(make, columns, two):
    """Columns that two pairs explain: 2, in one band of 64 data rows, in
    neighbouring ones and in the last; the columns beside them: their pair."""
    c = make()
    n = [agrees(c, hits) for _, hits in columns]
    assert n[:two] == [2] * two and n[two:] == [1] * (len(columns) - two), n
    assert [pair_search(c, syndrome(c, hits))[0] for _, hits in columns] == n


@pytest.mark.parametrize("k,e", [(129, 7), (245, 5)], ids=str)
def test_pairs_across_the_bands_of_64_rows(k, e):
    c = sm.cauchy_matrix(k, e)
    todo = cc.band_pairs(k, e)
    assert len(todo) >= 8
    for _, hits in todo:
        assert agrees(c, hits) == 1
        assert pair_search(c, syndrome(c, hits))[1] == (hits[0][0], hits[1][0], hits[0][1], hits[1][1])
    if k == 245:  # three data rows of three bands: no pair
        assert agrees(c, cc.three_bands(k)[0][1]) == 0


def test_no_new_constant_and_the_header_names_the_kernel():
    assert rsgpu.CORRECT_KERNELS == {"auto": 0, "two_pass": 1, "fused": 2}
    txt = open(HEADER).read()
    got = dict(re.findall(r"^#define RSGPU_CORRECT_(\w+)\s+(\d+)\s*$", txt, re.M))
    assert {k.lower(): int(v) for k, v in got.items()} == rsgpu.CORRECT_KERNELS
    assert "k_rs_jit_correct" in txt and "k_rs_jitw_correct" in txt
    assert "generated" in rsgpu.Context.set_correct_kernel.__doc__
