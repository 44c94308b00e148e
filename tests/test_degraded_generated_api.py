"""The generated degraded scrub on the CPU (include/rsgpu.h
rsgpu_set_degraded_kernel, k_rs_jit_degraded): the header names the kernel
and keeps its choices, the test hook of the group size is exported by the
hooks library alone, and the lists and damage of the GPU cases
(tests/test_gpu_degraded_generated.py, which imports its parameters from
here) give, on the model alone, the statuses that the GPU test asserts, so
that the GPU comparison cannot pass on an all-clean or all-DAMAGED batch.
No torch: the draws of tests/gpu_family.py mixed_lists and damage are
repeated here, as tests/test_degraded_kernel_api.py repeats mixed_lists."""
import os
import re
import subprocess

import numpy as np
import pytest

import degraded_model as dm
import rsgpu
import scrub_model as sm
from test_degraded_kernel_api import mixed_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rsgpu.h")
N = dm.NONE
TILE = 2048
L0 = 3 * TILE + 5 * 32
B0 = 67
# one and two waves of 8 rows; 2 x 10 / 12 / 16 rows; four waves of 10 / 12 / 16; e = 3
MATRICES = [(10, 4), (11, 12), (13, 20), (13, 24), (14, 32), (9, 34), (9, 44), (8, 56), (6, 3), (12, 4), (17, 3)]
# tests/test_gpu_degraded_fused.py test_blocks_the_prepare_finishes, at (5, 4)
FINISHED_LISTS = [[1, N, N, N], [3, 1, N, N], [0, 5 + 1, N, N], [0, 1, 2, 5 + 3], [N, N, N, N], [2, N, 4, N],
                  [5 + 0, 5 + 2, N, N], [1, 2, 3, 4], [4, N, N, N]]
# bad_matrix(5, 4): columns 1 and 2 are equal, so no parity rows determine both
BAD_MATRIX_LISTS = [[0, N, N, N], [1, 2, N, N], [3, 5 + 1, N, N], [0, 1, 2, N], [1, N, N, N]]


def matrix(k, e, kind):
    return sm.rs_matrix(k, e) if kind == "rs" else sm.cauchy_matrix(k, e)


def bad_matrix(k, e):
    """The Cauchy matrix with column 2 replaced by column 1."""
    c = sm.cauchy_matrix(k, e).copy()
    c[:, 2] = c[:, 1]
    return c


def statuses_of(k, e, kind, u):
    """What mixed_lists and damage on 67 blocks must show: n = 0 is among the
    lists, so e - n >= 2 occurs and a single damaged row is named; a list of e
    rows occurs exactly when u >= e."""
    return {dm.CLEAN, dm.ONE_ROW, dm.DAMAGED} | ({dm.UNCHECKED} if u >= e else set())


def damage_hits(lost, k, e, u, L, seed=9):
    """tests/gpu_family.py damage, which writes to the device: the same draws,
    as [(block, row, column, x)]."""
    rng = np.random.default_rng(seed)
    B, nmax, hits = len(lost), min(u, e), []
    for b in range(B):
        rows = dm.list_rows(lost[b], k, e) or []
        surv = [r for r in range(k + e) if r not in rows]
        spar = [r for r in surv if r >= k]
        kind = (b // (nmax + 1)) % 7 if B > 1 else 2
        x = lambda: int(rng.integers(1, 256))  # noqa: E731
        pick = lambda n: [int(r) for r in rng.choice(surv, n, replace=False)]  # noqa: E731
        if kind == 1:
            r, col = pick(1)[0], int(rng.integers(0, L))
            hits.append((b, r, col, x()))
        elif kind == 2:
            r = pick(1)[0]
            for col in sorted({0, L - 1, L // 2, (L // 3) | 1 if L > 1 else 0, min(17, L - 1)}):
                hits.append((b, r, col, x()))
        elif kind == 3:
            r1, r2 = pick(2)
            hits.append((b, r1, 0, x()))
            hits.append((b, r2, L - 1 if L > 1 else 0, x()))
        elif kind == 4:
            r1, r2 = pick(2)
            col = int(rng.integers(0, L))
            hits.append((b, r1, col, x()))
            hits.append((b, r2, col, x()))
        elif kind == 5 and spar:
            col = int(rng.integers(0, L))
            hits.append((b, spar[0], col, x()))
        elif kind == 6 and spar:
            col = int(rng.integers(0, L))
            hits.append((b, spar[-1], col, x()))
    return hits


def model_reports(c, lost, hits, locate=True):
    """The model's reports of consistent blocks damaged by `hits`: the lost
    rows' bytes cancel out of the verdict, so the syndromes are those of the
    damage alone, and only the damaged columns (and one clean one) are kept."""
    e, k = c.shape
    out = []
    for b in range(len(lost)):
        mine = [(r, col, x) for bb, r, col, x in hits if bb == b]
        cols = sorted({col for _, col, _ in mine})
        syn = np.zeros((e, len(cols) + 1), np.uint8)
        for r, col, x in mine:
            syn[:, cols.index(col)] ^= sm.gf_mul(dm.row_column(c, r), np.uint8(x))
        out.append(dm.report_syn(c, syn, lost[b], locate))
    return out


def pivot_lists(k):
    """Eight lost data rows; parity rows 0..3 and four data rows; parity rows
    1..7 and one data row (k >= 9)."""
    return [list(range(1, 9)), [3, 4, 5, 6] + [k + p for p in range(4)], [7] + [k + p for p in range(1, 8)]]


def pivot_hits(k, e, lists):
    """Per list three blocks, one damaged byte each: in the last pivot row (a
    Cauchy matrix: the pivots are the first surviving parity rows), in the
    last parity row, in data row 0."""
    hits = []
    for i, rows in enumerate(lists):
        surv_par = [r for r in range(k, k + e) if r not in rows]
        nd = sum(r < k for r in rows)
        for j, row in enumerate((surv_par[nd - 1], k + e - 1, 0)):
            b = 3 * i + j
            hits.append((b, row, TILE + 37 * b, 0x40 + b))
    return hits


@pytest.mark.parametrize("kind", ["cauchy", "rs"])
@pytest.mark.parametrize("k,e", MATRICES, ids=str)
def test_every_layout_meets_its_statuses_on_the_model(k, e, kind):
    u = min(8, e)
    c = matrix(k, e, kind)
    lost = mixed_lists(k, e, u, B0)
    want = model_reports(c, lost, damage_hits(lost, k, e, u, L0))
    assert {w[1] for w in want} == statuses_of(k, e, kind, u)
    assert any(e - len(dm.list_rows(l, k, e)) >= 2 for l in lost)
    assert any(len(dm.list_rows(l, k, e)) == e for l in lost) == (u >= e)


@pytest.mark.parametrize("k,e", [(13, 20), (9, 44)], ids=str)
def test_pivots_across_waves_on_the_model(k, e):
    """Every block has one bad column and names the damaged row; at (13, 20),
    ten rows per wave, the eight pivots of the first list lie in one wave and
    those of the other lists in two; at (9, 44), eleven rows per wave, the
    pivots of the third list reach the second wave."""
    c = sm.cauchy_matrix(k, e)
    lists = pivot_lists(k)
    hits = pivot_hits(k, e, lists)
    lost = np.array([dm.pad(np.array(lists[b // 3]), 8) for b in range(3 * len(lists))], np.uint8)
    want = model_reports(c, lost, hits)
    assert want == [(1, dm.ONE_ROW, row) for _, row, _, _ in hits]


def test_blocks_the_prepare_finishes_on_the_model():
    k, e = 5, 4
    for c, lists, statuses in (
            (sm.cauchy_matrix(k, e), FINISHED_LISTS,
             [dm.ONE_ROW, dm.BAD_LIST, dm.ONE_ROW, dm.UNCHECKED, dm.ONE_ROW, dm.BAD_LIST, dm.ONE_ROW, dm.UNCHECKED,
              dm.ONE_ROW]),
            # block 0: the damaged row 1 and row 2 have the same column, so two rows explain it
            (bad_matrix(k, e), BAD_MATRIX_LISTS, [dm.DAMAGED, dm.BAD_MATRIX, dm.ONE_ROW, dm.BAD_MATRIX, dm.ONE_ROW])):
        lost = np.array(lists, np.uint8)
        hits = []
        for b in range(len(lists)):
            rows = dm.list_rows(lost[b], k, e) or []
            hits.append((b, next(r for r in range(k + e) if r not in rows), (517 * b) % 4160, 0x11 + b))
        assert [w[1] for w in model_reports(c, lost, hits)] == statuses


def test_the_header_names_the_kernel_and_keeps_its_choices():
    txt = open(HEADER).read()
    at = txt.index("int rsgpu_set_degraded_kernel(")
    comment = txt[txt.rindex("\n\n", 0, at):at]
    assert "k_rs_jit_degraded" in comment and "RSGPU_SCRUB_GENERATED" in comment
    assert "has no influence on these calls" not in txt
    got = dict(re.findall(r"^#define RSGPU_DEGRADED_(\w+)\s+(\d+)\s*$", txt, re.M))
    assert {k.lower(): int(v) for k, v in got.items()} == rsgpu.DEGRADED_KERNELS == {"auto": 0, "two_pass": 1, "fused": 2}
    assert rsgpu.lib().rsgpu_set_degraded_kernel(None, 3) == -1
    assert "k_rs_jit_degraded" in rsgpu.Context.set_degraded_kernel.__doc__


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.strip()}


def test_the_group_hook_is_in_the_hooks_library_only():
    assert "rsgpu_internal_set_degraded_group" in exported(rsgpu.HOOKS_PATH)
    assert "rsgpu_internal_set_degraded_group" not in exported(rsgpu.LIB_PATH)
    fn = rsgpu.testhooks().rsgpu_internal_set_degraded_group
    assert fn(None, 0) == -1
