"""Locating several damaged rows per block on the CPU: the numpy model of the
contract (tests/locate_model.py) against a brute force that enumerates spans
instead of eliminating, against the scrub's model where one row or none is
damaged, on the degenerate cases, and over random draws for the two claims of
include/rsgpu.h: never a wrong set, and rarely no set.  The device path is in
tests/test_gpu_locate.py (-m gpu); what needs no device of
rsgpu_locate_blocks is checked here too."""
import itertools

import numpy as np
import pytest

import degraded_model as dm
import locate_model as lm
import rsgpu
import scrub_model as sm

N = dm.NONE


def matrix(k, e, kind):
    return sm.rs_matrix(k, e) if kind == "rs" else sm.cauchy_matrix(k, e)


def damaged_syndromes(c, L, rows_cols, rng):
    """The syndromes (e, L) of a consistent block after every (row, columns)
    pair of rows_cols had those bytes XORed with random non-zero values."""
    syn = np.zeros((c.shape[0], L), np.uint8)
    for row, cols in rows_cols:
        syn = sm.damage(c, syn, row, cols, rng.integers(1, 256, len(cols)))
    return syn


# ---- the brute force: spans as explicit sets, no elimination anywhere --------

def pack(v):
    """Vectors of e <= 4 bytes (last axis) as integers."""
    v = np.asarray(v, np.uint32)
    return sum(v[..., i] << (8 * i) for i in range(v.shape[-1]))


def span_set(vectors):
    """Every GF(2^8) combination of at most two vectors, packed and sorted."""
    vectors = [np.asarray(v, np.uint8) for v in vectors]
    assert len(vectors) <= 2
    x = np.arange(256, dtype=np.uint8)
    if not vectors:
        return np.zeros(1, np.uint32)
    a = sm.gf_mul(vectors[0][None, :], x[:, None])
    if len(vectors) == 1:
        return np.unique(pack(a))
    b = sm.gf_mul(vectors[1][None, :], x[:, None])
    return np.unique(pack(a[:, None, :] ^ b[None, :, :]))


def dim_of(span):
    return {1: 0, 256: 1, 65536: 2}[len(span)]


def brute(c, syn):
    """The contract on a block with at most two distinct bad columns, as a
    function of u."""
    e, k = c.shape
    bad = np.flatnonzero(syn.any(axis=0))
    if len(bad) == 0:
        return lambda u: ((0, lm.CLEAN, -1), tuple([N] * u))
    w = span_set(list(np.unique(syn[:, bad], axis=1).T))
    d = dim_of(w)
    rows = [r for r in range(k + e) if pack(dm.row_column(c, r)) in w]
    ok = len(rows) == d and dim_of(span_set([dm.row_column(c, r) for r in rows])) == d

    def verdict(u):
        if not ok or d > u:
            return (len(bad), lm.DAMAGED, -1), tuple([N] * u)
        return (len(bad), lm.ONE_ROW if d == 1 else lm.ROWS, rows[0]), tuple(rows + [N] * (u - d))

    return verdict


@pytest.mark.parametrize("k,e,kind", [(4, 2, "rs"), (5, 3, "rs"), (5, 3, "cauchy")], ids=str)
def test_model_against_brute_force(k, e, kind):
    """Every row subset of at most e - 1 rows, damaged in two columns: one
    column only (all 255 values for a single row), different columns, the
    same column, both columns."""
    c = matrix(k, e, kind)
    rng = np.random.default_rng(100 * k + e)
    cases = []
    for r in range(k + e):
        for x in range(1, 256):
            cases.append(sm.damage(c, np.zeros((e, 2), np.uint8), r, [1], [x]))
    for n in range(1, e):
        for rows in itertools.combinations(range(k + e), n):
            for pattern in itertools.product(([0], [1], [0, 1]), repeat=n):
                cases.append(damaged_syndromes(c, 2, list(zip(rows, pattern)), rng))
    cases.append(np.zeros((e, 2), np.uint8))
    located = 0
    for syn in cases:
        want = brute(c, syn)
        for u in (1, 2):
            rep, lst = lm.report_syn(c, syn, u)
            assert (rep, tuple(int(x) for x in lst)) == want(u)
            located += rep[1] in (lm.ONE_ROW, lm.ROWS)
    assert located > len(cases) // 2


@pytest.mark.parametrize("kind", ["rs", "cauchy"])
@pytest.mark.parametrize("k,e", [(16, 4), (5, 4), (20, 7)], ids=str)
def test_one_row_and_clean_equal_the_scrub(k, e, kind):
    """Locatable matrices: with one damaged row or none the report is the
    scrub's with LOCATE, field by field, and the list holds the row."""
    c = matrix(k, e, kind)
    assert sm.locatable(c)
    L = 48
    rng = np.random.default_rng(k + 7 * e)
    syns = [np.zeros((e, L), np.uint8)]
    for r in range(k + e):
        cols = rng.choice(L, int(rng.integers(1, 9)), replace=False)
        syns.append(damaged_syndromes(c, L, [(r, cols)], rng))
    for syn in syns:
        for u in (1, 8):
            rep, lst = lm.report_syn(c, syn, u)
            assert rep == sm.report(c, syn, locate=True)
            want = [] if rep[1] == lm.CLEAN else [rep[2]]
            assert list(lst) == list(dm.pad(want, u))
    assert lm.report_syn(c, syns[1], 8)[0][1] == lm.ONE_ROW


@pytest.mark.parametrize("kind", ["rs", "cauchy"])
def test_two_rows_in_one_column_is_damaged(kind):
    """Two rows hit only in the same single column: W has one dimension and
    holds neither row's column."""
    c = matrix(10, 4, kind)
    rng = np.random.default_rng(3)
    for rows in ((0, 7), (3, 11), (12, 13)):
        syn = damaged_syndromes(c, 32, [(rows[0], [5]), (rows[1], [5])], rng)
        rep, lst = lm.report_syn(c, syn, 8)
        assert rep == (1, lm.DAMAGED, -1) and (lst == N).all()


def test_more_dimensions_than_u_is_damaged():
    c = matrix(10, 4, "rs")
    rng = np.random.default_rng(4)
    syn = damaged_syndromes(c, 64, [(r, rng.choice(64, 20, replace=False)) for r in (1, 6, 12)], rng)
    for u, status in ((1, lm.DAMAGED), (2, lm.DAMAGED), (3, lm.ROWS), (8, lm.ROWS)):
        rep, lst = lm.report_syn(c, syn, u)
        assert rep[1] == status
        assert list(lst) == list(dm.pad([1, 6, 12] if status == lm.ROWS else [], u))
    # e == 1: W is everything, every row is a member
    assert lm.report_syn(matrix(6, 1, "rs"), np.array([[0, 9, 0]], np.uint8), 8)[0] == (1, lm.DAMAGED, -1)
    # e == 0 and len == 0
    assert lm.report_syn(np.zeros((0, 6), np.uint8), np.zeros((0, 5), np.uint8), 8)[0] == (0, lm.CLEAN, -1)
    assert lm.report_syn(c, np.zeros((4, 0), np.uint8), 8)[0] == (0, lm.CLEAN, -1)


DRAWS = [(10, 4, "rs"), (5, 4, "rs"), (16, 8, "rs"), (20, 7, "rs"), (10, 4, "cauchy"), (6, 3, "cauchy")]


@pytest.mark.parametrize("k,e,kind", DRAWS, ids=str)
def test_never_a_wrong_set_and_rarely_none(k, e, kind):
    """1 <= n <= min(u, e - 1) rows damaged in 40 random columns of 96 each:
    every ONE_ROW / ROWS verdict names exactly the damaged rows, and at least
    90 % of the draws get one (a draw that never locates would make the first
    claim vacuous)."""
    c = matrix(k, e, kind)
    L, u, draws = 96, 8, 60
    rng = np.random.default_rng(1000 * k + e)
    located = 0
    for _ in range(draws):
        n = int(rng.integers(1, min(u, e - 1) + 1))
        rows = sorted(int(r) for r in rng.choice(k + e, n, replace=False))
        syn = damaged_syndromes(c, L, [(r, rng.choice(L, 40, replace=False)) for r in rows], rng)
        rep, lst = lm.report_syn(c, syn, u)
        assert rep[0] == np.count_nonzero(syn.any(axis=0))
        if rep[1] == lm.DAMAGED:
            assert (lst == N).all() and rep[2] == -1
            continue
        assert rep[1] == (lm.ONE_ROW if n == 1 else lm.ROWS)
        assert list(lst) == list(dm.pad(rows, u)) and rep[2] == rows[0]
        located += 1
    assert located >= 0.9 * draws, (located, draws)


def test_null_context_and_constants():
    L = rsgpu.lib()
    assert L.rsgpu_locate_blocks(None, 10, 4, 4096, 4096, 1, None, None, None, 8, None, None) == -1
    assert (rsgpu.SCRUB_ROWS, rsgpu.LOCATE_MAX_ROWS) == (4, 8)
    assert rsgpu.SCRUB_ROWS == lm.ROWS
    assert "rsgpu_locate_blocks" in rsgpu.EXPORTED_SYMBOLS
