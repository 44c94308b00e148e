"""Correction per byte column on the CPU: the numpy model of the contract
(correct_model.py) against the repair's model, the properties the header
states, the damage the GPU suite injects (correct_cases.py) on every
gf_gen_rs_matrix shape it uses, and what of rsgpu_correct_blocks needs no
device.  The device path is in tests/test_gpu_correct.py (-m gpu)."""
import numpy as np
import pytest

import correct_cases as cc
import correct_model as cm
import repair_model as rm
import rsgpu
import scrub_model as sm


def matrix(k, e, kind):
    return sm.rs_matrix(k, e) if kind == "rs" else sm.cauchy_matrix(k, e)


def codeword(c, L, seed):
    """A consistent block of random data: (src, par)."""
    e, k = c.shape
    src = np.random.default_rng(seed).integers(0, 256, (k, L), dtype=np.uint8)
    return src, sm.syndromes(c, src, np.zeros((e, L), np.uint8))


def hit(src, par, row, col, x):
    k = src.shape[0]
    if row < k:
        src[row, col] ^= x
    else:
        par[row - k, col] ^= x


def damaged(c, L, block, seed=5):
    k = c.shape[1]
    src, par = codeword(c, L, seed)
    s1, p1 = src.copy(), par.copy()
    todo = cc.plan(k, c.shape[0], L, block)
    for _, col, hits in todo:
        for row, x in hits:
            hit(s1, p1, row, col, x)
    return src, par, s1, p1, todo


@pytest.mark.parametrize("k,e,kind", [(6, 5, "cauchy"), (16, 8, "rs"), (20, 7, "rs"), (10, 3, "rs")], ids=str)
def test_t1_is_the_repairs_columns_mode(k, e, kind):
    c = matrix(k, e, kind)
    if e >= 5:
        _, _, s1, p1, _ = damaged(c, 4113, 0)
    else:
        src, par = codeword(c, 300, 1)
        s1, p1 = src.copy(), par.copy()
        for row, col, x in [(0, 0, 1), (k, 7, 2), (3, 9, 3), (4, 9, 4), (k + 1, 299, 0xFF), (2, 299, 0x80)]:
            hit(s1, p1, row, col, x)
    s2, p2, (bad, corrected, two, status, row) = cm.correct(c, s1, p1, 1)
    r2, q2, want = rm.repair(c, s1, p1, "columns")
    assert (s2 == r2).all() and (p2 == q2).all()
    assert (bad, corrected, status, row) == want and two == 0 and 0 < corrected < bad


@pytest.mark.parametrize("k,e,kind", cc.SHAPES, ids=str)
def test_t2_corrects_what_columns_corrects_and_the_planned_pairs(k, e, kind):
    """Every shape of the GPU suite, gf_gen_rs_matrix (not MDS in general)
    included: each planned one- and two-row column comes back byte for byte,
    the columns COLUMNS corrects are corrected identically, and a second pass
    finds what the first one left."""
    c = matrix(k, e, kind)
    L = 4113
    for block in range(cc.BLOCKS):
        src, par, s1, p1, todo = damaged(c, L, block)
        s2, p2, (bad, corrected, two, status, row) = cm.correct(c, s1, p1, 2)
        r2, q2, (_, repaired, _, _) = rm.repair(c, s1, p1, "columns")
        for kind_, col, hits in todo:
            if kind_ != "three":
                assert (s2[:, col] == src[:, col]).all() and (p2[:, col] == par[:, col]).all(), (block, kind_, col)
            if kind_ == "one":
                assert (r2[:, col] == src[:, col]).all() and (q2[:, col] == par[:, col]).all()
        ones = sum(kind_ == "one" for kind_, _, _ in todo)
        pairs = sum(kind_ not in ("one", "three") for kind_, _, _ in todo)
        assert bad == len(todo) and repaired == ones and corrected >= ones + pairs and two == corrected - ones
        assert row == -1 and status == (cm.REPAIRED if corrected == bad else cm.PARTIAL)
        again = cm.correct(c, s2, p2, 2)[2]
        assert again[0] == bad - corrected and again[1] == 0


@pytest.mark.parametrize("k,e", [(6, 5), (12, 6), (8, 64)], ids=str)
def test_three_rows_of_a_cauchy_code_are_left_alone(k, e):
    """Any 5 columns of [C | I] of a Cauchy matrix are independent, so with
    e >= 5 no pair (and no row) explains a column damaged in three rows."""
    c = sm.cauchy_matrix(k, e)
    src, par = codeword(c, 64, 3)
    rng = np.random.default_rng(k)
    s1, p1 = src.copy(), par.copy()
    for col in range(0, 64, 4):
        for row in rng.choice(k + e, 3, replace=False):
            hit(s1, p1, int(row), col, int(rng.integers(1, 256)))
    for t in (1, 2):
        s2, p2, verdict = cm.correct(c, s1, p1, t)
        assert verdict == (16, 0, 0, cm.DAMAGED, -1) and (s2 == s1).all() and (p2 == p1).all()


def test_one_row_corrections_in_one_row_name_it():
    c = sm.cauchy_matrix(12, 6)
    src, par = codeword(c, 50, 4)
    s1, p1 = src.copy(), par.copy()
    hit(s1, p1, 7, 3, 0x55)
    hit(s1, p1, 7, 40, 0x01)
    s2, p2, verdict = cm.correct(c, s1, p1, 2)
    assert verdict == (2, 2, 0, cm.REPAIRED, 7) and (s2 == src).all() and (p2 == par).all()
    # a two-row correction beside them: no common row
    hit(s1, p1, 7, 9, 0x10)
    hit(s1, p1, 13, 9, 0x20)
    s2, p2, verdict = cm.correct(c, s1, p1, 2)
    assert verdict == (3, 3, 1, cm.REPAIRED, -1) and (s2 == src).all() and (p2 == par).all()
    assert cm.correct(c, s1, p1, 1)[2] == (3, 2, 0, cm.PARTIAL, 7)


def test_scattered_damage_is_corrected():
    """The case the call exists for: damage in 12 rows, two per column."""
    for k, e, kind in [(12, 6, "cauchy"), (20, 7, "rs"), (64, 32, "rs"), (245, 5, "cauchy"), (100, 20, "rs")]:
        c = matrix(k, e, kind)
        src, par = codeword(c, 256, 8)
        s1, p1 = src.copy(), par.copy()
        for col, hits in cc.scattered(k, e, 256):
            for row, x in hits:
                hit(s1, p1, row, col, x)
        s2, p2, verdict = cm.correct(c, s1, p1, 2)
        assert verdict == (12, 12, 12, cm.REPAIRED, -1) and (s2 == src).all() and (p2 == par).all()


@pytest.mark.parametrize("k,e,kind", cc.BAND_SHAPES, ids=str)
def test_pairs_across_bands_are_two_row_corrections(k, e, kind):
    """What tests/test_gpu_correct.py test_pairs_across_bands relies on: every
    column of band_pairs is a two-row correction of exactly its pair and the
    block comes back as the codeword; t = 1 leaves every byte; a second pass
    finds nothing."""
    c = matrix(k, e, kind)
    src, par = codeword(c, 4128, 2)
    s1, p1 = src.copy(), par.copy()
    todo = cc.band_pairs(k, e)
    assert len(todo) == (17 if k > 192 else 14 if k > 128 else 11)
    assert any(a < k and b < k and a // 64 != b // 64 for _, ((a, _), (b, _)) in todo)
    for col, hits in todo:
        for row, x in hits:
            hit(s1, p1, row, col, x)
    syn = sm.syndromes(c, s1, p1)
    for col, hits in todo:
        assert cm.verdict(c, syn[:, col], 2) == hits, (col, hits)
    s2, p2, verdict = cm.correct(c, s1, p1, 2)
    assert verdict == (len(todo), len(todo), len(todo), cm.REPAIRED, -1)
    assert (s2 == src).all() and (p2 == par).all()
    s3, p3, verdict = cm.correct(c, s1, p1, 1)
    assert verdict == (len(todo), 0, 0, cm.DAMAGED, -1) and (s3 == s1).all() and (p3 == p1).all()
    assert cm.correct(c, s2, p2, 2)[2] == (0, 0, 0, cm.CLEAN, -1)


def test_three_rows_of_three_bands_are_left_alone():
    """(245, 5) Cauchy, distance 6: the column damaged in rows of three
    different bands stays byte for byte, the one beside it in row 244 alone
    is corrected."""
    k, e = 245, 5
    c = sm.cauchy_matrix(k, e)
    src, par = codeword(c, 4128, 3)
    s1, p1 = src.copy(), par.copy()
    (col3, hits3), (col1, hits1) = cc.three_bands(k)
    assert len({r // 64 for r, _ in hits3}) == 3 and hits1[0][0] == 244
    for col, hits in ((col3, hits3), (col1, hits1)):
        for row, x in hits:
            hit(s1, p1, row, col, x)
    s2, p2, verdict = cm.correct(c, s1, p1, 2)
    assert verdict == (2, 1, 0, cm.PARTIAL, 244)
    assert (s2[:, col3] == s1[:, col3]).all() and (s2[:, col1] == src[:, col1]).all() and (p2 == p1).all()


def test_two_matching_pairs_leave_the_column_alone():
    """Ambiguity is decided per column, by the definition: with four dependent
    columns of [C | I] the columns in their common line stay as they are."""
    c = cc.dependent_matrix()
    src, par = codeword(c, 2100, 6)
    s1, p1 = src.copy(), par.copy()
    for col, hits in cc.AMBIGUOUS + cc.UNIQUE:
        for row, x in hits:
            hit(s1, p1, row, col, x)
    s2, p2, verdict = cm.correct(c, s1, p1, 2)
    assert verdict == (6, 1, 1, cm.PARTIAL, -1)
    for col, hits in cc.UNIQUE:
        for row, x in hits:
            hit(s1, p1, row, col, x)
    assert (s2 == s1).all() and (p2 == p1).all()


def test_two_matching_pairs_in_different_bands():
    """The same at (129, 7) with the two pairs in one 64-row band, in two
    neighbouring ones and in the last, one-row band: each ambiguous column has
    exactly its two pairs and stays as it is, the two beside them come back."""
    c = cc.dependent_wide_matrix()
    src, par = codeword(c, 2100, 7)
    s1, p1 = src.copy(), par.copy()
    for col, hits in cc.AMBIGUOUS_WIDE + cc.UNIQUE_WIDE:
        for row, x in hits:
            hit(s1, p1, row, col, x)
    syn = sm.syndromes(c, s1, p1)
    bands = set()
    for col, _ in cc.AMBIGUOUS_WIDE:
        pairs = {(a, b) for a, b, _, _ in cm.explaining_pairs(c, syn[:, col])}
        assert len(pairs) == 2 and not sm.explaining_rows(c, syn[:, col]), (col, pairs)
        bands.add(tuple(sorted(b // 64 for _, b in pairs)))
    assert bands == {(0, 0), (0, 1), (1, 2)}
    s2, p2, verdict = cm.correct(c, s1, p1, 2)
    n = len(cc.AMBIGUOUS_WIDE)
    assert verdict == (n + 2, 2, 2, cm.PARTIAL, -1)
    for col, hits in cc.UNIQUE_WIDE:
        for row, x in hits:
            hit(s1, p1, row, col, x)
    assert (s2 == s1).all() and (p2 == p1).all()


def test_argument_rules_of_the_model():
    for c, t in [(sm.cauchy_matrix(6, 4), 2), (sm.cauchy_matrix(6, 2), 1), (sm.cauchy_matrix(6, 5), 0),
                 (sm.cauchy_matrix(6, 5), 3), (sm.cauchy_matrix(4, 65), 2), (np.ones((5, 4), np.uint8), 2)]:
        with pytest.raises(ValueError):
            cm.correct(c, np.zeros((c.shape[1], 4), np.uint8), np.zeros((c.shape[0], 4), np.uint8), t)
    assert cm.supported(sm.cauchy_matrix(4, 65), 1) and cm.supported(sm.cauchy_matrix(6, 4), 1)


def test_correct_blocks_null_context_is_an_argument_error():
    L = rsgpu.lib()
    assert L.rsgpu_correct_blocks(None, 16, 8, 4096, 4096, 1, None, None, None, 2, None) == -1


def test_report_dtype_is_the_headers_struct():
    dt = rsgpu.CORRECT_REPORT_DTYPE
    assert dt.itemsize == 32
    assert [(n, dt.fields[n][0].str, dt.fields[n][1]) for n in dt.names] == [
        ("bad_columns", "<u8", 0), ("corrected_columns", "<u8", 8), ("two_row_columns", "<u8", 16),
        ("status", "<i4", 24), ("row", "<i4", 28)]
    assert (cm.CLEAN, cm.REPAIRED, cm.PARTIAL, cm.DAMAGED) == (
        rsgpu.REPAIR_CLEAN, rsgpu.REPAIR_REPAIRED, rsgpu.REPAIR_PARTIAL, rsgpu.REPAIR_DAMAGED)
