"""Rebuild in place on the CPU: the numpy model of the contract
(tests/rebuild_model.py) against the oracle's general decode on consistent and
on inconsistent survivors, against the degraded model for every status of the
checked mode, the claim that a located row can always join the list, and the
hazard of tests/test_degraded.py continued to its end.  The device path is in
tests/test_gpu_rebuild.py (-m gpu); what needs no device of
rsgpu_rebuild_blocks is checked here too."""
import itertools

import numpy as np
import pytest

import degraded_model as dm
import rebuild_model as rm
import rsgpu
import scrub_model as sm
from oracle_lib import Oracle

N = dm.NONE


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def block(c, L, seed):
    """A consistent block of the e x k code c: (src, par)."""
    e, k = c.shape
    src = np.random.default_rng(seed).integers(0, 256, (k, L), dtype=np.uint8)
    return src, rm.encode(c, src)


def xor_byte(src, par, row, col, x):
    k = src.shape[0]
    if row < k:
        src[row, col] ^= x
    else:
        par[row - k, col] ^= x


def noise(src, par, rows, rng):
    """Whatever the lost rows hold."""
    k = src.shape[0]
    for r in rows:
        (src[r] if r < k else par[r - k])[:] = rng.integers(0, 256, src.shape[1], dtype=np.uint8)


def lists_of(k, e, rng):
    """Data only, parity only and mixed lists of 1, 2, 3 and e rows, the first
    and the last row of the block among them."""
    out = [[0], [k + e - 1], [0, k + e - 1], [k - 1, k]]
    for n in sorted({1, 2, 3, min(e, 5), e}):
        out.append(sorted(int(r) for r in rng.choice(k, n, replace=False)))
        out.append(sorted(int(k + p) for p in rng.choice(e, n, replace=False)))
        out.append(sorted(int(r) for r in rng.choice(k + e, n, replace=False)))
    return out


CODES = [(5, 4, "rs"), (16, 4, "rs"), (20, 7, "rs"), (64, 32, "rs"), (10, 4, "cauchy")]


@pytest.mark.parametrize("k,e,kind", CODES, ids=str)
def test_model_against_the_oracle(orc, k, e, kind):
    """The rebuilt rows are the ones ISA-L's gf_gen_decode_matrix path
    recovers, with consistent survivors and with two damaged ones (where the
    greedy pivots, the first |D| surviving parity rows, define the result)."""
    c = sm.rs_matrix(k, e) if kind == "rs" else sm.cauchy_matrix(k, e)
    enc = orc.gen_rs_matrix(k + e, k) if kind == "rs" else orc.gen_cauchy1_matrix(k + e, k)
    assert (enc[k:] == c).all()
    L = 24
    rng = np.random.default_rng(k * 100 + e)
    src, par = block(c, L, seed=k + e)
    for lost in lists_of(k, e, rng):
        surv = [r for r in range(k + e) if r not in lost]
        for damaged in (False, True):
            s2, p2 = src.copy(), par.copy()
            if damaged:
                for r in rng.choice(surv, 2, replace=False):
                    xor_byte(s2, p2, int(r), int(rng.integers(0, L)), int(rng.integers(1, 256)))
            noise(s2, p2, lost, rng)
            rc, rec = orc.decode_general(enc, list(s2) + list(p2), lost)
            assert rc == 0, lost
            q = rm.greedy_q(c, lost)
            nd = sum(r < k for r in lost)
            assert q == [p for p in range(e) if k + p not in lost][:nd]
            rep, s3, p3 = rm.call(c, s2, p2, dm.pad(lost, len(lost)), check=False)
            assert rep == (0, dm.CLEAN, -1)
            for i, r in enumerate(lost):
                got = s3[r] if r < k else p3[r - k]
                assert (got == rec[i]).all(), (lost, damaged, r)
            # nothing else moved, and consistent survivors give the original
            keep = np.ones(k + e, bool)
            keep[lost] = False
            assert (np.vstack([s3, p3])[keep] == np.vstack([s2, p2])[keep]).all()
            if not damaged:
                assert (s3 == src).all() and (p3 == par).all()


def check_block(c, src, par, s2, p2, lst):
    """The checked call on a block (s2, p2) whose original is (src, par):
    the status rules of the contract, each against the degraded model."""
    e, k = c.shape
    want = dm.report(c, s2, p2, lst)
    rep, s3, p3 = rm.call(c, s2, p2, lst, check=True)
    lost = dm.list_rows(lst, k, e)
    if want[1] in (dm.BAD_LIST, dm.BAD_MATRIX, dm.DAMAGED):
        assert rep == want and s3 is s2 and p3 is p2
    elif want[1] == dm.UNCHECKED:
        out = rm.rebuild_rows(c, s2, p2, lost)
        if out is None:
            assert rep == (0, dm.BAD_MATRIX, -1) and s3 is s2 and p3 is p2
        else:
            assert rep == want and (s3 == out[0]).all() and (p3 == out[1]).all()
    else:
        assert rep == want
        rows = lost + ([want[2]] if want[1] == dm.ONE_ROW else [])
        keep = np.ones(k + e, bool)
        keep[rows] = False
        assert (np.vstack([s3, p3])[keep] == np.vstack([s2, p2])[keep]).all()
        # the block is complete and consistent now
        assert not sm.syndromes(c, s3, p3).any()
        bad = np.vstack([s2, p2])[keep] != np.vstack([src, par])[keep]
        if not bad.any():  # all the damage lay in the rows that were rebuilt
            assert (s3 == src).all() and (p3 == par).all()
    return rep[1]


@pytest.mark.parametrize("k,e,kind", [(5, 4, "rs"), (16, 4, "rs"), (20, 7, "rs"), (10, 4, "cauchy")], ids=str)
def test_checked_mode_against_the_degraded_model(k, e, kind):
    c = sm.rs_matrix(k, e) if kind == "rs" else sm.cauchy_matrix(k, e)
    L = 16
    rng = np.random.default_rng(k)
    src, par = block(c, L, seed=3 * k)
    seen = set()
    for n in range(0, e + 1):
        for trial in range(4):
            lost = sorted(int(r) for r in rng.choice(k + e, n, replace=False))
            surv = [r for r in range(k + e) if r not in lost]
            s2, p2 = src.copy(), par.copy()
            noise(s2, p2, lost, rng)
            if trial == 1:  # one survivor, two columns
                r = int(rng.choice(surv))
                xor_byte(s2, p2, r, 0, 0x41)
                xor_byte(s2, p2, r, L - 1, 0x07)
            elif trial == 2:  # two survivors, two columns
                r1, r2 = (int(r) for r in rng.choice(surv, 2, replace=False))
                xor_byte(s2, p2, r1, 3, 0x80)
                xor_byte(s2, p2, r2, 5, 0x1D)
            elif trial == 3:  # two survivors, one column
                r1, r2 = (int(r) for r in rng.choice(surv, 2, replace=False))
                xor_byte(s2, p2, r1, 4, 0xFE)
                xor_byte(s2, p2, r2, 4, 0x02)
            seen.add(check_block(c, src, par, s2, p2, dm.pad(lost, max(1, e))))
    assert seen == {dm.CLEAN, dm.ONE_ROW, dm.DAMAGED, dm.UNCHECKED}


def test_lists_and_matrices():
    """The batch of tests/test_gpu_degraded.py test_lists_and_matrices: every
    malformation, n == e, a first parity row that is zero on D (the greedy
    pivots skip it) and a rank-deficient matrix, also with n == e."""
    k, e, L = 8, 4, 20
    c = sm.cauchy_matrix(k, e).copy()
    c[:, 5] = sm.gf_mul(c[:, 2], 0x35)  # columns 2 and 5 proportional
    c[0, 1] = c[0, 4] = 0               # parity row 0 blind to rows 1 and 4
    src, par = block(c, L, seed=9)
    lists = [[3, 3, N, N, N], [4, 2, N, N, N], [12, N, N, N, N], [N, 2, N, N, N], [0, N, 1, N, N],
             [0, 1, 2, 3, 4], [0, 1, 2, 200, N],
             [0, 1, 2, 3, N], [8, 9, 10, 11, N], [0, 3, 9, 11, N],
             [1, 4, N, N, N], [1, 4, N, N, N], [1, 4, 8, N, N], [1, 4, N, N, N],
             [2, 5, N, N, N], [2, 5, 9, N, N], [2, N, N, N, N], [5, 11, N, N, N],
             [N, N, N, N, N], [11, N, N, N, N], [0, N, N, N, N],
             [2, 5, 8, 9, N], [2, 5, 6, 7, N], [1, 4, 8, 9, N]]
    dmg = {0: (6, 5, 0x11), 7: (6, 5, 0x11), 11: (6, 10, 0x40), 12: (k + 1, 19, 0x01), 13: (k + 0, 0, 0x80),
           14: (6, 5, 0x11), 16: (7, 7, 0x07), 18: (0, 0, 0x01)}
    rng = np.random.default_rng(2)
    got = []
    for b, lst in enumerate(lists):
        s2, p2 = src.copy(), par.copy()
        noise(s2, p2, dm.list_rows(lst, k, e) or [], rng)
        if b in dmg:
            xor_byte(s2, p2, *dmg[b])
        got.append(check_block(c, src, par, s2, p2, lst))
        # the trusting call: BAD_LIST and BAD_MATRIX as the checked one
        rep, s3, p3 = rm.call(c, s2, p2, lst, check=False)
        if got[-1] in (dm.BAD_LIST, dm.BAD_MATRIX):
            assert rep[1] == got[-1] and s3 is s2 and p3 is p2
    assert got[:7] == [dm.BAD_LIST] * 7 and got[7:10] == [dm.UNCHECKED] * 3
    assert got[10] == dm.CLEAN and got[14:16] == [dm.BAD_MATRIX] * 2 and got[16] == dm.ONE_ROW
    assert rm.greedy_q(c, [1, 4]) == [1, 2] and rm.greedy_q(c, [1, 4, 8]) == [1, 2]
    # n == e: the degraded scrub says UNCHECKED, the rebuild looks at the matrix
    assert dm.report(c, src, par, lists[21])[1] == dm.UNCHECKED
    assert got[21:] == [dm.BAD_MATRIX, dm.BAD_MATRIX, dm.UNCHECKED]
    # with parity row 0 blind and rows 8, 9 lost, rows 1 and 4 hang on parity rows 2 and 3
    assert rm.greedy_q(c, [1, 4, 8, 9]) == [2, 3]


def test_a_located_row_always_joins():
    """(5, 4), every list with a spare of two rows or more, every surviving
    row damaged in turn: the report is ONE_ROW, the extended list is
    determined and the checked rebuild returns the original block."""
    k, e, L = 5, 4, 3
    c = sm.rs_matrix(k, e)
    src, par = block(c, L, seed=21)
    rng = np.random.default_rng(4)
    cases = 0
    for n in range(0, e - 1):
        for lost in itertools.combinations(range(k + e), n):
            for r in range(k + e):
                if r in lost:
                    continue
                s2, p2 = src.copy(), par.copy()
                noise(s2, p2, lost, rng)
                xor_byte(s2, p2, r, int(rng.integers(0, L)), int(rng.integers(1, 256)))
                rep, s3, p3 = rm.call(c, s2, p2, dm.pad(lost, 3), check=True)
                assert rep == (1, dm.ONE_ROW, r), (lost, r)
                assert rm.greedy_q(c, sorted(lost + (r,))) is not None
                assert (s3 == src).all() and (p3 == par).all(), (lost, r)
                cases += 1
    assert cases == 9 + 9 * 8 + 36 * 7


def test_the_hazard_closed(orc):
    """tests/test_degraded.py test_the_hazard to its end: the trusting rebuild
    seals the flipped survivor in and the scrub then blames a healthy parity
    row; the checked rebuild returns the original block where a spare of two
    rows lets it, and writes nothing where it cannot know."""
    k, e, L = 5, 4, 24
    c = sm.rs_matrix(k, e)
    src, par = block(c, L, seed=12)
    assert (np.stack(orc.encode_block(list(src), e)) == par).all()
    flipped, col = 3, 10
    bad_src = src.copy()
    bad_src[flipped, col] ^= 0x5A

    lost3 = [0, 1, 4]
    held = bad_src.copy()
    held[lost3] = 0
    rep, s3, p3 = rm.call(c, held, par, dm.pad(lost3, 4), check=False)
    assert rep == (0, dm.CLEAN, -1) and not (s3 == src).all()
    bad, status, row = sm.scrub(c, s3, p3)
    assert (bad, status) == (1, sm.ONE_ROW) and row == k + 3  # a healthy parity row is blamed
    rep, s3, p3 = rm.call(c, held, par, dm.pad(lost3, 4), check=True)
    assert rep == (1, dm.DAMAGED, -1) and s3 is held and p3 is par  # one spare row: nothing is written

    lost2 = [0, 4]
    held2 = bad_src.copy()
    held2[lost2] = 0
    rep, s3, p3 = rm.call(c, held2, par, dm.pad(lost2, 4), check=False)
    assert rep == (0, dm.CLEAN, -1) and not (s3 == src).all()
    assert sm.scrub(c, s3, p3)[1] != sm.CLEAN
    rep, s3, p3 = rm.call(c, held2, par, dm.pad(lost2, 4), check=True)
    assert rep == (1, dm.ONE_ROW, flipped)
    assert (s3 == src).all() and (p3 == par).all()
    assert sm.scrub(c, s3, p3) == (0, sm.CLEAN, -1)


def test_null_context_and_constants():
    L = rsgpu.lib()
    assert L.rsgpu_rebuild_blocks(None, 16, 4, 4096, 4096, 1, None, None, None, 1, None, 1, None) == -1
    assert rsgpu.REBUILD_CHECK == 1
    assert "rsgpu_rebuild_blocks" in rsgpu.EXPORTED_SYMBOLS
