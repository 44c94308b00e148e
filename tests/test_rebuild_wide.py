"""Rebuild in place of lists of 9 to 32 rows, on the CPU: the numpy model of the
contract (tests/rebuild_model.py, which has no cap) against the oracle's
general decode for lists of 9 to e rows, the pivots of a matrix with a blind
first parity row and a rank-deficient one at n > 8, and the rule for `u` of
include/rsgpu.h rsgpu_rebuild_blocks as a table.  The device path is in
tests/test_gpu_rebuild_wide.py (-m gpu)."""
import numpy as np
import pytest

import degraded_model as dm
import rebuild_model as rm
import rsgpu
import scrub_model as sm
from oracle_lib import Oracle
from test_rebuild import block, noise, xor_byte

N = dm.NONE


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def u_accepted(e, u, check):
    """include/rsgpu.h: 1 <= u <= 7 with RSGPU_REBUILD_CHECK, otherwise
    1 <= u <= max(8, min(e, RSGPU_REBUILD_MAX_LOST))."""
    return 1 <= u <= (7 if check else max(8, min(e, rsgpu.REBUILD_MAX_LOST)))


# (e, u, check) -> accepted
U_RULE = [
    (12, 1, False, True), (12, 8, False, True), (12, 9, False, True), (12, 12, False, True),
    (12, 13, False, False), (12, 0, False, False),
    (4, 8, False, True), (4, 9, False, False),      # today's range stays, and its end
    (0, 8, False, True), (0, 9, False, False),
    (32, 32, False, True), (32, 33, False, False),
    (40, 32, False, True), (40, 33, False, False),  # the cap, whatever e
    (12, 7, True, True), (12, 8, True, False), (12, 9, True, False), (12, 12, True, False),
    (32, 32, True, False), (4, 7, True, True), (4, 0, True, False),
]


def test_the_rule_for_u():
    assert rsgpu.REBUILD_MAX_LOST == 32
    for e, u, check, ok in U_RULE:
        assert u_accepted(e, u, check) == ok, (e, u, check)
    assert rsgpu.REBUILD_KERNELS == {"auto": 0, "lanes": 1, "threaded": 2}
    assert "rsgpu_set_rebuild_kernel" in rsgpu.EXPORTED_SYMBOLS
    assert rsgpu.lib().rsgpu_set_rebuild_kernel(None, 0) == -1


def wide_lists(k, e, rng):
    """Lists of 9 .. e rows: every length once as a mix of data and parity
    rows; all data rows and all parity rows at 9 and at e (where k allows)."""
    out = []
    for n in range(9, e + 1):
        out.append(sorted(int(r) for r in rng.choice(k + e, n, replace=False)))
    for n in (9, e):
        if n <= k:
            out.append(sorted(int(r) for r in rng.choice(k, n, replace=False)))
        out.append(sorted(int(k + p) for p in rng.choice(e, n, replace=False)))
    return out


# the seed of the rs code's lists is chosen so that every drawn list has the
# first |D| surviving parity rows as its pivots (asserted below for all codes:
# no list is left out)
CODES = [(20, 12, "cauchy", 1), (64, 32, "cauchy", 2), (20, 12, "rs", 3)]


@pytest.mark.parametrize("k,e,kind,seed", CODES, ids=str)
def test_model_against_the_oracle(orc, k, e, kind, seed):
    c = sm.rs_matrix(k, e) if kind == "rs" else sm.cauchy_matrix(k, e)
    enc = orc.gen_rs_matrix(k + e, k) if kind == "rs" else orc.gen_cauchy1_matrix(k + e, k)
    assert (enc[k:] == c).all()
    L = 24
    rng = np.random.default_rng(seed)
    src, par = block(c, L, seed=k + e)
    lists = wide_lists(k, e, rng)
    assert {len(lost) for lost in lists} == set(range(9, e + 1))
    for lost in lists:
        surv = [r for r in range(k + e) if r not in lost]
        nd = sum(r < k for r in lost)
        assert rm.greedy_q(c, lost) == [p for p in range(e) if k + p not in lost][:nd], lost
        for damaged in (False, True):
            s2, p2 = src.copy(), par.copy()
            if damaged:
                for r in rng.choice(surv, 2, replace=False):
                    xor_byte(s2, p2, int(r), int(rng.integers(0, L)), int(rng.integers(1, 256)))
            noise(s2, p2, lost, rng)
            rc, rec = orc.decode_general(enc, list(s2) + list(p2), lost)
            assert rc == 0, lost
            rep, s3, p3 = rm.call(c, s2, p2, dm.pad(lost, len(lost)), check=False)
            assert rep == (0, dm.CLEAN, -1)
            for i, r in enumerate(lost):
                got = s3[r] if r < k else p3[r - k]
                assert (got == rec[i]).all(), (lost, damaged, r)
            keep = np.ones(k + e, bool)
            keep[lost] = False
            assert (np.vstack([s3, p3])[keep] == np.vstack([s2, p2])[keep]).all()
            if not damaged:
                assert (s3 == src).all() and (p3 == par).all()


def custom_matrix(k=20, e=12):
    """Cauchy with parity row 0 blind to rows 1, 4, 6 .. 13 and columns 2 and
    5 proportional: what tests/test_rebuild.py's matrix does at (8, 4), for
    lists of more than 8 rows."""
    c = sm.cauchy_matrix(k, e).copy()
    c[:, 5] = sm.gf_mul(c[:, 2], 0x35)
    c[0, [1, 4] + list(range(6, 14))] = 0
    return c


BLIND = [1, 4, 6, 7, 8, 9, 10, 11, 12, 13]          # 10 data rows parity row 0 does not see
BLIND_AND_PARITY = BLIND[:9] + [20 + 3, 20 + 11]    # two parity rows among them: Q is every useful row left
BLIND_SHORT = BLIND + [20 + 3, 20 + 11]             # n == e, and one of the 10 rows left is the blind one
DEFICIENT = [2, 5, 6, 7, 8, 9, 10, 11, 12]          # rows 2 and 5 cannot be told apart
DEFICIENT_FULL = [0, 2, 3, 5] + list(range(24, 32))  # the same with n == e


def test_custom_matrix_at_more_than_eight_rows():
    k, e, L = 20, 12, 20
    c = custom_matrix(k, e)
    src, par = block(c, L, seed=5)
    rng = np.random.default_rng(8)
    # parity row 0 is zero on all of D: the pivots skip it
    assert rm.greedy_q(c, BLIND) == list(range(1, 11))
    assert rm.greedy_q(c, BLIND_AND_PARITY) == [1, 2, 4, 5, 6, 7, 8, 9, 10]
    for lost in (BLIND, BLIND_AND_PARITY):
        s2, p2 = src.copy(), par.copy()
        noise(s2, p2, lost, rng)
        rep, s3, p3 = rm.call(c, s2, p2, dm.pad(lost, e), check=False)
        assert rep == (0, dm.CLEAN, -1) and (s3 == src).all() and (p3 == par).all()
    # BAD_MATRIX, also judged at n == e, where the degraded scrub looks at no matrix
    assert len(DEFICIENT_FULL) == e
    assert len(BLIND_SHORT) == e
    for lost in (DEFICIENT, DEFICIENT_FULL, BLIND_SHORT):
        assert rm.greedy_q(c, lost) is None
        s2, p2 = src.copy(), par.copy()
        noise(s2, p2, lost, rng)
        rep, s3, p3 = rm.call(c, s2, p2, dm.pad(lost, e), check=False)
        assert rep == (0, dm.BAD_MATRIX, -1) and s3 is s2 and p3 is p2
    assert dm.report(c, src, par, dm.pad(DEFICIENT_FULL, e))[1] == dm.UNCHECKED
    # n > e is a malformed list
    rep, s3, p3 = rm.call(c, src, par, dm.pad(list(range(13)), 13), check=False)
    assert rep == (0, dm.BAD_LIST, -1) and s3 is src
