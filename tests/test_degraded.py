"""Degraded scrub on the CPU: the numpy model of the contract
(tests/degraded_model.py) against brute force over every choice of the lost
bytes, its independence from what the lost rows hold, the all-NONE identity
with the scrub's model, the list and matrix verdicts, and the hazard the call
exists for (a rebuild that folds a bad survivor in, then a scrub that names a
healthy parity row).  The device path is in tests/test_gpu_degraded.py (-m gpu);
what needs no device of rsgpu_scrub_degraded_blocks is checked here too."""
import itertools

import numpy as np
import pytest

import degraded_model as dm
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
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (k, L), dtype=np.uint8)
    par = np.zeros((e, L), np.uint8)
    for j in range(k):
        par ^= sm.gf_mul(c[:, j][:, None], src[j][None, :])
    return src, par


def xor_byte(src, par, row, col, x):
    k = src.shape[0]
    if row < k:
        src[row, col] ^= x
    else:
        par[row - k, col] ^= x


def pack(s):
    """Syndrome columns (e, N), e <= 3, as integers."""
    out = np.zeros(s.shape[1], np.int64)
    for p in range(s.shape[0]):
        out |= s[p].astype(np.int64) << (8 * p)
    return out


def brute_span(c, lost):
    """What the lost rows can add to the syndromes: the set of A x over ALL
    256^n choices x of the lost bytes, as a membership table over the packed
    syndromes.  A column is consistent exactly when its syndromes (taken with
    zero lost bytes) are in the set."""
    e, k = c.shape
    table = np.zeros(1 << (8 * e), bool)
    n = len(lost)
    choices = ((np.arange(256 ** n)[:, None] >> (8 * np.arange(n))[None, :]) & 255).astype(np.uint8)
    s = np.zeros((e, len(choices)), np.uint8)
    for n, r in enumerate(lost):
        s ^= sm.gf_mul(dm.row_column(c, r)[:, None], choices[:, n][None, :])
    table[pack(s)] = True
    return table


def brute_report(c, syn, lost, span, locate=True):
    """The contract by exhaustion: consistency by membership in span =
    brute_span(c, lost), "explains" by trying every surviving row and every
    x != 0."""
    e, k = c.shape
    bad = np.flatnonzero(~span[pack(syn)])
    if len(bad) == 0:
        return 0, dm.CLEAN, -1
    if not locate:
        return len(bad), dm.DAMAGED, -1
    x = np.arange(1, 256, dtype=np.uint8)
    seen = set()
    for i in bad:
        rows = [r for r in range(k + e) if r not in lost and
                span[pack(syn[:, i][:, None] ^ sm.gf_mul(dm.row_column(c, r)[:, None], x[None, :]))].any()]
        if len(rows) != 1:
            return len(bad), dm.DAMAGED, -1
        seen.add(rows[0])
    return (len(bad), dm.ONE_ROW, seen.pop()) if len(seen) == 1 else (len(bad), dm.DAMAGED, -1)


@pytest.mark.parametrize("k,e,kind", [(4, 2, "rs"), (5, 3, "rs"), (5, 3, "cauchy")], ids=str)
def test_model_against_brute_force(k, e, kind):
    """Every lost set of n <= 2 rows (n < e), a clean block and blocks with
    one, two and three damaged survivors: the model's report is the one that
    exhausting all 256^n lost-byte choices gives."""
    c = sm.rs_matrix(k, e) if kind == "rs" else sm.cauchy_matrix(k, e)
    L = 12
    src, par = block(c, L, seed=k * 10 + e)
    rng = np.random.default_rng(3)
    statuses = set()
    for n in range(0, min(2, e - 1) + 1):
        for lost in itertools.combinations(range(k + e), n):
            surv = [r for r in range(k + e) if r not in lost]
            span = brute_span(c, lost)
            for case in range(5):
                s2, p2 = src.copy(), par.copy()
                for r in lost:  # whatever the lost rows hold
                    for col in range(L):
                        xor_byte(s2, p2, r, col, int(rng.integers(0, 256)))
                if case == 1:  # one survivor, two columns
                    xor_byte(s2, p2, surv[case % len(surv)], 0, 0x41)
                    xor_byte(s2, p2, surv[case % len(surv)], L - 1, 0x07)
                elif case == 2:  # two survivors, two columns
                    xor_byte(s2, p2, surv[0], 3, 0x80)
                    xor_byte(s2, p2, surv[-1], 5, 0x1D)
                elif case == 3:  # two survivors, one column
                    xor_byte(s2, p2, surv[1], 4, 0xFE)
                    xor_byte(s2, p2, surv[-2], 4, 0x02)
                elif case == 4:  # three survivors, one column
                    for r in rng.choice(surv, 3, replace=False):
                        xor_byte(s2, p2, int(r), 7, int(rng.integers(1, 256)))
                syn = sm.syndromes(c, s2, p2)
                # the span is taken from zero lost bytes: fold the stored ones out
                syn0 = syn.copy()
                for r in lost:
                    row = s2[r] if r < k else p2[r - k]
                    syn0 ^= sm.gf_mul(dm.row_column(c, r)[:, None], row[None, :])
                for locate in (True, False):
                    want = brute_report(c, syn0, lost, span, locate)
                    got = dm.report(c, s2, p2, dm.pad(lost, 2), locate)
                    assert got == want, (lost, case, locate)
                    statuses.add(got[1])
    assert {dm.CLEAN, dm.DAMAGED} <= statuses
    if e >= 3:
        assert dm.ONE_ROW in statuses


def test_model_ignores_what_the_lost_rows_hold():
    c = sm.rs_matrix(16, 4)
    k, e, L = 16, 4, 40
    src, par = block(c, L, seed=5)
    xor_byte(src, par, 7, 11, 0x33)
    xor_byte(src, par, 7, 39, 0x01)
    lst = dm.pad([2, k + 1], 4)
    want = dm.report(c, src, par, lst)
    assert want == (2, dm.ONE_ROW, 7)
    rng = np.random.default_rng(8)
    for _ in range(3):
        s2, p2 = src.copy(), par.copy()
        s2[2] = rng.integers(0, 256, L, dtype=np.uint8)
        p2[1] = rng.integers(0, 256, L, dtype=np.uint8)
        assert dm.report(c, s2, p2, lst) == want
        assert dm.report(c, s2, p2, lst, locate=False) == (2, dm.DAMAGED, -1)


@pytest.mark.parametrize("kind", ["rs", "cauchy"])
@pytest.mark.parametrize("k,e", [(16, 4), (5, 4), (20, 7)], ids=str)
def test_all_none_is_the_scrub(kind, k, e):
    c = sm.rs_matrix(k, e) if kind == "rs" else sm.cauchy_matrix(k, e)
    L = 33
    src, par = block(c, L, seed=k)
    cases = [[], [(0, 0, 0x01)], [(k - 1, 5, 0x10), (k - 1, L - 1, 0xFF)], [(k, 2, 0x55)],
             [(k + e - 1, 32, 0x80)], [(1, 3, 0x11), (k + 1, 9, 0x22)], [(1, 3, 0x11), (2, 3, 0x22)]]
    for dmg in cases:
        s2, p2 = src.copy(), par.copy()
        for row, col, x in dmg:
            xor_byte(s2, p2, row, col, x)
        for locate in (True, False):
            assert dm.report(c, s2, p2, [N, N], locate) == sm.scrub(c, s2, p2, locate), dmg


def test_malformed_lists():
    c = sm.rs_matrix(5, 4)
    src, par = block(c, 8, seed=1)
    for lst in ([3, 3, N, N], [4, 2, N, N], [9, N, N, N], [N, 2, N, N], [0, N, 1, N], [0, 1, 2, 200],
                [0, 1, 2, 3, 4]):
        assert dm.report(c, src, par, lst) == (0, dm.BAD_LIST, -1), lst
    # the last row and a full list are well formed
    assert dm.report(c, src, par, [8, N, N, N]) == (0, dm.CLEAN, -1)
    assert dm.report(c, src, par, [0, 1, 2, N]) == (0, dm.CLEAN, -1)
    # e == 0 and len == 0: CLEAN, but a malformed list stays BAD_LIST
    c0 = np.zeros((0, 5), np.uint8)
    assert dm.report(c0, src, np.zeros((0, 8), np.uint8), [N, N]) == (0, dm.CLEAN, -1)
    assert dm.report(c0, src, np.zeros((0, 8), np.uint8), [0, N]) == (0, dm.BAD_LIST, -1)
    assert dm.report(c, src[:, :0], par[:, :0], [0, 1, 2, 3]) == (0, dm.CLEAN, -1)
    assert dm.report(c, src[:, :0], par[:, :0], [1, 0, N, N]) == (0, dm.BAD_LIST, -1)


def test_no_spare_row_is_unchecked():
    c = sm.rs_matrix(5, 4)
    src, par = block(c, 8, seed=2)
    xor_byte(src, par, 4, 1, 0x77)  # damage nobody can see
    for lst in ([0, 1, 2, 3], [5, 6, 7, 8], [0, 3, 6, 8]):
        assert dm.report(c, src, par, lst) == (0, dm.UNCHECKED, -1)


def test_first_parity_row_blind_to_the_lost_rows():
    """c[0] is zero on D: a greedy choice of pivot rows has to skip parity row
    0, and the verdicts are what they are for any valid choice."""
    k, e, L = 6, 4, 16
    c = sm.cauchy_matrix(k, e).copy()
    c[0, 1] = c[0, 4] = 0
    src, par = block(c, L, seed=4)
    lst = dm.pad([1, 4], 2)
    assert dm.determined(c, [1, 4])
    assert dm.report(c, src, par, lst) == (0, dm.CLEAN, -1)
    s2, p2 = src.copy(), par.copy()
    xor_byte(s2, p2, 3, 9, 0x21)
    got = dm.report(c, s2, p2, lst)
    assert got[0] == 1 and got[1] in (dm.ONE_ROW, dm.DAMAGED)
    assert got == brute_free(c, s2, p2, [1, 4])
    # parity row 0 sees none of D: damage in it is its own business
    s2, p2 = src.copy(), par.copy()
    xor_byte(s2, p2, k, 2, 0x05)
    assert dm.report(c, s2, p2, lst) == brute_free(c, s2, p2, [1, 4])


def brute_free(c, src, par, lost):
    """A second, slower statement of the contract for codes with e > 3:
    "explains" by the rank of [A | s ^ x g_r] for every x, one at a time."""
    e, k = c.shape
    a = np.stack([dm.row_column(c, r) for r in lost], axis=1)
    ra = dm.rank(a)
    syn = sm.syndromes(c, src, par)
    bad = [i for i in range(syn.shape[1]) if dm.rank(np.column_stack([a, syn[:, i]])) != ra]
    if not bad:
        return 0, dm.CLEAN, -1
    seen = set()
    for i in bad:
        rows = []
        for r in range(k + e):
            if r in lost:
                continue
            g = dm.row_column(c, r)
            if any(dm.rank(np.column_stack([a, syn[:, i] ^ sm.gf_mul(g, x)])) == ra for x in range(1, 256)):
                rows.append(r)
        if len(rows) != 1:
            return len(bad), dm.DAMAGED, -1
        seen.add(rows[0])
    return (len(bad), dm.ONE_ROW, seen.pop()) if len(seen) == 1 else (len(bad), dm.DAMAGED, -1)


def test_rank_deficient_matrix():
    """Columns 2 and 5 of c are proportional: lost together, no parity rows
    determine them.  Lost one at a time they are fine."""
    k, e, L = 8, 4, 8
    c = sm.cauchy_matrix(k, e).copy()
    c[:, 5] = sm.gf_mul(c[:, 2], 0x35)
    src, par = block(c, L, seed=6)
    assert dm.report(c, src, par, [2, 5, N]) == (0, dm.BAD_MATRIX, -1)
    assert dm.report(c, src, par, [2, 5, k + 1]) == (0, dm.BAD_MATRIX, -1)
    assert dm.report(c, src, par, [2, N, N]) == (0, dm.CLEAN, -1)
    # the definition itself: no |D| surviving parity rows give an invertible c[p][D]
    for lost in ([2, 5], [2, 5, k + 1], [2], [0, 1, 3]):
        d = [r for r in lost if r < k]
        surv = [p for p in range(e) if k + p not in lost]
        some = any(dm.rank(c[np.ix_(q, d)]) == len(d) for q in itertools.combinations(surv, len(d)))
        assert dm.determined(c, lost) is some, lost
    # malformed beats everything, n == e beats the matrix
    assert dm.report(c, src, par, [5, 2, N])[1] == dm.BAD_LIST
    assert dm.report(c, src, par, [2, 5, 6, 7])[1] == dm.UNCHECKED


def test_the_hazard(orc):
    """Why the call exists.  (5, 4), three data rows lost, one byte of a
    surviving row flipped.  The rebuild trusts the survivor; afterwards the
    complete block looks like ONE damaged parity row -- the one spare row the
    decoder did not use -- and a repair would seal the wrong data in.  The
    degraded scrub, asked BEFORE the rebuild, says DAMAGED (one spare row
    cannot locate); with only two rows lost it names the flipped survivor."""
    k, e, L = 5, 4, 24
    c = sm.rs_matrix(k, e)
    enc = orc.gen_rs_matrix(k + e, k)
    assert (enc[k:] == c).all()
    src, par = block(c, L, seed=12)
    assert (np.stack(orc.encode_block(list(src), e)) == par).all()
    flipped, col = 3, 10
    bad_src = src.copy()
    bad_src[flipped, col] ^= 0x5A

    lost3 = [0, 1, 4]
    held = bad_src.copy()
    held[lost3] = 0  # the lost rows hold nothing
    rc, rec = orc.decode_general(enc, list(held) + list(par), lost3)
    assert rc == 0
    rebuilt = held.copy()
    for i, r in enumerate(lost3):
        rebuilt[r] = rec[i]
    assert not (rebuilt == src).all()  # the flip went into the rebuilt rows
    bad, status, row = sm.scrub(c, rebuilt, par)
    assert (bad, status) == (1, sm.ONE_ROW) and row == k + 3  # a healthy parity row is blamed
    # asked before the rebuild
    assert dm.report(c, held, par, dm.pad(lost3, 4)) == (1, dm.DAMAGED, -1)
    assert dm.report(c, held, par, dm.pad(lost3, 4), locate=False) == (1, dm.DAMAGED, -1)
    lost2 = [0, 4]
    held2 = bad_src.copy()
    held2[lost2] = 0
    assert dm.report(c, held2, par, dm.pad(lost2, 4)) == (1, dm.ONE_ROW, flipped)
    # and the way out: the named row joins the erasure list
    rc, rec = orc.decode_general(enc, list(held2) + list(par), [0, flipped, 4])
    assert rc == 0
    assert all((rec[i] == src[r]).all() for i, r in enumerate([0, flipped, 4]))


def test_lists_and_damage_of_the_wide_cases():
    """What the GPU suites take for granted at more than 64 source (or parity)
    rows, tests/gpu_family.py WIDE_CASES: band_lists gives blocks 2..5 lists
    of min(u, e) - 1 ascending rows around the edges of the 64-row bands which
    between them hold every such row of the shape, and the model calls the two
    deliberately damaged blocks of wide_plan ONE_ROW, in a row of the second
    band or above (a parity row from k + 64 on at (9, 70)), and DAMAGED; with
    the lists of the checked rebuild (u <= 7) as well."""
    pytest.importorskip("torch")
    import gpu_family as gf
    assert [(k, e) for k, e, *_ in gf.WIDE_CASES] == [(65, 6), (100, 20), (129, 9), (213, 37), (245, 5), (9, 70)]
    for k, e, kind, L, B, u, mode in gf.WIDE_CASES:
        assert k + e <= 250 and max(k, e) > 64
        pool = {63, 64, 65, 127, 128, 129, 191, 192, k - 1, k, k + 63, k + 64, k + e - 1}
        have = {r for r in pool if r < k + e}
        assert have == set(gf.band_members(k, e)) and max(have) == k + e - 1
        c = gf.matrix(k, e, kind)
        src, par = block(c, 64, seed=k)
        for uu in {u, min(u, 7)}:
            lists = gf.band_lists(k, e, uu, B)
            rows = [dm.list_rows(lst, k, e) for lst in lists]
            assert lists.shape == (4, uu) and all(r is not None for r in rows)
            assert all(len(r) == min(min(uu, e) - 1, len(have)) and set(r) <= have for r in rows)
            assert set().union(*rows) == have
            lost = gf.wide_lists(k, e, uu, B)
            assert (lost[2:6] == lists).all() and (lost[:2] == gf.mixed_lists(k, e, uu, B)[:2]).all()
            hits, one, two = gf.wide_plan(lost, k, e, 64)
            want = {one: (1, dm.ONE_ROW, gf.wide_row(k, e)), two: (2, dm.DAMAGED, -1)}
            assert gf.wide_row(k, e) >= (k + 64 if k <= 64 else 64) and one != two and {one, two} <= {0, 2, 3, 4}
            for b in (one, two):
                s2, p2 = src.copy(), par.copy()
                for blk, row, col, x in hits:
                    if blk == b:
                        assert row not in dm.list_rows(lost[b], k, e)
                        xor_byte(s2, p2, row, col, x)
                for r in dm.list_rows(lost[b], k, e):  # whatever the lost rows hold
                    xor_byte(s2, p2, r, 5, 0x77)
                assert dm.report(c, s2, p2, lost[b]) == want[b], (k, e, uu, b)


def test_null_context_and_constants():
    L = rsgpu.lib()
    assert L.rsgpu_scrub_degraded_blocks(None, 16, 4, 4096, 4096, 1, None, None, None, 1, None, 1, None) == -1
    assert (rsgpu.LOST_NONE, rsgpu.SCRUB_UNCHECKED, rsgpu.SCRUB_BAD_MATRIX, rsgpu.SCRUB_BAD_LIST) == (
        dm.NONE, dm.UNCHECKED, dm.BAD_MATRIX, dm.BAD_LIST)
    assert (rsgpu.SCRUB_CLEAN, rsgpu.SCRUB_ONE_ROW, rsgpu.SCRUB_DAMAGED) == (dm.CLEAN, dm.ONE_ROW, dm.DAMAGED)
    assert "rsgpu_scrub_degraded_blocks" in rsgpu.EXPORTED_SYMBOLS
