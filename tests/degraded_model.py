"""numpy model of the degraded scrub's contract (include/rsgpu.h
rsgpu_scrub_degraded_blocks), following its definitions literally:

* a column is consistent when SOME choice of bytes for the lost rows makes
  all e syndromes zero -- decided by Gaussian elimination over GF(2^8) of the
  system "lost rows' columns x unknown bytes = syndromes";
* a surviving row r explains a bad column when XORing SOME x != 0 into its
  byte makes the column consistent -- every surviving row and every x tried.

No pivot rows, no reduced syndromes: it shares no code and no derivation with
the kernels.  GF(2^8) tables come from tests/scrub_model.py.  Not a test
module: tests/test_degraded.py and tests/test_gpu_degraded.py import it.
"""
import numpy as np

import scrub_model as sm

NONE = 255
CLEAN, ONE_ROW, DAMAGED, UNCHECKED, BAD_MATRIX, BAD_LIST = 0, 1, 2, 3, -1, -2


def pad(rows, u):
    """A list of u entries: `rows`, then NONE."""
    out = np.full(u, NONE, np.uint8)
    out[: len(rows)] = rows
    return out


def list_rows(lst, k, e):
    """The lost rows of a list, or None when it is malformed: not strictly
    ascending, an index >= k + e, a row after a NONE, more than e rows."""
    rows, none, prev = [], False, -1
    for j in (int(x) for x in lst):
        if j == NONE:
            none = True
            continue
        if none or j >= k + e or j <= prev:
            return None
        prev = j
        rows.append(j)
    return rows if len(rows) <= e else None


def row_column(c, r):
    """What a unit change of row r's byte adds to the e syndromes."""
    e, k = c.shape
    if r < k:
        return c[:, r].copy()
    g = np.zeros(e, np.uint8)
    g[r - k] = 1
    return g


def consistent(a, s):
    """For every column of s (e, N): is a x = s[:, i] solvable?  a is (e, n).
    Gauss-Jordan on [a | s], all N right-hand sides at once; a column is
    solvable when the rows left without a pivot are zero in it."""
    a = np.array(a, np.uint8, copy=True)
    s = np.array(s, np.uint8, copy=True)
    e, n = a.shape
    rank = 0
    for col in range(n):
        piv = next((r for r in range(rank, e) if a[r, col]), None)
        if piv is None:
            continue
        if piv != rank:
            a[[rank, piv]] = a[[piv, rank]]
            s[[rank, piv]] = s[[piv, rank]]
        inv = sm.gf_inv(int(a[rank, col]))
        a[rank] = sm.gf_mul(a[rank], inv)
        s[rank] = sm.gf_mul(s[rank], inv)
        for r in range(e):
            f = int(a[r, col])
            if r != rank and f:
                a[r] ^= sm.gf_mul(a[rank], f)
                s[r] ^= sm.gf_mul(s[rank], f)
        rank += 1
    return ~s[rank:].any(axis=0)


def rank(a):
    a = np.array(a, np.uint8, copy=True)
    rows, cols = a.shape
    rk = 0
    for col in range(cols):
        piv = next((r for r in range(rk, rows) if a[r, col]), None)
        if piv is None:
            continue
        a[[rk, piv]] = a[[piv, rk]]
        a[rk] = sm.gf_mul(a[rk], sm.gf_inv(int(a[rk, col])))
        for r in range(rows):
            f = int(a[r, col])
            if r != rk and f:
                a[r] ^= sm.gf_mul(a[rk], f)
        rk += 1
    return rk


def determined(c, lost):
    """Some |D| surviving parity rows p have c[p][D] invertible: the rank of
    the surviving parity rows' c[p][D] is |D|."""
    e, k = c.shape
    d = [r for r in lost if r < k]
    surv = [p for p in range(e) if k + p not in lost]
    if not d:
        return True
    return rank(c[np.ix_(surv, d)]) == len(d)


def explaining_rows(c, a, lost, s):
    """Every surviving row that explains the syndrome column s (length e)."""
    e, k = c.shape
    x = np.arange(1, 256, dtype=np.uint8)
    rows = [r for r in range(k + e) if r not in lost]
    cand = np.empty((e, len(rows), 255), np.uint8)
    for n, r in enumerate(rows):
        cand[:, n, :] = s[:, None] ^ sm.gf_mul(row_column(c, r)[:, None], x[None, :])
    fits = consistent(a, cand.reshape(e, -1)).reshape(len(rows), 255).any(axis=1)
    return [r for r, f in zip(rows, fits) if f]


def report_syn(c, syn, lst, locate=True):
    """(bad_columns, status, row) of a block from its list and its syndromes
    (e, L), taken with whatever bytes the lost rows hold."""
    c = np.asarray(c, np.uint8)
    e, k = c.shape
    lost = list_rows(lst, k, e)
    if lost is None:
        return 0, BAD_LIST, -1
    if e == 0 or syn.shape[1] == 0:
        return 0, CLEAN, -1
    if len(lost) == e:
        return 0, UNCHECKED, -1
    if not determined(c, lost):
        return 0, BAD_MATRIX, -1
    a = np.stack([row_column(c, r) for r in lost], axis=1) if lost else np.zeros((e, 0), np.uint8)
    bad = np.flatnonzero(~consistent(a, syn))
    if len(bad) == 0:
        return 0, CLEAN, -1
    if not locate:
        return len(bad), DAMAGED, -1
    seen, memo = set(), {}
    for i in bad:
        key = syn[:, i].tobytes()
        if key not in memo:
            memo[key] = explaining_rows(c, a, lost, syn[:, i])
        rows = memo[key]
        if len(rows) != 1:
            return len(bad), DAMAGED, -1
        seen.add(rows[0])
    if len(seen) == 1:
        return len(bad), ONE_ROW, seen.pop()
    return len(bad), DAMAGED, -1


def report(c, src, par, lst, locate=True):
    """(bad_columns, status, row) of a block: src (k, L), par (e, L)."""
    c = np.asarray(c, np.uint8)
    e, k = c.shape
    if list_rows(lst, k, e) is None:
        return 0, BAD_LIST, -1
    syn = sm.syndromes(c, src, par) if e else np.zeros((0, src.shape[1]), np.uint8)
    return report_syn(c, syn, lst, locate)
