"""numpy model of the rebuild's contract (include/rsgpu.h rsgpu_rebuild_blocks),
following its definitions literally:

* the pivot rows Q: the surviving parity rows in ascending order, each kept
  when it raises the RANK of c[Q][D] (tests/degraded_model.py rank);
* the lost data bytes: the solution of the linear system "syndromes of the
  rows in Q are zero", by Gaussian elimination on [c[Q][D] | right-hand side]
  with all columns at once;
* the lost parity rows: the encode of the completed data;
* the checked mode: the degraded model's report decides (report_syn).

No inverse matrix, no table of factors: it shares no code and no derivation
with the kernels.  Not a test module: tests/test_rebuild.py and
tests/test_gpu_rebuild.py import it.
"""
import numpy as np

import degraded_model as dm
import scrub_model as sm


def greedy_q(c, lost):
    """The pivot parity indices for the lost rows `lost`, or None when the
    surviving parity rows do not determine the lost data rows."""
    e, k = c.shape
    d = [r for r in lost if r < k]
    q = []
    for p in range(e):
        if len(q) == len(d):
            break
        if k + p in lost:
            continue
        if dm.rank(c[np.ix_(q + [p], d)]) > len(q):
            q.append(p)
    return q if len(q) == len(d) else None


def solve(a, rhs):
    """x with a x = rhs for an invertible a (n, n) and rhs (n, L)."""
    a = np.array(a, np.uint8, copy=True)
    x = np.array(rhs, np.uint8, copy=True)
    n = a.shape[0]
    for col in range(n):
        piv = next(r for r in range(col, n) if a[r, col])
        if piv != col:
            a[[col, piv]] = a[[piv, col]]
            x[[col, piv]] = x[[piv, col]]
        inv = sm.gf_inv(int(a[col, col]))
        a[col] = sm.gf_mul(a[col], inv)
        x[col] = sm.gf_mul(x[col], inv)
        for r in range(n):
            f = int(a[r, col])
            if r != col and f:
                a[r] ^= sm.gf_mul(a[col], f)
                x[r] ^= sm.gf_mul(x[col], f)
    return x


def encode(c, src):
    par = np.zeros((c.shape[0], src.shape[1]), np.uint8)
    for j in range(src.shape[0]):
        par ^= sm.gf_mul(c[:, j][:, None], src[j][None, :])
    return par


def rebuild_rows(c, src, par, lost):
    """(src, par) with the rows `lost` rebuilt from the others, or None when
    they are not determined.  The rows in `lost` are not read."""
    c = np.asarray(c, np.uint8)
    e, k = c.shape
    q = greedy_q(c, lost)
    if q is None:
        return None
    src, par = src.copy(), par.copy()
    d = [r for r in lost if r < k]
    if d:
        held = src.copy()
        held[d] = 0
        rhs = par[q] ^ encode(c[q], held)
        src[d] = solve(c[np.ix_(q, d)], rhs)
    lp = [r - k for r in lost if r >= k]
    if lp:
        par[lp] = encode(c[lp], src)
    return src, par


def call(c, src, par, lst, check, report=None):
    """The call on one block: ((bad_columns, status, row), src, par).  report:
    the degraded model's report of the block when the caller has it already
    (check only)."""
    c = np.asarray(c, np.uint8)
    e, k = c.shape
    lost = dm.list_rows(lst, k, e)
    if lost is None:
        return (0, dm.BAD_LIST, -1), src, par
    if e == 0 or src.shape[1] == 0:
        return (0, dm.CLEAN, -1), src, par
    if not check:
        out = rebuild_rows(c, src, par, lost)
        if out is None:
            return (0, dm.BAD_MATRIX, -1), src, par
        return (0, dm.CLEAN, -1), out[0], out[1]
    rep = dm.report(c, src, par, lst) if report is None else tuple(report)
    if rep[1] in (dm.BAD_MATRIX, dm.DAMAGED):
        return rep, src, par
    rows = sorted(lost + [rep[2]]) if rep[1] == dm.ONE_ROW else lost
    out = rebuild_rows(c, src, par, rows)
    if out is None:  # UNCHECKED looked at no matrix
        return (0, dm.BAD_MATRIX, -1), src, par
    return rep, out[0], out[1]
