"""numpy model of the contract of rsgpu_locate_blocks (include/rsgpu.h),
following its definitions literally:

* W is the matrix of the block's distinct bad syndrome columns, d its rank;
* row r is a member when rank([W | h_r]) == rank(W), h_r being
  degraded_model.row_column;
* the verdict stands when d <= u, the members are d in number and their
  columns have rank d.

No echelon basis kept along the way, no merge, no lanes: it shares nothing
with the kernels but the field (tests/scrub_model.py) and the rank
(tests/degraded_model.py).  Not a test module: tests/test_locate.py and
tests/test_gpu_locate.py import it.
"""
import numpy as np

import degraded_model as dm
import scrub_model as sm

NONE = dm.NONE
CLEAN, ONE_ROW, DAMAGED, ROWS = 0, 1, 2, 4


def span_matrix(syn):
    """The block's distinct non-zero syndrome columns as an (e, n) matrix, and
    the number of bad columns."""
    bad = np.flatnonzero(syn.any(axis=0))
    if len(bad) == 0:
        return np.zeros((syn.shape[0], 0), np.uint8), 0
    return np.unique(syn[:, bad], axis=1), len(bad)


def members(c, w):
    """R = the rows whose column lies in the span of w's columns."""
    e, k = c.shape
    d = dm.rank(w)
    return [r for r in range(k + e) if dm.rank(np.column_stack([w, dm.row_column(c, r)])) == d]


def report_syn(c, syn, u):
    """((bad_columns, status, row), list of u entries) of a block from its
    syndromes (e, L)."""
    c = np.asarray(c, np.uint8)
    none = dm.pad([], u)
    if c.shape[0] == 0 or syn.shape[1] == 0:
        return (0, CLEAN, -1), none
    w, bad = span_matrix(syn)
    if bad == 0:
        return (0, CLEAN, -1), none
    d = dm.rank(w)
    if d > u:
        return (bad, DAMAGED, -1), none
    rows = members(c, w)
    if len(rows) != d or dm.rank(np.column_stack([dm.row_column(c, r) for r in rows])) != d:
        return (bad, DAMAGED, -1), none
    return (bad, ONE_ROW if d == 1 else ROWS, rows[0]), dm.pad(rows, u)


def report(c, src, par, u):
    """The same from the block's rows: src (k, L), par (e, L)."""
    c = np.asarray(c, np.uint8)
    syn = sm.syndromes(c, src, par) if c.shape[0] else np.zeros((0, src.shape[1]), np.uint8)
    return report_syn(c, syn, u)
