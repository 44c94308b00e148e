"""numpy model of the in-place repair's contract (include/rsgpu.h
rsgpu_repair_blocks), on top of the scrub's model (scrub_model.py): a bad
column is corrected when exactly one row explains it, by brute force over rows
(scrub_model.explaining_rows) and over the error value.  Not a test module:
tests/test_repair.py and tests/test_gpu_repair.py import it.
"""
import numpy as np

import scrub_model as sm

CLEAN, REPAIRED, PARTIAL, DAMAGED = 0, 1, 2, 3
MODES = ("one_row", "columns")


def error_value(c: np.ndarray, s: np.ndarray, row: int) -> int:
    """The x with which `row` explains the syndrome column s: c[p][row] x = s_p
    for every p (a source row), or s_p0 itself (parity row k + p0)."""
    e, k = c.shape
    if row >= k:
        return int(s[row - k])
    xs = [x for x in range(1, 256) if (sm.MUL[c[:, row], x] == s).all()]
    assert len(xs) == 1
    return xs[0]


def repair(c: np.ndarray, src: np.ndarray, par: np.ndarray, mode: str):
    """(src', par', (bad_columns, repaired_columns, status, row)) of one block:
    src (k, L), par (e, L); the inputs are left as they are."""
    assert mode in MODES
    c = np.asarray(c, np.uint8)
    e, k = c.shape
    if not sm.locatable(c) or (mode == "columns" and e < 3):
        raise ValueError("unsupported")
    src, par = np.array(src, np.uint8, copy=True), np.array(par, np.uint8, copy=True)
    syn = sm.syndromes(c, src, par)
    bad = [int(i) for i in np.flatnonzero(syn.any(axis=0))]
    if not bad:
        return src, par, (0, 0, CLEAN, -1)
    fixes = {}  # column -> (row, x) where exactly one row explains it
    memo = {}
    for i in bad:
        key = syn[:, i].tobytes()
        if key not in memo:
            rows = sm.explaining_rows(c, syn[:, i])
            memo[key] = (rows[0], error_value(c, syn[:, i], rows[0])) if len(rows) == 1 else None
        if memo[key] is not None:
            fixes[i] = memo[key]
    rows = {r for r, _ in fixes.values()}
    if mode == "one_row" and not (len(fixes) == len(bad) and len(rows) == 1):
        return src, par, (len(bad), 0, DAMAGED, -1)
    for i, (r, x) in fixes.items():
        if r < k:
            src[r, i] ^= x
        else:
            par[r - k, i] ^= x
    status = REPAIRED if len(fixes) == len(bad) else PARTIAL if fixes else DAMAGED
    return src, par, (len(bad), len(fixes), status, rows.pop() if len(rows) == 1 else -1)
