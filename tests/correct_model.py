"""numpy model of the correction per byte column (include/rsgpu.h
rsgpu_correct_blocks), on top of the scrub's and the repair's models
(scrub_model.py, repair_model.py): per bad column E1, every row that explains
it alone (scrub_model.explaining_rows), and E2, every pair of rows {a, b} with
s = x h_a + y h_b, x and y non-zero, by brute force over all pairs and all
(x, y): for every row a and every x the rest s ^ x h_a is looked up among all
255 (k + e) vectors y h_b.  Not a test module: tests/test_correct.py and
tests/test_gpu_correct.py import it.
"""
import numpy as np

import repair_model as rm
import scrub_model as sm

CLEAN, REPAIRED, PARTIAL, DAMAGED = rm.CLEAN, rm.REPAIRED, rm.PARTIAL, rm.DAMAGED

_multiples = {}  # matrix -> (P, {bytes of y h_b: [(b, y)]})
_verdicts = {}  # (matrix, t, syndrome column) -> verdict


def supported(c: np.ndarray, t: int) -> bool:
    """The argument rules of the call for a matrix with e > 0."""
    e = np.asarray(c).shape[0]
    return t in (1, 2) and sm.locatable(c) and (e >= 3 if t == 1 else 5 <= e <= 64)


def multiples(c: np.ndarray):
    """P[r][x - 1] = x h_r for every row r of [0, k + e) and every x != 0, and
    the rows and factors behind every such vector."""
    c = np.ascontiguousarray(c, np.uint8)
    key = (c.shape, c.tobytes())
    if key not in _multiples:
        e, k = c.shape
        h = np.concatenate([c, np.eye(e, dtype=np.uint8)], axis=1)  # column r is h_r
        p = sm.MUL[h.T[:, None, :], np.arange(1, 256, dtype=np.uint8)[None, :, None]]  # (k + e, 255, e)
        where = {}
        for b in range(k + e):
            for y in range(1, 256):
                where.setdefault(p[b, y - 1].tobytes(), []).append((b, y))
        _multiples[key] = p, where
    return _multiples[key]


def explaining_pairs(c: np.ndarray, s: np.ndarray):
    """E2 of the syndrome column s: [(a, b, x, y)], a < b, over all pairs of
    rows of [0, k + e) and all non-zero x and y."""
    p, where = multiples(c)
    s = np.asarray(s, np.uint8)
    rest = p ^ s[None, None, :]
    found = set()
    for a in range(p.shape[0]):
        for x in range(1, 256):
            for b, y in where.get(rest[a, x - 1].tobytes(), ()):
                if a < b:
                    found.add((a, b, x, y))
                elif b < a:
                    found.add((b, a, y, x))
    return sorted(found)


def verdict(c: np.ndarray, s: np.ndarray, t: int):
    """What the call does to a bad column with syndromes s: [(row, x)] to XOR
    in, of length 0 (left alone), 1 or 2.  Memoised per syndrome column."""
    c = np.ascontiguousarray(c, np.uint8)
    key = (c.shape, c.tobytes(), t, np.asarray(s, np.uint8).tobytes())
    if key not in _verdicts:
        _verdicts[key] = _verdict(c, s, t)
    return _verdicts[key]


def _verdict(c, s, t):
    one = sm.explaining_rows(c, s)
    if len(one) == 1:
        return [(one[0], rm.error_value(c, s, one[0]))]
    if t == 2 and not one:
        pairs = explaining_pairs(c, s)
        if len({(a, b) for a, b, _, _ in pairs}) == 1:
            assert len(pairs) == 1  # independent h_a, h_b: one (x, y)
            a, b, x, y = pairs[0]
            return [(a, x), (b, y)]
    return []


def correct(c: np.ndarray, src: np.ndarray, par: np.ndarray, t: int):
    """(src', par', (bad_columns, corrected_columns, two_row_columns, status,
    row)) of one block: src (k, L), par (e, L); the inputs are left as they
    are."""
    c = np.asarray(c, np.uint8)
    e, k = c.shape
    if not supported(c, t):
        raise ValueError("unsupported")
    src, par = np.array(src, np.uint8, copy=True), np.array(par, np.uint8, copy=True)
    syn = sm.syndromes(c, src, par)
    bad = [int(i) for i in np.flatnonzero(syn.any(axis=0))]
    if not bad:
        return src, par, (0, 0, 0, CLEAN, -1)
    corrected = two = 0
    rows = set()  # of the corrected columns; -1 stands for a two-row correction
    for i in bad:
        fix = verdict(c, syn[:, i], t)
        if not fix:
            continue
        corrected += 1
        two += len(fix) == 2
        rows.add(fix[0][0] if len(fix) == 1 else -1)
        for r, x in fix:
            if r < k:
                src[r, i] ^= x
            else:
                par[r - k, i] ^= x
    status = REPAIRED if corrected == len(bad) else PARTIAL if corrected else DAMAGED
    return src, par, (len(bad), corrected, two, status, rows.pop() if len(rows) == 1 else -1)
