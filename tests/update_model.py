"""numpy model of the partial-stripe update's contract (include/rsgpu.h
rsgpu_update_blocks) on top of scrub_model.py's field and matrices: the list
is validated first, then the listed source rows are replaced (or the rows
taken as deltas) and every parity row receives XOR_i c[p][j_i] * delta_i.
Not a test module: tests/test_update.py and tests/test_gpu_update.py import it.
"""
import numpy as np

from scrub_model import MUL

NONE = 255
OK, MALFORMED = 0, -2


def list_rows(cols, k: int):
    """The rows a list names, or None when it is malformed: indices in [0, k)
    strictly ascending, then only NONE to the end."""
    rows = []
    seen_none = False
    for j in (int(x) for x in cols):
        if j == NONE:
            seen_none = True
            continue
        if seen_none or j >= k or (rows and j <= rows[-1]):
            return None
        rows.append(j)
    return rows


def pad(rows, u: int) -> np.ndarray:
    """A list of width u from the rows."""
    out = np.full(u, NONE, np.uint8)
    out[: len(rows)] = rows
    return out


def update(c, src, par, cols, upd, delta: bool = False):
    """One block: c (e, k), src (k, L), par (e, L), cols (u,), upd (u, L).
    Returns (src', par', status); a malformed list leaves both as they were.
    Slots whose entry is NONE are not read."""
    c = np.asarray(c, np.uint8).reshape(par.shape[0], src.shape[0])
    src2 = np.array(src, np.uint8, copy=True)
    par2 = np.array(par, np.uint8, copy=True)
    rows = list_rows(cols, src.shape[0])
    if rows is None:
        return src2, par2, MALFORMED
    for i, j in enumerate(rows):
        d = np.asarray(upd[i], np.uint8)
        if not delta:
            d = d ^ src2[j]
            src2[j] = upd[i]
        if par2.shape[0]:
            par2 ^= MUL[c[:, j][:, None], d[None, :]]
    return src2, par2, OK
