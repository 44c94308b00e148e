"""numpy model of the parity scrub's contract (include/rsgpu.h
rsgpu_scrub_blocks): syndromes per byte column, which row explains a bad
column (brute force over all k + e rows), the locatable-matrix rule and the
per-block report.  GF(2^8) with polynomial 0x11D, generator 2, computed here.
Not a test module: tests/test_scrub.py and tests/test_gpu_scrub.py import it.
"""
import numpy as np

CLEAN, ONE_ROW, DAMAGED = 0, 1, 2


def _tables():
    exp = np.zeros(512, np.uint8)
    log = np.zeros(256, np.int32)
    v = 1
    for i in range(255):
        exp[i] = exp[i + 255] = v
        log[v] = i
        v <<= 1
        if v & 0x100:
            v ^= 0x11D
    exp[510], exp[511] = exp[0], exp[1]
    mul = np.zeros((256, 256), np.uint8)
    a = np.arange(1, 256)
    mul[1:, 1:] = exp[log[a][:, None] + log[a][None, :]]
    return exp, log, mul


EXP, LOG, MUL = _tables()


def gf_mul(a, b):
    """Element-wise product of uint8 arrays (broadcasting)."""
    return MUL[np.asarray(a, np.uint8), np.asarray(b, np.uint8)]


def gf_inv(a: int) -> int:
    assert a != 0
    return int(EXP[255 - LOG[a]])


def rs_matrix(k: int, e: int) -> np.ndarray:
    """Rows k..k+e-1 of gf_gen_rs_matrix(k+e, k): c[p][j] = 2^(p j)."""
    p = np.arange(e)[:, None]
    j = np.arange(k)[None, :]
    return EXP[(p * j) % 255].astype(np.uint8)


def cauchy_matrix(k: int, e: int) -> np.ndarray:
    """Rows k..k+e-1 of gf_gen_cauchy1_matrix(k+e, k): 1 / (i ^ j)."""
    c = np.zeros((e, k), np.uint8)
    for p in range(e):
        for j in range(k):
            c[p, j] = gf_inv((k + p) ^ j)
    return c


def locatable(c: np.ndarray) -> bool:
    """e >= 2, no zero in rows 0 and 1, the k ratios c[1][j] / c[0][j] distinct."""
    c = np.asarray(c, np.uint8)
    e, k = c.shape
    if e < 2 or (c[:2] == 0).any():
        return False
    ratios = {int(MUL[c[1, j], gf_inv(int(c[0, j]))]) for j in range(k)}
    return len(ratios) == k


def syndromes(c: np.ndarray, src: np.ndarray, par: np.ndarray) -> np.ndarray:
    """s[p][i] = par[p][i] ^ XOR_j c[p][j] src[j][i]; src (k, L), par (e, L)."""
    c = np.asarray(c, np.uint8)
    s = np.array(par, np.uint8, copy=True)
    for j in range(src.shape[0]):
        s ^= MUL[c[:, j][:, None], src[j][None, :]]
    return s


def damage(c: np.ndarray, syn: np.ndarray, row: int, cols, xors) -> np.ndarray:
    """The syndromes after row `row` of the block had bytes `cols` XORed with
    `xors`: the syndromes are linear in the rows, so a source row r adds
    c[p][r] x to every s_p and parity row k + p0 adds x to s_p0."""
    c = np.asarray(c, np.uint8)
    e, k = c.shape
    out = syn.copy()
    for col, x in zip(cols, xors):
        if row < k:
            out[:, col] ^= MUL[c[:, row], x]
        else:
            out[row - k, col] ^= x
    return out


def explaining_rows(c: np.ndarray, s: np.ndarray):
    """Every row of [0, k + e) that explains the syndrome column s (length e),
    by brute force over rows and over x."""
    c = np.asarray(c, np.uint8)
    e, k = c.shape
    s = np.asarray(s, np.uint8)
    # products[p][r][x - 1] = c[p][r] x for every x != 0
    products = MUL[c][:, :, 1:]
    fits = (products == s[:, None, None]).all(axis=0).any(axis=1)
    rows = [int(r) for r in np.flatnonzero(fits)]
    nz = np.flatnonzero(s)
    if len(nz) == 1:
        rows.append(k + int(nz[0]))
    return rows


def report(c: np.ndarray, syn: np.ndarray, locate: bool = True):
    """(bad_columns, status, row) of a block from its syndromes (e, L)."""
    bad = np.flatnonzero(syn.any(axis=0))
    if len(bad) == 0:
        return 0, CLEAN, -1
    if not locate:
        return len(bad), DAMAGED, -1
    seen = set()
    memo = {}
    for i in bad:
        key = syn[:, i].tobytes()
        if key not in memo:
            memo[key] = explaining_rows(c, syn[:, i])
        rows = memo[key]
        if len(rows) != 1:  # no row (or, for a matrix that is not locatable, several)
            return len(bad), DAMAGED, -1
        seen.add(rows[0])
    if len(seen) == 1:
        return len(bad), ONE_ROW, seen.pop()
    return len(bad), DAMAGED, -1


def scrub(c: np.ndarray, src: np.ndarray, par: np.ndarray, locate: bool = True):
    return report(c, syndromes(c, src, par), locate)
