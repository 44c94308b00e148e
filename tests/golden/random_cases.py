"""Seeded random inputs of the oracle-vs-reference cross-checks in
tests/test_oracle.py and the digest of a library's results on them.

gen_golden.py records the REFERENCE's digests in reference_random.json, so the
cross-checks run where the reference library (oracle/_ref) is not built; where
it is, the tests also compare with it live.  `lib` below is an
oracle_lib.Oracle or an oracle_lib.Reference (same method names).
"""
import hashlib

import numpy as np

MATRIX_SHAPES = ((9, 5), (20, 16), (96, 64), (120, 100), (250, 200))


def digest(*parts) -> str:
    """SHA-256 (first 16 hex digits) over the bytes of every part in order."""
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes())
    return h.hexdigest()[:16]


def encode_cases():
    rng = np.random.default_rng(11)  # TEST_SEED of erasure_code_base_test.c:62
    for _ in range(30):
        k = int(rng.integers(1, 40))
        rows = int(rng.integers(1, 20))
        L = int(rng.integers(1, 700))
        coef = rng.integers(0, 256, (rows, k), dtype=np.uint8)
        data = [rng.integers(0, 256, L, dtype=np.uint8) for _ in range(k)]
        vec_i = int(rng.integers(0, k))
        yield k, rows, L, coef, data, vec_i


def encode_result(lib, case) -> str:
    """Tables, the encoded rows and the rows after the update path
    (ec_encode_data_update_base) of source vec_i."""
    k, rows, L, coef, data, vec_i = case
    g = lib.init_tables(k, rows, coef)
    out = [np.zeros(L, np.uint8) for _ in range(rows)]
    lib.encode_data(L, k, rows, g, data, out)
    upd = [x.copy() for x in out]
    lib.encode_data_update(L, k, rows, vec_i, g, data[vec_i], upd)
    return digest(g, *out, *upd)


def invert_cases():
    rng = np.random.default_rng(5)
    for _ in range(40):
        n = int(rng.integers(1, 60))
        mat = rng.integers(0, 256, (n, n), dtype=np.uint8)
        if rng.random() < 0.3:  # force singular: duplicate a row
            mat[n - 1] = mat[0]
        yield mat


def invert_result(lib, mat) -> str:
    rc, inv = lib.invert_matrix(mat)
    return digest(np.int32(rc), inv) if rc == 0 else digest(np.int32(rc))


def matrices_result(lib, m, k) -> str:
    return digest(lib.gen_rs_matrix(m, k), lib.gen_cauchy1_matrix(m, k))


def general_cases():
    """(kind, k, m, erased rows) over data and parity rows."""
    rng = np.random.default_rng(13)
    for trial in range(400):
        k = int(rng.integers(1, 60))
        p = int(rng.integers(1, 24))
        m = k + p
        n = int(rng.integers(1, p + 1))
        err = np.sort(rng.choice(m, n, replace=False)).astype(np.uint8)
        yield ("rs" if trial % 2 else "cauchy"), k, m, err


def general_result(lib, enc, err) -> str:
    """Status, decode matrix and survivor choice of gf_gen_decode_matrix."""
    rc, dm, idx = lib.gen_decode_matrix(enc, err)
    return digest(np.int32(rc), dm, idx) if rc == 0 else digest(np.int32(rc))
