"""Parity scrub on the CPU: the numpy model of the contract (scrub_model.py)
against parity made by the oracle, the host-only rsgpu_scrub_locatable against
the model's rule, and the argument check of rsgpu_scrub_blocks that needs no
device.  The device paths are in tests/test_gpu_scrub.py (-m gpu)."""
import numpy as np
import pytest

import rsgpu
import scrub_model as sm
from oracle_lib import Oracle

# (k, e) the locatable rule was checked for (RS and Cauchy both)
CODES = [(16, 4), (64, 32), (100, 20), (5, 4), (20, 7), (248, 2), (213, 37), (9, 40), (24, 12)]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def oracle_block(orc, c, k, e, L, seed):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (k, L), dtype=np.uint8)
    par = [np.zeros(L, np.uint8) for _ in range(e)]
    orc.encode_data(L, k, e, orc.init_tables(k, e, c), list(src), par)
    return src, np.stack(par)


def test_model_matrices_are_the_librarys(orc):
    for k, e in CODES:
        assert (sm.rs_matrix(k, e) == orc.gen_rs_matrix(k + e, k)[k:]).all()
        assert (sm.cauchy_matrix(k, e) == orc.gen_cauchy1_matrix(k + e, k)[k:]).all()


@pytest.mark.parametrize("k,e", [(16, 4), (5, 4), (20, 7), (9, 40)], ids=str)
@pytest.mark.parametrize("code", ["rs", "cauchy"])
def test_model_on_oracle_parity(orc, code, k, e):
    """CLEAN on the oracle's parity; single-row damage names the row, with
    the exact column count, for source and parity rows."""
    c = sm.rs_matrix(k, e) if code == "rs" else sm.cauchy_matrix(k, e)
    L = 97
    src, par = oracle_block(orc, c, k, e, L, seed=k * 100 + e)
    assert sm.scrub(c, src, par) == (0, sm.CLEAN, -1)
    assert sm.scrub(c, src, par, locate=False) == (0, sm.CLEAN, -1)
    clean = sm.syndromes(c, src, par)
    for row in (0, k - 1, k, k + e - 1):
        s2, p2 = src.copy(), par.copy()
        cols, xors = [0, 31, L - 1], [0x01, 0x80, 0xFF]
        for col, x in zip(cols, xors):
            if row < k:
                s2[row, col] ^= x
            else:
                p2[row - k, col] ^= x
        assert sm.scrub(c, s2, p2) == (3, sm.ONE_ROW, row)
        assert sm.scrub(c, s2, p2, locate=False) == (3, sm.DAMAGED, -1)
        # the linear shortcut the GPU tests use gives the same syndromes
        assert (sm.damage(c, clean, row, cols, xors) == sm.syndromes(c, s2, p2)).all()


def test_model_two_rows(orc):
    k, e, L = 16, 4, 64
    c = sm.rs_matrix(k, e)
    src, par = oracle_block(orc, c, k, e, L, seed=9)
    s2 = src.copy()
    s2[3, 5] ^= 0x11
    s2[9, 40] ^= 0x22
    assert sm.scrub(c, s2, par) == (2, sm.DAMAGED, -1)
    # the same column, e >= 3: distance >= 4, two errors never look like one
    s3 = src.copy()
    s3[3, 5] ^= 0x11
    s3[9, 5] ^= 0x22
    assert sm.scrub(c, s3, par) == (1, sm.DAMAGED, -1)


def test_scrub_locatable_known_codes():
    for k, e in CODES:
        assert sm.locatable(sm.rs_matrix(k, e)) and sm.locatable(sm.cauchy_matrix(k, e)), (k, e)
        assert rsgpu.scrub_locatable(k, e) is True
        assert rsgpu.scrub_locatable(k, e, sm.rs_matrix(k, e)) is True
        assert rsgpu.scrub_locatable(k, e, sm.cauchy_matrix(k, e)) is True


def test_scrub_locatable_rejects():
    assert rsgpu.scrub_locatable(16, 1) is False
    assert rsgpu.scrub_locatable(16, 0) is False
    assert rsgpu.scrub_locatable(16, 1, np.ones((1, 16), np.uint8)) is False
    c = sm.rs_matrix(16, 4).copy()
    c[0, 7] = 0
    assert not sm.locatable(c) and rsgpu.scrub_locatable(16, 4, c) is False
    c = sm.cauchy_matrix(16, 4).copy()
    c[:, 9] = sm.gf_mul(c[:, 2], 0x35)  # column 9 a multiple of column 2: equal ratios
    assert not sm.locatable(c) and rsgpu.scrub_locatable(16, 4, c) is False


def test_scrub_locatable_agrees_with_the_model_on_random_matrices():
    rng = np.random.default_rng(20)
    seen = set()
    for n in range(200):
        k, e = int(rng.integers(1, 13)), int(rng.integers(1, 6))
        # few distinct values: zeros and repeated ratios are common, not rare
        c = rng.integers(0 if n % 2 else 1, 256 if n % 4 < 2 else 8, (e, k), dtype=np.uint8)
        want = sm.locatable(c)
        seen.add(want)
        assert rsgpu.scrub_locatable(k, e, c) is want, (k, e, c)
    assert seen == {True, False}


def test_scrub_blocks_null_context_is_an_argument_error():
    L = rsgpu.lib()
    assert L.rsgpu_scrub_blocks(None, 16, 4, 4096, 4096, 1, None, None, None, 1, None) == -1
    assert L.rsgpu_set_scrub_kernel(None, 0) == -1


def test_report_dtype_is_the_headers_struct():
    dt = rsgpu.SCRUB_REPORT_DTYPE
    assert dt.itemsize == 16
    assert [(n, dt.fields[n][0].str, dt.fields[n][1]) for n in dt.names] == [
        ("bad_columns", "<u8", 0), ("status", "<i4", 8), ("row", "<i4", 12)]
    assert (rsgpu.SCRUB_CLEAN, rsgpu.SCRUB_ONE_ROW, rsgpu.SCRUB_DAMAGED) == (sm.CLEAN, sm.ONE_ROW, sm.DAMAGED)
