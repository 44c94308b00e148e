"""In-place repair on the CPU: the numpy model of the contract
(repair_model.py) against parity made by the oracle, the e = 2 miscorrection
the header warns of, and what of rsgpu_repair_blocks needs no device.  The
device paths are in tests/test_gpu_repair.py (-m gpu)."""
import numpy as np
import pytest

import repair_model as rm
import rsgpu
import scrub_model as sm
from oracle_lib import Oracle


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def oracle_block(orc, c, k, e, L, seed):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (k, L), dtype=np.uint8)
    par = [np.zeros(L, np.uint8) for _ in range(e)]
    orc.encode_data(L, k, e, orc.init_tables(k, e, c), list(src), par)
    return src, np.stack(par)


def hit(src, par, row, col, x):
    k = src.shape[0]
    if row < k:
        src[row, col] ^= x
    else:
        par[row - k, col] ^= x


@pytest.mark.parametrize("k,e", [(16, 4), (5, 4), (20, 7), (9, 40)], ids=str)
@pytest.mark.parametrize("code", ["rs", "cauchy"])
def test_model_on_oracle_parity(orc, code, k, e):
    c = sm.rs_matrix(k, e) if code == "rs" else sm.cauchy_matrix(k, e)
    L = 97
    src, par = oracle_block(orc, c, k, e, L, seed=k * 100 + e)
    for mode in rm.MODES:
        s2, p2, verdict = rm.repair(c, src, par, mode)
        assert verdict == (0, 0, rm.CLEAN, -1) and (s2 == src).all() and (p2 == par).all()
    # one row: restored byte for byte in both modes
    for row in (0, k - 1, k, k + e - 1):
        s1, p1 = src.copy(), par.copy()
        for col, x in zip([0, 31, L - 1], [0x01, 0x80, 0xFF]):
            hit(s1, p1, row, col, x)
        for mode in rm.MODES:
            s2, p2, verdict = rm.repair(c, s1, p1, mode)
            assert verdict == (3, 3, rm.REPAIRED, row)
            assert (s2 == src).all() and (p2 == par).all()
    # two rows, different columns: only COLUMNS restores
    for ra, rb in ((1, k - 1), (2, k + 1), (k, k + e - 1)):
        s1, p1 = src.copy(), par.copy()
        hit(s1, p1, ra, 5, 0x11)
        hit(s1, p1, rb, 40, 0x22)
        s2, p2, verdict = rm.repair(c, s1, p1, "one_row")
        assert verdict == (2, 0, rm.DAMAGED, -1) and (s2 == s1).all() and (p2 == p1).all()
        s2, p2, verdict = rm.repair(c, s1, p1, "columns")
        assert verdict == (2, 2, rm.REPAIRED, -1) and (s2 == src).all() and (p2 == par).all()
    # two rows in one column, e >= 3: distance >= 4, two errors never look
    # like one, so no row explains the column and nothing is written
    for ra, rb in ((1, 3), (0, k + e - 1), (k, k + 2)):
        s1, p1 = src.copy(), par.copy()
        hit(s1, p1, ra, 5, 0x11)
        hit(s1, p1, rb, 5, 0x22)
        for mode in rm.MODES:
            s2, p2, verdict = rm.repair(c, s1, p1, mode)
            assert verdict == (1, 0, rm.DAMAGED, -1) and (s2 == s1).all() and (p2 == p1).all()
        # and one correctable column beside it
        hit(s1, p1, k - 1, 60, 0x33)
        s2, p2, verdict = rm.repair(c, s1, p1, "one_row")
        assert verdict == (2, 0, rm.DAMAGED, -1) and (s2 == s1).all() and (p2 == p1).all()
        s2, p2, verdict = rm.repair(c, s1, p1, "columns")
        assert verdict == (2, 1, rm.PARTIAL, k - 1)
        hit(s1, p1, k - 1, 60, 0x33)
        assert (s2 == s1).all() and (p2 == p1).all()


def test_one_row_mode_miscorrects_with_two_parity_rows(orc):
    """The caveat's witness: (4, 2), gf_gen_rs_matrix rows (1 1 1 1) and
    (1 2 4 8).  Rows 0 and 1 damaged in one column by 0xF5 and 0x01 give the
    syndromes (0xF4, 0xF7) = (1, 4) * 0xF4: exactly row 2 damaged by 0xF4.
    ONE_ROW mode "repairs" row 2: a consistent block with three wrong bytes."""
    k, e, L = 4, 2, 16
    c = sm.rs_matrix(k, e)
    assert (c == [[1, 1, 1, 1], [1, 2, 4, 8]]).all()
    src, par = oracle_block(orc, c, k, e, L, seed=2)
    s1 = src.copy()
    s1[0, 9] ^= 0xF5
    s1[1, 9] ^= 0x01
    assert (sm.syndromes(c, s1, par)[:, 9] == [0xF4, 0xF7]).all()
    s2, p2, verdict = rm.repair(c, s1, par, "one_row")
    assert verdict == (1, 1, rm.REPAIRED, 2)
    assert not sm.syndromes(c, s2, p2).any()
    assert [(int(r), int(i)) for r, i in zip(*np.nonzero(s2 ^ src))] == [(0, 9), (1, 9), (2, 9)]
    assert s2[2, 9] == src[2, 9] ^ 0xF4 and (p2 == par).all()
    with pytest.raises(ValueError):
        rm.repair(c, s1, par, "columns")  # e < 3: refused


def test_repair_blocks_null_context_is_an_argument_error():
    L = rsgpu.lib()
    assert L.rsgpu_repair_blocks(None, 16, 4, 4096, 4096, 1, None, None, None, 0, None) == -1


def test_report_dtype_is_the_headers_struct():
    dt = rsgpu.REPAIR_REPORT_DTYPE
    assert dt.itemsize == 24
    assert [(n, dt.fields[n][0].str, dt.fields[n][1]) for n in dt.names] == [
        ("bad_columns", "<u8", 0), ("repaired_columns", "<u8", 8), ("status", "<i4", 16), ("row", "<i4", 20)]
    assert (rsgpu.REPAIR_CLEAN, rsgpu.REPAIR_REPAIRED, rsgpu.REPAIR_PARTIAL, rsgpu.REPAIR_DAMAGED) == (
        rm.CLEAN, rm.REPAIRED, rm.PARTIAL, rm.DAMAGED)
    assert rsgpu.REPAIR_MODES == {"one_row": rsgpu.REPAIR_ONE_ROW, "columns": rsgpu.REPAIR_COLUMNS}
    assert (rsgpu.REPAIR_ONE_ROW, rsgpu.REPAIR_COLUMNS) == (0, 1)
