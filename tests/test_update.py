"""Partial-stripe update on the CPU: the numpy model of the contract
(update_model.py) against parity made by the oracle, the invariance of the
syndromes, list validation, and what of rsgpu_update_blocks needs no device.
The device path is in tests/test_gpu_update.py (-m gpu)."""
import numpy as np
import pytest

import rsgpu
import scrub_model as sm
import update_model as um
from oracle_lib import Oracle


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def oracle_parity(orc, c, src):
    e, k = c.shape
    L = src.shape[1]
    par = [np.zeros(L, np.uint8) for _ in range(e)]
    orc.encode_data(L, k, e, orc.init_tables(k, e, c), [np.ascontiguousarray(r) for r in src], par)
    return np.stack(par)


@pytest.mark.parametrize("k,e", [(5, 4), (16, 4), (20, 7), (9, 40)], ids=str)
@pytest.mark.parametrize("code", ["rs", "cauchy"])
def test_model_on_oracle_parity(orc, code, k, e):
    """A consistent block, updated, has the oracle's parity of its new rows."""
    c = sm.rs_matrix(k, e) if code == "rs" else sm.cauchy_matrix(k, e)
    L = 97
    rng = np.random.default_rng(k * 100 + e)
    src = rng.integers(0, 256, (k, L), dtype=np.uint8)
    par = oracle_parity(orc, c, src)
    for rows in ([0], [k - 1], [0, k - 1], [1, 2, 4], list(range(k))):
        for u in {len(rows), k}:
            cols = um.pad(rows, u)
            upd = rng.integers(0, 256, (u, L), dtype=np.uint8)
            s2, p2, st = um.update(c, src, par, cols, upd)
            assert st == um.OK
            want = src.copy()
            want[rows] = upd[: len(rows)]
            assert (s2 == want).all()
            assert (p2 == oracle_parity(orc, c, want)).all()
            # the same as deltas: the source rows stay, the parity is the same
            deltas = upd.copy()
            deltas[: len(rows)] ^= src[rows]
            s3, p3, st = um.update(c, src, par, cols, deltas, delta=True)
            assert st == um.OK and (s3 == src).all() and (p3 == p2).all()
    # an all-NONE list: nothing
    s2, p2, st = um.update(c, src, par, um.pad([], 3), rng.integers(0, 256, (3, L), dtype=np.uint8))
    assert st == um.OK and (s2 == src).all() and (p2 == par).all()


@pytest.mark.parametrize("k,e", [(16, 4), (24, 12)], ids=str)
def test_syndromes_are_unchanged(k, e):
    """A block that is not consistent -- random parity, or damage in a row
    that is or is not rewritten -- keeps every syndrome across an update."""
    c = sm.cauchy_matrix(k, e)
    L = 64
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, (k, L), dtype=np.uint8)
    par = rng.integers(0, 256, (e, L), dtype=np.uint8)
    syn = sm.syndromes(c, src, par)
    assert syn.any()
    for rows in ([3], [0, 5, k - 1]):
        upd = rng.integers(0, 256, (len(rows), L), dtype=np.uint8)
        s2, p2, st = um.update(c, src, par, um.pad(rows, len(rows)), upd)
        assert st == um.OK and (sm.syndromes(c, s2, p2) == syn).all()
    # one damaged row keeps its verdict
    par = sm.syndromes(c, src, np.zeros((e, L), np.uint8))
    src[2, 9] ^= 0x41
    before = sm.scrub(c, src, par)
    assert before == (1, sm.ONE_ROW, 2)
    s2, p2, st = um.update(c, src, par, um.pad([7], 2), rng.integers(0, 256, (2, L), dtype=np.uint8))
    assert st == um.OK and sm.scrub(c, s2, p2) == before


def test_list_validation():
    k = 6
    N = um.NONE
    good = {(0,): [0], (5,): [5], (0, 5): [0, 5], (1, N): [1], (N, N): [], (0, 1, 2, 3, 4, 5): [0, 1, 2, 3, 4, 5],
            (2, 4, N, N): [2, 4]}
    for cols, rows in good.items():
        assert um.list_rows(cols, k) == rows
    bad = [(3, 1),        # descending
           (2, 2),        # duplicate
           (6,),          # index k
           (1, 254),      # an index >= k other than NONE
           (N, 1),        # a row after NONE
           (0, N, 3)]
    for cols in bad:
        assert um.list_rows(cols, k) is None, cols
    # a malformed list touches nothing
    rng = np.random.default_rng(1)
    c = sm.rs_matrix(k, 3)
    src = rng.integers(0, 256, (k, 8), dtype=np.uint8)
    par = rng.integers(0, 256, (3, 8), dtype=np.uint8)
    for cols in bad:
        upd = rng.integers(0, 256, (len(cols), 8), dtype=np.uint8)
        for delta in (False, True):
            s2, p2, st = um.update(c, src, par, cols, upd, delta=delta)
            assert st == um.MALFORMED and (s2 == src).all() and (p2 == par).all()


def test_update_blocks_null_context_is_an_argument_error():
    L = rsgpu.lib()
    assert L.rsgpu_update_blocks(None, 16, 4, 4096, 4096, 1, 1, None, None, None, None, None, 0, None) == -1


def test_constants_are_the_headers():
    assert (rsgpu.UPDATE_NONE, rsgpu.UPDATE_DELTA) == (um.NONE, 1) == (255, 1)
    assert hasattr(rsgpu.Context, "update_blocks") and hasattr(rsgpu.GpuEncoder, "update")
