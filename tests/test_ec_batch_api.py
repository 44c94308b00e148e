"""rsgpu_ec_encode_data_batch on the CPU (include/rsgpu.h): the header declares
the call and its flag, the library exports it, the wrapper binds it, and bad
arguments are argument errors -- a null context through the call itself, the
rest through the check the call makes behind the context
(rsgpu_internal_ec_batch_args of the test-hooks library; no device).  Then the
case list of the GPU suite (tests/ec_batch_cases.py), on the list alone: every
program layout, every class of length and every kind of block is there, so
that the GPU comparison cannot pass on trivial input; the oracle runs over the
whole list, and a decode-matrix case recovers the rows it claims."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ec_batch_cases as bc
import rsgpu
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rsgpu.h")


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def test_the_header_declares_the_call_and_the_flag():
    txt = open(HEADER).read()
    assert re.search(r"^#define RSGPU_BATCH_ALIGNED32\s+1\b", txt, re.M)
    proto = re.search(r"^int rsgpu_ec_encode_data_batch\(([^;]*)\);", txt, re.M | re.S)
    assert proto, "no prototype"
    args = " ".join(proto.group(1).split())
    assert args == ("rsgpu_ctx *ctx, int k, int rows, const unsigned char *gftbls, size_t blocks, "
                    "const unsigned char *const *d_data, unsigned char *const *d_coding, const int *d_len, "
                    "int max_len, int flags, int *d_status")
    # the two footprints and the rejection rule are part of the contract
    doc = txt[: proto.start()].rsplit("/* rsgpu_ec_encode_data over", 1)[1]
    for phrase in ("status -2", "nothing else", "reads bytes [0, d_len[b]) only", "max_len"):
        assert phrase in " ".join(doc.split()), phrase


def test_the_library_exports_the_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", rsgpu.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r" T rsgpu_ec_encode_data_batch$", out, re.M)


def test_the_wrapper_binds_it():
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    fn = rsgpu.lib().rsgpu_ec_encode_data_batch
    assert fn.restype is C.c_int
    assert fn.argtypes == [vp, i, i, vp, sz, vp, vp, vp, i, i, vp]
    assert "rsgpu_ec_encode_data_batch" in rsgpu.EXPORTED_SYMBOLS
    assert rsgpu.BATCH_ALIGNED32 == 1 and "BATCH_ALIGNED32" in rsgpu.__all__ and "row_tables" in rsgpu.__all__
    assert callable(rsgpu.Context.ec_encode_data_batch) and callable(rsgpu.row_tables)


def test_a_null_context_is_an_argument_error():
    g = np.zeros(32 * 4 * 2, np.uint8)
    assert rsgpu.lib().rsgpu_ec_encode_data_batch(None, 4, 2, g.ctypes.data, 1, None, None, None, 0, 0, None) == -1
    assert rsgpu.lib().rsgpu_ec_encode_data_batch(None, 0, 0, None, 0, None, None, None, 0, 0, None) == -1


def test_bad_arguments_behind_the_context():
    hook = rsgpu.testhooks().rsgpu_internal_ec_batch_args
    hook.restype = C.c_int
    hook.argtypes = [C.c_int] * 5
    ok = lambda **kw: hook(*[{"k": 4, "rows": 2, "tables": 1, "max_len": 64, "flags": 0, **kw}[n]  # noqa: E731
                             for n in ("k", "rows", "tables", "max_len", "flags")])
    assert ok() == 0 and ok(flags=rsgpu.BATCH_ALIGNED32) == 0
    assert ok(k=250, rows=255) == 0 and ok(rows=0, tables=0) == 0 and ok(max_len=0) == 0
    for bad in (dict(k=0), dict(k=-1), dict(k=251), dict(rows=256), dict(rows=-1), dict(max_len=-1),
                dict(tables=0), dict(flags=2), dict(flags=-1)):
        assert ok(**bad) == -1, bad


def test_the_list_covers_every_layout_length_and_block():
    assert {(k, r) for k, r, _ in bc.CASES} == set(bc.GEOMS)
    assert {bc.layout_of(r) for _, r in bc.GEOMS} == {"8-row", "2x10", "2x12", "2x16", "4-wave", "passes"}
    assert [bc.layout_of(r) for _, r in bc.GEOMS] == ["8-row", "8-row", "2x10", "2x12", "2x16", "4-wave", "4-wave",
                                                      "passes", "8-row"]
    assert bc.passes_of(70) == 2 and all(bc.passes_of(r) == 1 for _, r in bc.GEOMS if r != 70)
    assert [bc.chunk_sources(r) for _, r in bc.GEOMS] == [8, 8, 5, 6, 6, 5, 6, 5, 8]
    assert all(k % bc.chunk_sources(r) for k, r in bc.GEOMS), "k off its layout's chunk size: a ragged last chunk"
    assert {kind for _, _, kind in bc.CASES} == {"rs", "cauchy", "random", "decode"}
    assert {(k, r) for k, r, kind in bc.CASES if kind == "decode"} == {(4, 2), (11, 27)}
    assert bc.LENGTHS == [0, 1, 31, 32, 33, 2016, 2047, 2048, 2080, 4096, 6144, 6145, 8209, 10240]
    tags = set().union(*(bc.length_classes(n) for n in bc.LENGTHS))
    assert tags == {"empty", "tail only", "one lane", "lanes and a tail", "partial tile", "whole tiles",
                    "tail against the tile edge", "odd tile count", "idle trailing tile"}
    assert bc.MAX_LENS == (10240, 16384)
    assert {bc.block_kind(b) for b in range(len(bc.LENGTHS))} == {"null", "source+1", "output+8", "shared source",
                                                                  "plain"}


@pytest.mark.parametrize("k,rows", bc.GEOMS, ids=str)
def test_the_plan_places_the_rows_as_it_says(k, rows):
    p = bc.plan(k, rows)
    d, c, n = p.tables(base=1 << 20)
    assert d.shape == (14, k) and c.shape == (14, rows) and n.tolist() == bc.LENGTHS
    assert not d[bc.NULL_BLOCK].any() and not c[bc.NULL_BLOCK].any()
    for b in range(1, 14):
        low = sorted({int(x) % 16 for x in d[b]} | {int(x) % 16 for x in c[b]})
        assert low == ([0, 1] if b in bc.SRC_OFF1 else [0, 8] if b in bc.OUT_OFF8 else [0]), (b, low)
        assert p.aligned(b) == (b not in bc.SRC_OFF1 + bc.OUT_OFF8)
    assert d[bc.SHARED[0], 0] == d[bc.SHARED[1], 0]
    # no two rows overlap, each has its guard, and the order is not the blocks'
    regs = [p.lay[nm] for b in range(14) for nm in set(p.src[b] + p.out[b]) if nm]
    uniq = sorted({(r.start, r.end) for r in regs})
    assert all(a[1] + 4096 <= b[0] for a, b in zip(uniq, uniq[1:]))
    starts = [p.lay[p.out[b][0]].start for b in range(1, 14)]
    assert starts != sorted(starts)
    assert all(b in range(14) and p.aligned(b) and bc.LENGTHS[b] % 32 == 0 for b in bc.ALIGNED32_KEEP)
    by_len, by_ptr = bc.ALIGNED32_BREAK
    assert p.aligned(by_len) and bc.LENGTHS[by_len] % 32 and not p.aligned(by_ptr) and bc.LENGTHS[by_ptr] % 32 == 0


def test_the_random_matrix_has_zeros_and_ones(orc):
    for k, rows, kind in bc.CASES:
        if kind == "random":
            c = bc.matrix(k, rows, kind, orc)
            assert c.shape == (rows, k) and (c == 0).sum() >= 2 and (c == 1).sum() >= 2 and (c > 1).sum() >= 2


@pytest.mark.parametrize("k,rows,kind", bc.CASES, ids=str)
def test_the_oracle_runs_over_the_whole_list(orc, k, rows, kind):
    """Expected bytes of every block, and their first principles: byte i of
    output r is the GF sum of c[r][j] * source j byte i."""
    p = bc.plan(k, rows)
    c = bc.matrix(k, rows, kind, orc)
    noise = p.lay.noise(1)
    want = p.expected(c, noise, orc)
    assert len(want) == 14 * rows and all(len(want[(b, r)]) == bc.LENGTHS[b] for b in range(14) for r in range(rows))
    rng = np.random.default_rng(3)
    for b in range(1, 14):
        n = bc.LENGTHS[b]
        for r in {0, rows - 1, int(rng.integers(0, rows))}:
            for i in {0, n - 1, int(rng.integers(0, n))}:
                v = 0
                for j in range(k):
                    v ^= orc.gf_mul(int(c[r, j]), int(noise[p.lay[p.src[b][j]].start + i]))
                assert want[(b, r)][i] == v, (b, r, i)


@pytest.mark.parametrize("k,rows", [(4, 2), (11, 27)], ids=str)
def test_a_decode_matrix_recovers_the_rows_it_claims(orc, k, rows):
    """The k sources of a block are the surviving rows of a stripe.  The stripe
    they determine: data = inverse x survivors, every row = encode matrix x
    data.  The decode matrix applied to the survivors gives its lost rows."""
    enc, lost, surv, inv, dmat = bc.decode_setup(k, rows, orc)
    assert (bc.matrix(k, rows, "decode", orc) == dmat).all()
    assert (lost < k).any() and (lost >= k).any() and len(set(lost) | set(surv)) == k + rows
    rc, inv2 = orc.invert_matrix(enc[surv])
    assert rc == 0 and (inv2 == inv).all()
    assert (bc.gf_matmul(orc, inv, enc[surv]) == np.eye(k, dtype=np.uint8)).all()
    p = bc.plan(k, rows)
    noise = p.lay.noise(1)
    want = p.expected(dmat, noise, orc)
    for b in (4, 8, 12):
        n = bc.LENGTHS[b]
        s = [np.ascontiguousarray(noise[p.lay[nm].start: p.lay[nm].start + n]) for nm in p.src[b]]
        data = [np.zeros(n, np.uint8) for _ in range(k)]
        orc.encode_data(n, k, k, orc.init_tables(k, k, inv), s, data)
        stripe = [np.zeros(n, np.uint8) for _ in range(k + rows)]
        orc.encode_data(n, k, k + rows, orc.init_tables(k, k + rows, enc), data, stripe)
        for i, r in enumerate(surv):
            assert (stripe[r] == s[i]).all(), "the survivors are rows of that stripe"
        for i, r in enumerate(lost):
            assert (want[(b, i)] == stripe[r]).all(), (b, i, r)
