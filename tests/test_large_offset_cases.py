"""tests/large_offset_cases.py without a device: the geometries' arithmetic,
the mutation check of tests/test_gpu_large_offsets.py by a numpy model of the
offset computations (which byte would a 32-bit offset touch, and does the GPU
test compare that byte?), and the periodic reference of the long rows against
the oracle."""
import numpy as np
import pytest

import large_offset_cases as lo
import scrub_model as sm
from oracle_lib import Oracle

T31, T32 = lo.T31, lo.T32


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.mark.parametrize("k,e,B,s_src,s_par", [(5, 4, 1027, 819, 1023), (64, 32, 131, 63, 127), (10, 4, 1027, 409, 1023),
                                              (9, 5, 823, 455, 819)])
def test_deep_geometry(k, e, B, s_src, s_par):
    p = lo.DEEP_PITCH
    assert p == 2 ** 20 + 64 and p & (p - 1) != 0
    assert lo.deep_blocks(e) == B
    assert (lo.straddler(k, p), lo.straddler(e, p)) == (s_src, s_par)
    # both buffers pass 2^32 on their own, by at least two whole blocks
    for rows, s in ((k, s_src), (e, s_par)):
        assert lo.row_offset(s, 0, rows, p) < T32 <= lo.row_offset(s + 1, 0, rows, p)
        assert s + 2 < B and lo.row_offset(B - 1, 0, rows, p) > T32
    sp = lo.special_blocks(k, e, p, B)
    assert {0, B - 1, s_src - 1, s_src, s_src + 1, s_par - 1, s_par, s_par + 1} == set(sp)


def aliases(mut, rows, pitch, B, L, blocks):
    """{(b, r): what the mutated offset of column 0 of row r of block b is} for
    the rows whose offset the mutation changes."""
    out = {}
    for b in blocks:
        for r in range(rows):
            a = mut(b, r, rows, 0)
            if a != lo.row_offset(b, r, rows, pitch):
                out[(b, r)] = lo.locate(a, rows, pitch, B, L)
    return out


@pytest.mark.parametrize("name", ["block_base_u32", "row_index_u32"])
@pytest.mark.parametrize("k,e", [(5, 4), (64, 32)])
def test_deep_mutations_land_in_compared_bytes(k, e, name):
    """A block base or a row index cut to 32 bits: from the straddling block
    on, every row's offset is another row's byte or its padding inside the
    buffer (never outside it), of a block before the straddler -- a byte the
    GPU tests compare with the model or with the fill.  The special blocks
    carry the damage, so a read there sees another block's bytes."""
    p, L = lo.DEEP_PITCH, 4176
    B = lo.deep_blocks(e)
    mut = lo.mutations(k, e, p)[name]
    for rows in (k, e):
        s = lo.straddler(rows, p)
        al = aliases(mut, rows, p, B, L, range(B))
        assert al and min(b for b, _ in al) in (s, s + 1)
        assert all(b >= s for b, _ in al)
        # every row of every block behind the straddler is affected
        assert {(b, r) for b in range(s + 1, B) for r in range(rows)} <= set(al)
        for (b, r), where in al.items():
            assert where is not None, (b, r)
            tb = where[1] if where[0] == "pad" else where[0]
            assert tb < b and tb <= B - s
        special = set(lo.special_blocks(k, e, p, B))
        assert {b for b, _ in al} & special >= {s + 1, B - 1}


def test_wide_mutations():
    """(2, 2) at pitch 2^31 + 64: a 32-bit row index sends block 1 to block
    0's bytes; an int pitch is negative and leaves the buffer (a fault, not a
    wrong byte).  (5, 4) at 2^30 + 64: a 32-bit row * pitch sends row 4 of
    either block to its row 0."""
    k, e, B, L = 2, 2, 2, 4176
    p = T31 + 64
    m = lo.mutations(k, e, p)
    al = aliases(m["row_index_u32"], k, p, B, L, range(B))
    assert al == {(1, 0): (0, 0, 128), (1, 1): (0, 1, 128)}
    assert lo.cut31(p) < 0
    assert aliases(m["pitch_int"], k, p, B, L, range(B)) == {(0, 1): None, (1, 0): None, (1, 1): None}
    k, e = 5, 4
    p = (1 << 30) + 64
    m = lo.mutations(k, e, p)
    assert lo.row_offset(0, 4, k, p) > T32 and lo.row_offset(1, 0, e, p) > T32
    assert aliases(m["row_pitch_u32"], k, p, B, L, range(B)) == {(0, 4): (0, 0, 256), (1, 4): (1, 0, 256)}
    assert aliases(m["row_index_u32"], e, p, B, L, range(B)) == {(1, r): (0, r, 256) for r in range(4)}
    assert aliases(m["pitch_int"], k, p, B, L, range(B)) == {}  # fits an int: the wider pitch is what catches it


@pytest.mark.parametrize("K", [5, 64])
@pytest.mark.parametrize("L,B,factor", [(32, 70, 66), (2080, 4, 2)])
def test_flat_edge(L, B, factor, K):
    """Both sides of the flat guard of the compiled encode, (5, 4) and (64, 16): below it
    the largest lane offset the kernel cuts to 32 bits is below 2^32 (and
    past 2^31); the same tiling one pitch step above would pass 2^32, and the
    cut offset would be a compared byte of an earlier block."""
    assert lo.flat_factor(L) == factor
    below, above = lo.flat_pitches(L, K)
    assert below % 32 == 0 and above == below + 32
    assert factor * K * below < T32 <= factor * K * above
    assert lo.flat_guard(L, K, below, B) and not lo.flat_guard(L, K, above, B)
    off, blk, col = lo.flat_lane_offsets(L, K, below, B)
    assert len(off) == B * L // 32            # every 32-byte piece of every block once
    # past 2^31 at len 32 (db up to 63); at len 2080 db <= 1 and K * pitch < 2^31 by the guard, so the
    # largest offset is K * pitch + o, o < 2016: past 2^31 for K = 5, 64 bytes short of it for K = 64
    assert (T31 if L == 32 or K == 5 else T31 - 2048) <= off.max() < T32
    # the mutation (the guard widened by a factor of 2): flat tiles where the
    # guard forbids them.  At L = 2080 a lane is at most one block from its
    # tile's first (x < 2 L), so no pitch the guard's double admits passes
    # 2^32: what the case pins is the offsets past 2^31.  At L = 32 a tile is
    # 64 whole blocks, db <= 63 where the guard allows for 65: offsets pass
    # 2^32 from lo.flat_true_edge on, the third pitch of the GPU test.
    off, blk, col = lo.flat_lane_offsets(L, K, above, B)
    if L == 2080:
        assert T31 - 2048 <= off.max() < T32 and 2 * factor * K * above > T32
        return
    assert off.max() < T32
    edge = lo.flat_true_edge(L, K)
    assert edge % 32 == 0 and above < edge and not lo.flat_guard(L, K, edge, B)
    assert 2 * 63 * K * edge > T32 > lo.flat_lane_offsets(L, K, edge - 32, B)[0].max()
    off, blk, col = lo.flat_lane_offsets(L, K, edge, B)
    over = off >= T32
    assert over.any()
    for o, b, c in zip(off[over], blk[over], col[over]):
        tile_b0 = b - o // (K * edge)
        where = lo.locate(lo.row_offset(tile_b0, 0, K, edge) + lo.cut32(o), K, edge, B, L)
        # another block's data byte or its padding, inside the buffer
        assert where is not None and (where[1] if where[0] == "pad" else where[0]) < b


def test_flat_guard_is_the_launchers():
    """The model's guard, term by term, at shapes the existing suites run."""
    assert lo.flat_guard(96, 16, 1 << 22, 130) and not lo.flat_guard(32, 64, 1 << 20, 67)
    assert not lo.flat_guard(2048, 5, 4096, 4) and not lo.flat_guard(2080, 5, 4096, 1)


def test_periodic_reference_is_the_oracles(orc):
    """Rows of period p tiled to 3 p + 100 bytes: the oracle's parity of the
    whole rows is its parity of one period, tiled.  A reference whose phase is
    off by 2^32 mod p (or 2^31 mod p) differs: a read at an offset cut to 32
    bits has the wrong phase."""
    p = lo.PERIOD
    assert p % 2 == 1 and T32 % p != 0 and T31 % p != 0
    for k, e in ((2, 1), (2, 2)):
        c = sm.rs_matrix(k, e)
        pat = lo.patterns(k)
        n = 3 * p + 100
        rows = lo.tile_to(pat, n)
        assert (rows[:, :p] == pat).all() and (rows[:, p: 2 * p] == pat).all() and (rows[:, 3 * p:] == pat[:, :100]).all()
        want = [np.zeros(n, np.uint8) for _ in range(e)]
        orc.encode_data(n, k, e, orc.init_tables(k, e, c), [np.ascontiguousarray(r) for r in rows], want)
        per = lo.parity_period(orc, c, pat)
        assert (lo.tile_to(per, n) == np.stack(want)).all()
        assert (per == lo.model_parity(c, pat)).all()
        for cut in (T32, T31):
            shifted = lo.tile_to(per, n, phase=cut % p)
            assert (shifted != np.stack(want)).mean() > 0.9
    # distinct patterns per row
    assert not (pat[0] == pat[1]).all()


def test_chunks():
    n = T32 + 2048 + 32
    ch, (t0, tn) = lo.chunks(n)
    assert sum(c for _, c in ch) == n // lo.PERIOD and t0 == n // lo.PERIOD * lo.PERIOD and t0 + tn == n
    assert all(c * lo.PERIOD <= 1 << 30 for _, c in ch) and [a for a, _ in ch] == sorted(a for a, _ in ch)
    assert all(a1 == a0 + c0 * lo.PERIOD for (a0, c0), (a1, _) in zip(ch, ch[1:]))
