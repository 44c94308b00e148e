"""Damage for rsgpu_correct_blocks under rsgpu_set_correct_kernel FUSED with the
scrub kernel GENERATED (k_rs_jit_correct, k_rs_jitw_correct), planned by
position in the generated kernels' tile.  Not a test module:
tests/test_correct_generated_api.py (the model and the host hook) and
tests/test_gpu_correct_generated.py (the device) import it.

A tile is 2048 byte columns; tile lane `lane` holds 32 of them, and the cold
path lays them into LDS in eight passes of 4 bytes per lane:

    column = 2048 tile + 32 lane + 4 pass + byte

Column c = 4 lane + byte of a pass's 256 is walked by thread c mod 64 NV of the
tile's NV waves (1: e <= 8; 2: e <= 32; 4: e <= 64) at trip c div 64 NV, so
wave w owns the tile lanes with lane mod 16 NV in [16 w, 16 w + 16) and makes
4 / NV trips: four with one wave, two with two, one with four.  A workgroup of
the two-wave wide layouts (16 < e <= 32) covers TPW = 1, 2 or 3 consecutive
tiles.

plan(k, e, L, block) is what one block gets, as correct_cases.plan gives it:
[(kind, column, [(row, x)])], every column once, all below L."""
import numpy as np

from correct_fused_cases import PAIR_KINDS, hits_of

# three tiles and five lanes: with TPW = 3 workgroup 0 owns tiles 0 .. 2 and the
# last one tile 3 (five lanes) and two tiles past the row end
L0 = 3 * 2048 + 5 * 32

# the matrices of the GPU suite with t = 2, (k, e, kind): every layout of the
# generated kernels -- one wave of 8 rows, two waves of 8, two of 10 / 12 / 16,
# four of 10 / 12 / 16 -- and two gf_gen_rs_matrix codes that are not compiled in
CAUCHY = [(10, 5), (11, 12), (13, 20), (13, 24), (14, 32), (9, 34), (9, 44), (8, 56)]
T2_SHAPES = [(k, e, "cauchy") for k, e in CAUCHY] + [(10, 6, "rs"), (14, 32, "rs")]
# t = 1 only, and more than 64 data rows
T1_SHAPES = [(10, 4, "cauchy"), (6, 3, "cauchy"), (17, 3, "cauchy")]
BAND_SHAPES = [(65, 6, "cauchy"), (129, 7, "cauchy"), (245, 5, "cauchy")]


def col(tile, lane, pas, byte):
    return 2048 * tile + 32 * lane + 4 * pas + byte


def where(c):
    """(tile, lane, pass, byte) of column c."""
    return c // 2048, c % 2048 // 32, c % 32 // 4, c % 4


def plan(k, e, L, block):
    assert L % 32 == 0 and L > 0
    rng = np.random.default_rng(9000 * k + 90 * e + block)
    want = []  # (kind, column)
    # every pass holds a one-row and a pending column; the pair kinds in turn
    for pas in range(8):
        want.append(("one" if pas % 2 == 0 else "one-parity", col(0, 5 + pas, pas, 1)))
        want.append((PAIR_KINDS[pas % len(PAIR_KINDS)], col(0, 20 + 3 * pas, pas, 2)))
    # two pending columns in adjacent bytes of one lane and pass
    want += [("data+data", col(0, 9, 1, 2)), ("parity+parity", col(0, 9, 1, 3))]
    # a one-row and a pending column in one dword
    want += [("one", col(0, 11, 2, 0)), ("parity0+last", col(0, 11, 2, 3))]
    # pending columns of one pass in every wave's share (NV = 1: all wave 0's;
    # NV = 2: lanes 0, 32 wave 0 and 16, 48 wave 1; NV = 4: a wave each)
    want += [(kind, col(0, lane, 3, 1)) for kind, lane in
             (("data+data", 0), ("data+parity", 16), ("parity0+last", 32), ("data+parity0", 48))]
    # two trips of one thread's walk: columns c and c + 64 NV of pass 0, lanes
    # l and l + 16 NV: (2, 18) with one wave, (2, 34) with two; four waves make one trip
    want += [("data+data", col(0, lane, 0, 3)) for lane in (2, 18, 34)]
    # the corners of a full tile, and the first column of the next one
    want += [("data+data", col(0, 0, 0, 0)), ("data+parity", col(0, 63, 7, 3)), ("data+data", col(1, 0, 0, 0))]
    assert col(0, 63, 7, 3) == 2047 and col(1, 0, 0, 0) == 2048
    # the third tile of a workgroup of three
    want += [("data+parity0", col(2, 7, 5, 2)), ("one", col(2, 7, 6, 0))]
    # the last tile (partial unless L % 2048 == 0): its first column, a one-row
    # column in its first lane, the first and the last byte of its last lane
    t0 = (L - 1) // 2048 * 2048
    want += [("parity01", t0), ("one", t0 + 4 + 2), ("data+parity", L - 32), ("data+data", L - 1)]
    # three rows: left as they are
    want += [("three", col(0, 40, 1, 0)), ("three-mixed", col(0, 41, 2, 3)), ("three", col(1, 3, 3, 1))]
    out, seen = [], set()
    for kind, c in want:
        hits = hits_of(kind, k, e, rng)  # drawn even when the column is dropped: the same damage at every L
        if c < L and c not in seen:
            seen.add(c)
            out.append((kind, c, hits))
    return out


def t1_plan(k, e, L, block):
    """e < 5, t = 1 only: one-row columns at the plan's positions, and columns
    damaged in two rows, which stay."""
    rng = np.random.default_rng(7100 * k + 71 * e + block)
    out = []
    for n, (_, c, _) in enumerate(plan(k, 5, L, block)):
        kind = ("one", "one-parity", "data+data")[n % 3]
        out.append((kind, c, hits_of(kind, k, e, rng)))
    return out
