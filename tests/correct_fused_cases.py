"""Damage for rsgpu_correct_blocks under rsgpu_set_correct_kernel FUSED
(k_rs_bs_correct), planned by position in the fused kernel's tile.  Not a test
module: tests/test_correct_kernel_api.py (the model and the host hook) and
tests/test_gpu_correct_fused.py (the device) import it.

A workgroup of NW waves takes a tile of 2048 byte columns; tile lane `lane`
holds 32 of them, and the cold path lays them into LDS in four passes of 8
bytes per lane:

    column = 2048 tile + 32 lane + 8 pass + byte

Column c = 8 lane + byte of a pass is walked by thread c mod 64 NW of the
workgroup at step c div 64 NW, so tile lanes 8 w .. 8 w + 7 (mod 8 NW) belong
to wave w.  Wave w also owns the parity rows [w OPW, (w + 1) OPW), OPW =
ceil(e / NW): their syndromes reach LDS from that wave's registers.

plan(k, e, L, block) is what one block gets, as correct_cases.plan gives it:
[(kind, column, [(row, x)])], every column once, all below L."""
import numpy as np

# the compiled codes with t = 2 (5 <= e <= 64), those with t = 1 only, and
# the waves of each one's workgroup (csrc/gen_enc_progs.py)
T2_CODES = [(16, 8), (20, 7), (64, 16), (64, 32), (100, 20)]
T1_CODES = [(16, 4), (5, 4)]
WAVES = {(16, 4): 1, (16, 8): 1, (64, 32): 4, (64, 16): 2, (100, 20): 4, (5, 4): 1, (20, 7): 1}
PAIR_KINDS = ("data+data", "data+parity", "data+parity0", "parity01", "parity+parity", "parity0+last")


def col(tile, lane, pas, byte):
    return 2048 * tile + 32 * lane + 8 * pas + byte


def hits_of(kind, k, e, rng):
    """[(row, x)] of one damaged column of `kind`; e >= 5 for the pairs."""
    x = lambda: int(rng.integers(1, 256))  # noqa: E731
    data = lambda n: [int(r) for r in rng.choice(k, n, replace=False)]  # noqa: E731
    if kind == "one":
        return [(data(1)[0], x())]
    if kind == "one-parity":
        return [(k + int(rng.integers(0, e)), x())]
    if kind == "data+data":
        return [(r, x()) for r in sorted(data(2))]
    if kind == "data+parity":  # parity row k + p, p >= 1
        return [(data(1)[0], x()), (k + int(rng.integers(1, e)), x())]
    if kind == "data+parity0":
        return [(data(1)[0], x()), (k, x())]
    if kind == "parity01":
        return [(k, x()), (k + 1, x())]
    if kind == "parity+parity":
        p, q = sorted(int(v) for v in rng.choice(np.arange(1, e), 2, replace=False))
        return [(k + p, x()), (k + q, x())]
    if kind == "parity0+last":  # NW > 1: rows of the first and of the last wave
        return [(k, x()), (k + e - 1, x())]
    if kind == "three":
        return [(r, x()) for r in sorted(data(3))]
    if kind == "three-mixed":
        return [(data(1)[0], x()), (k, x()), (k + e - 1, x())]
    raise ValueError(kind)


def plan(k, e, L, block):
    assert L % 32 == 0 and L > 0
    rng = np.random.default_rng(5000 * k + 50 * e + block)
    want = []  # (kind, column)
    # every pass holds a one-row and a pending column; the pair kinds in turn
    for pas in range(4):
        want.append(("one" if pas % 2 == 0 else "one-parity", col(0, 5 + pas, pas, 1)))
        want.append((PAIR_KINDS[pas], col(0, 20 + 3 * pas, pas, 6)))
    # two pending columns in adjacent bytes of one lane and pass
    want += [("data+data", col(0, 9, 1, 2)), ("parity+parity", col(0, 9, 1, 3))]
    # a one-row and a pending column in one 8-byte group
    want += [("one", col(0, 11, 2, 0)), ("parity0+last", col(0, 11, 2, 5))]
    # pending columns of one pass in different waves (NW = 2: lanes 0, 8; NW = 4: 0, 8, 16, 24)
    want += [(kind, col(0, lane, 3, 4)) for kind, lane in
             (("data+data", 0), ("data+parity", 8), ("parity0+last", 16), ("data+parity0", 24))]
    # two steps of one thread's walk: columns c and c + 64 NW of pass 0, NW = 1, 2, 4
    want += [("data+data", col(0, lane, 0, 3)) for lane in (2, 10, 18, 34)]
    # the corners of a full tile, and the first column of the next one
    want += [("data+data", col(0, 0, 0, 0)), ("data+parity", col(0, 63, 3, 7)), ("data+data", col(1, 0, 0, 0))]
    assert col(0, 63, 3, 7) == 2047 and col(1, 0, 0, 0) == 2048
    # the last tile (partial unless L % 2048 == 0): its first column, a one-row
    # column in its first lane, the first and the last byte of its last lane
    t0 = (L - 1) // 2048 * 2048
    want += [("parity01", t0), ("one", t0 + 8 + 2), ("data+parity", L - 32), ("data+data", L - 1)]
    # three rows: left as they are
    want += [("three", col(0, 40, 1, 0)), ("three-mixed", col(0, 41, 2, 7)), ("three", col(1, 3, 3, 5))]
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
    rng = np.random.default_rng(7000 * k + 70 * e + block)
    out = []
    for n, (_, c, _) in enumerate(plan(k, 5, L, block)):
        kind = ("one", "one-parity", "data+data")[n % 3]
        out.append((kind, c, hits_of(kind, k, e, rng)))
    return out
