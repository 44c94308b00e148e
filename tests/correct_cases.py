"""The codes, layouts and damage of the suites of rsgpu_correct_blocks
(tests/test_correct.py on the model, tests/test_gpu_correct.py on the device).
Not a test module.

plan(k, e, L, block) is what one block gets: [(kind, column, [(row, x)])].
The columns are chosen for k_correct_compare's walk: a thread owns a 16-byte
group of 16-byte aligned rows (a byte of unaligned ones), a wave 64 of them.

The shapes with more than 64 data rows, (65, 6) (129, 7) (245, 5) Cauchy and
(100, 20) (213, 37) RS, are there for the loops of the wave over the data
rows (the per-row tables, the data-plus-parity search, the data-pair search
in bands of 64 rows): band_pairs(k, e) damages pairs of rows inside a band,
across two bands and on both sides of every band's edge."""
import numpy as np

# (k, e, matrix): Cauchy for the MDS property; gf_gen_rs_matrix shapes that the
# model corrects in every planned one- and two-row column (test_correct.py);
# k + e > 64 rows; a lane per syndrome used up (e = 64); k > 64, where the
# wave's loops over the data rows take a second trip: one lane on it (65),
# the C5 code (100, 20), three trips (129), k + e = 250 (245, 5)
SHAPES = [(6, 5, "cauchy"), (12, 6, "cauchy"), (16, 8, "rs"), (20, 7, "rs"), (64, 32, "rs"), (8, 64, "cauchy"),
          (65, 6, "cauchy"), (100, 20, "rs"), (129, 7, "cauchy"), (245, 5, "cauchy")]
# the shapes of band_pairs: SHAPES' k > 64 and the scrub's large RS shape
BAND_SHAPES = SHAPES[6:] + [(213, 37, "rs")]
# (len, gpu_family.pitch_of mode): len % 32 == 0 under a longer pitch, whose
# bytes in [len, pitch) are sentinels; a 16-byte body with a byte tail; rows one
# byte off the allocation's alignment, every column on the byte path
LAYOUTS = [(4128, "plus48"), (4096 + 17, "tail"), (4128, "mis1")]
BLOCKS = 4


def plan(k, e, L, block):
    rng = np.random.default_rng(1000 * k + 10 * e + block)
    x = lambda: int(rng.integers(1, 256))  # noqa: E731
    data = lambda n: [int(r) for r in rng.choice(k, n, replace=False)]  # noqa: E731
    par = lambda lo: k + int(rng.integers(lo, e))  # noqa: E731
    d = data(2)
    out = [
        ("one", 3, [(d[0], x())]),
        ("one", 40, [(par(0), x())]),
        ("data+data", 100, [(d[0], x()), (d[1], x())]),
        ("data+parity", 205, [(data(1)[0], x()), (par(2), x())]),
        ("data+parity0", 310, [(data(1)[0], x()), (k, x())]),
        ("data+parity1", 415, [(data(1)[0], x()), (k + 1, x())]),
        ("parity01", 520, [(k, x()), (k + 1, x())]),
        ("parity+parity", 625, [(k + 2, x()), (k + e - 1, x())]),
        ("parity0+parity", 626, [(k, x()), (par(2), x())]),
        ("three", 730, [(r, x()) for r in data(3)]),
        ("three", 731, [(data(1)[0], x()), (k, x()), (k + e - 1, x())]),
        # two columns of one 16-byte group
        ("data+data", 1024 + 2, [(r, x()) for r in data(2)]),
        ("data+parity", 1024 + 9, [(data(1)[0], x()), (par(0), x())]),
        # two 16-byte groups of one wave's 64
        ("data+data", 2048 + 16 + 5, [(r, x()) for r in data(2)]),
        ("data+parity", 2048 + 7 * 16 + 1, [(data(1)[0], x()), (par(0), x())]),
        # one 16-byte group; on the byte path two lanes of one wave
        ("data+data", 3000, [(r, x()) for r in data(2)]),
        ("parity+parity", 3007, [(k + 1, x()), (k + e - 2, x())]),
        # the row's end: its last column (the byte tail where there is one)
        ("one", L - 2, [(data(1)[0], x())]),
        ("data+data", L - 1, [(0, x()), (k - 1, x())]),
    ]
    return out


def scattered(k, e, L, rows=12):
    """Damage in `rows` distinct rows, two of them per column, the pairs
    chained so that the block's syndrome columns span `rows` - 1 dimensions
    or more: [(column, [(row, x)])]."""
    rng = np.random.default_rng(77 * k + e)
    pool = [int(r) for r in rng.choice(k + e, rows, replace=False)]
    cols = [int(i) for i in rng.choice(L, rows, replace=False)]
    return [(cols[n], [(pool[n], int(rng.integers(1, 256))), (pool[(n + 1) % rows], int(rng.integers(1, 256)))])
            for n in range(rows)]


def band_pairs(k, e):
    """k > 64: one bad column per pair of rows around the edges of the 64-row
    bands of the data rows, [(column, [(ra, x), (rb, y)])] with ra < rb: data
    pairs inside a band, across neighbouring bands and across distant ones,
    pairs of a data and a parity row, and past 128 and 192 rows the same
    around those edges.  Some pairs coincide at small k; each keeps its
    column."""
    last = (k - 1) // 64 * 64
    pairs = [(0, 64), (63, 64), (64, 65), (1, k - 1), (last - 1, last), (k - 2, k - 1),
             (64, k), (k - 1, k), (k - 1, k + 1), (last, k + e - 1), (65, k + 2)]
    if k > 128:
        pairs += [(127, 128), (128, 129), (70, 130)]
    if k > 192:
        pairs += [(191, 192), (5, 200), (130, k - 1)]
    assert all(0 <= a < b < k + e for a, b in pairs)
    rng = np.random.default_rng(31 * k + e)
    return [(7 + 233 * n, [(a, int(rng.integers(1, 256))), (b, int(rng.integers(1, 256)))])
            for n, (a, b) in enumerate(pairs)]


def three_bands(k):
    """(245, 5): a column damaged in three data rows of three different bands,
    which no row and no pair explains (the code's distance is 6), and beside
    it a column damaged in the last data row alone: [(column, [(row, x)])]."""
    return [(2050, [(10, 0x1D), (100, 0x72), (200, 0xE3)]), (2051, [(k - 1, 0x4C)])]


def dependent_matrix():
    """A locatable (12, 6) matrix that is not MDS, made from the Cauchy one:
    h_3 = h_0 + 2 h_1 + 3 h_2, so that h_0 + 2 h_1 is also h_3 + 3 h_2, and
    h_4 = 5 h_5 + 7 u_2 + 9 u_0 (u_p: parity row k + p), so that 5 h_5 + 7 u_2
    is also h_4 + 9 u_0."""
    import scrub_model as sm
    c = sm.cauchy_matrix(12, 6).copy()
    c[:, 3] = c[:, 0] ^ sm.MUL[c[:, 1], 2] ^ sm.MUL[c[:, 2], 3]
    c[:, 4] = sm.MUL[c[:, 5], 5]
    c[2, 4] ^= 7
    c[0, 4] ^= 9
    assert sm.locatable(c)
    return c


def dependent_wide_matrix():
    """The same at (129, 7), for the data-pair search's walk over the bands of
    64 rows (WIDE_DEPENDENCIES): h_3 in the plane of h_0, h_1, h_2 (both pairs
    in the first band, so the walk stops after it), h_100 in that of h_5, h_6,
    h_70 (a pair in the first band and one in the second, found by two lanes
    on different trips) and h_128 in that of h_64, h_65, h_127 (the second
    band and the third, which has one row)."""
    import scrub_model as sm
    c = sm.cauchy_matrix(129, 7).copy()
    for d, r0, r1, r2, f, g in WIDE_DEPENDENCIES:
        c[:, d] = c[:, r0] ^ sm.MUL[c[:, r1], f] ^ sm.MUL[c[:, r2], g]
    assert sm.locatable(c)
    return c


# h_d = h_r0 + f h_r1 + g h_r2 as (d, r0, r1, r2, f, g); f and g are the first
# factors from 2 on with which every entry of the matrix stays non-zero and
# the matrix locatable, one dependency after the other
WIDE_DEPENDENCIES = [(3, 0, 1, 2, 2, 5), (100, 5, 6, 70, 2, 4), (128, 64, 65, 127, 2, 4)]


def _mul(a, b):
    import scrub_model as sm
    return int(sm.MUL[a, b])


# columns of dependent_wide_matrix() that two pairs explain, each from either
# side (x h_r0 + f x h_r1 is also x h_d + g x h_r2), and two beside them that
# only their own pair explains
AMBIGUOUS_WIDE = [(50 + 2 * n + side, sorted([(r0, x), (r1, _mul(f, x))] if side == 0 else [(d, x), (r2, _mul(g, x))]))
                  for n, (d, r0, r1, r2, f, g) in enumerate(WIDE_DEPENDENCIES)
                  for side, x in ((0, 1 + 6 * n), (1, 0x35 + n))]
UNIQUE_WIDE = [(80, [(0, 1), (1, 1)]), (2049, [(70, 1), (127, 1)])]

# columns of dependent_matrix() that two pairs explain, each from either side,
# and one beside them that only its own pair explains: (column, [(row, x)])
AMBIGUOUS = [(50, [(0, 1), (1, 2)]), (51, [(2, 3), (3, 1)]), (52, [(5, 5), (14, 7)]), (53, [(4, 1), (12, 9)]),
             (2049, [(0, 0x35), (1, 0x6A)])]
UNIQUE = [(54, [(0, 1), (1, 3)])]
