"""The codes, layouts and damage of the suites of rsgpu_correct_blocks
(tests/test_correct.py on the model, tests/test_gpu_correct.py on the device).
Not a test module.

plan(k, e, L, block) is what one block gets: [(kind, column, [(row, x)])].
The columns are chosen for k_correct_compare's walk: a thread owns a 16-byte
group of 16-byte aligned rows (a byte of unaligned ones), a wave 64 of them."""
import numpy as np

# (k, e, matrix): Cauchy for the MDS property; gf_gen_rs_matrix shapes that the
# model corrects in every planned one- and two-row column (test_correct.py);
# k + e > 64 rows; a lane per syndrome used up (e = 64)
SHAPES = [(6, 5, "cauchy"), (12, 6, "cauchy"), (16, 8, "rs"), (20, 7, "rs"), (64, 32, "rs"), (8, 64, "cauchy")]
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


# columns of dependent_matrix() that two pairs explain, each from either side,
# and one beside them that only its own pair explains: (column, [(row, x)])
AMBIGUOUS = [(50, [(0, 1), (1, 2)]), (51, [(2, 3), (3, 1)]), (52, [(5, 5), (14, 7)]), (53, [(4, 1), (12, 9)]),
             (2049, [(0, 0x35), (1, 0x6A)])]
UNIQUE = [(54, [(0, 1), (1, 3)])]
