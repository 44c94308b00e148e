"""The cases of the batched ec_encode_data suite (tests/test_gpu_ec_batch.py;
rsgpu_ec_encode_data_batch, include/rsgpu.h) and what both suites derive from
them on the host: the matrices, where every row of every block lies in one
arena (tests/footprint.py), the device tables, and the expected bytes from
the project's oracle.  Not a test module; tests/test_ec_batch_api.py asserts on
this list alone that it covers every program layout, every class of length
and every kind of block.

One call carries 14 blocks, block b of LENGTHS[b] bytes:
    block 0         length 0, every pointer null
    blocks 3, 9     one source row one byte past its alignment (byte kernel)
    block 5         one output row eight bytes past its alignment (byte kernel)
    blocks 11, 12   share their first source row (12's; 11 reads its head)
The rows are laid into the arena in seeded random order, each behind a guard
band.  The source bytes are the arena's own noise."""
import functools

import numpy as np

import footprint as fp

# (k, rows): one per layout of the generated program, k off the chunk sizes
GEOMS = [(4, 2), (13, 16), (7, 18), (9, 22), (11, 27), (6, 40), (5, 64), (3, 70), (1, 1)]
# (k, rows, kind of matrix)
CASES = [
    (4, 2, "rs"), (4, 2, "decode"), (13, 16, "cauchy"), (13, 16, "random"), (7, 18, "random"), (9, 22, "rs"),
    (11, 27, "cauchy"), (11, 27, "decode"), (6, 40, "random"), (5, 64, "rs"), (3, 70, "cauchy"), (1, 1, "rs"),
]
LENGTHS = [0, 1, 31, 32, 33, 2016, 2047, 2048, 2080, 4096, 6144, 6145, 8192 + 17, 10240]
MAX_LENS = (max(LENGTHS), 16384)  # the largest length; a grid with workgroups past every block
NULL_BLOCK = 0
SRC_OFF1 = (3, 9)
OUT_OFF8 = (5,)
SHARED = (11, 12)
# the aligned32 call: the blocks that keep the promise, then one that breaks
# it by its length and one by a pointer
ALIGNED32_KEEP = (0, 7, 8, 10, 13)
ALIGNED32_BREAK = (4, 9)
TILE = 2048


def layout_of(rows):
    """The layout the shared program of `rows` rows runs in (csrc/rs_jit.hip
    jitw_rows, jitw_layout; csrc/rs_jit.h wide_passes)."""
    if rows <= 16:
        return "8-row"
    if rows > 64:
        return "passes"
    if rows > 32:
        return "4-wave"
    return "2x16" if rows > 24 else "2x12" if rows > 20 else "2x10"


def chunk_sources(rows):
    """Sources per LDS chunk of that layout (csrc/rs_jit.h Wide<R, CS>; 8 in the
    8-row layout): 5 for waves of 10 rows, else 6."""
    if rows <= 16:
        return 8
    per_pass = rows if rows <= 64 else rows // ((rows + 63) // 64)
    waves = 4 if per_pass > 32 else 2
    return 5 if (per_pass + waves - 1) // waves <= 10 else 6


def passes_of(rows):
    """Launches of the program per call."""
    if rows <= 16:
        return 1
    return (rows + 63) // 64 if rows > 64 else 1


def length_classes(n):
    """What a block of n bytes exercises, with two tiles per workgroup."""
    lo = n & ~31
    tiles = (lo + TILE - 1) // TILE
    tags = set()
    if n == 0:
        tags.add("empty")
    if 0 < n < 32:
        tags.add("tail only")
    if n == 32:
        tags.add("one lane")
    if lo and n > lo:
        tags.add("lanes and a tail")
    if lo and lo % TILE:
        tags.add("partial tile")
    if lo and lo % TILE == 0:
        tags.add("whole tiles")
    if lo % TILE == TILE - 32 and n > lo:
        tags.add("tail against the tile edge")
    if tiles > 1 and tiles % 2:
        tags.add("odd tile count")
    if tiles > 1 and tiles % 2 and lo % TILE == 0:
        tags.add("idle trailing tile")
    return tags


def block_kind(b):
    if b == NULL_BLOCK:
        return "null"
    if b in SRC_OFF1:
        return "source+1"
    if b in OUT_OFF8:
        return "output+8"
    if b in SHARED:
        return "shared source"
    return "plain"


def gf_matmul(orc, a, b):
    """a (n x m) times b (m x p) over GF(2^8)."""
    out = np.zeros((a.shape[0], b.shape[1]), np.uint8)
    for i in range(a.shape[0]):
        for j in range(b.shape[1]):
            v = 0
            for t in range(a.shape[1]):
                v ^= orc.gf_mul(int(a[i, t]), int(b[t, j]))
            out[i, j] = v
    return out


def decode_setup(k, rows, orc):
    """A stripe of the [I; Cauchy] code of k data rows among m = k + rows that
    has lost `rows` of them: returns (enc m x k, lost, survivors, inverse of
    enc[survivors], decode matrix rows x k).  Decode row i rebuilds lost[i]
    from the k survivors: the inverse's row of a lost data row, the encode row
    times the inverse for a lost parity row (the reference's
    gf_gen_decode_matrix)."""
    m = k + rows
    enc = orc.gen_cauchy1_matrix(m, k)
    rng = np.random.default_rng(100 * k + rows)
    nd = max(1, min(k, rows) // 2)  # lost data rows; the other lost rows are parity rows
    lost = np.sort(np.concatenate([rng.choice(k, nd, replace=False), k + rng.choice(rows, rows - nd, replace=False)]))
    surv = np.array([r for r in range(m) if r not in set(lost.tolist())])
    assert len(surv) == k
    rc, inv = orc.invert_matrix(enc[surv])
    assert rc == 0
    dmat = np.stack([inv[r] if r < k else gf_matmul(orc, enc[r:r + 1], inv)[0] for r in lost])
    return enc, lost, surv, inv, np.ascontiguousarray(dmat, np.uint8)


def matrix(k, rows, kind, orc):
    """The rows x k matrix of a case."""
    if kind == "rs":
        return np.ascontiguousarray(orc.gen_rs_matrix(k + rows, k)[k:])
    if kind == "cauchy":
        return np.ascontiguousarray(orc.gen_cauchy1_matrix(k + rows, k)[k:])
    if kind == "decode":
        return decode_setup(k, rows, orc)[4]
    assert kind == "random"
    rng = np.random.default_rng(7 * k + rows)
    c = rng.integers(0, 256, (rows, k), dtype=np.uint8)
    flat = c.reshape(-1)
    flat[rng.choice(flat.size, max(2, flat.size // 8), replace=False)] = 0
    flat[rng.choice(flat.size, max(2, flat.size // 8), replace=False)] = 1
    flat[0], flat[-1] = 0, 1
    return c


class Plan:
    """Where the rows of a (k, rows) call lie: one arena (a footprint.Arena,
    not yet allocated) with a region per row, the three tables and the status
    as flat regions; src[b][j] / out[b][r] name the regions (None: a null
    pointer)."""

    def __init__(self, k, rows, lengths=LENGTHS, seed=5, special=True):
        self.k, self.rows, self.lens = k, rows, list(lengths)
        self.B = B = len(self.lens)
        self.lay = lay = fp.Arena()
        self.src = [[None] * k for _ in range(B)]
        self.out = [[None] * rows for _ in range(B)]
        todo = []
        for b, n in enumerate(self.lens):
            if special and b == NULL_BLOCK:
                assert n == 0
                continue
            for j in range(k):
                if special and b == SHARED[0] and j == 0:
                    continue  # the other block's row
                todo.append(("s", b, j, 1 if special and b in SRC_OFF1 and j == k - 1 else 0))
            for r in range(rows):
                todo.append(("o", b, r, 8 if special and b in OUT_OFF8 and r == rows // 2 else 0))
        order = np.random.default_rng(seed).permutation(len(todo))
        lay.flat("status", 4 * B)
        for i in order:
            kind, b, i2, off = todo[i]
            name = f"{kind}{b}_{i2}"
            lay.rows(name, 1, 1, max(self.lens[b], 1), self.lens[b], off)
            (self.src if kind == "s" else self.out)[b][i2] = name
        if special:
            assert self.lens[SHARED[0]] <= self.lens[SHARED[1]]
            self.src[SHARED[0]][0] = self.src[SHARED[1]][0]
        lay.flat("data_tab", 8 * B * k)
        lay.flat("coding_tab", 8 * B * rows)
        lay.flat("len_tab", 4 * B)

    def addr(self, name, base=0):
        return 0 if name is None else base + self.lay[name].start

    def tables(self, base, blocks=None, lens=None):
        """(data [n, k], coding [n, rows]) uint64 and lens int32 [n] of the
        blocks `blocks` (all of them: None) of an arena at address `base`."""
        bl = range(self.B) if blocks is None else blocks
        d = np.array([[self.addr(s, base) for s in self.src[b]] for b in bl], np.uint64).reshape(len(bl), self.k)
        c = np.array([[self.addr(o, base) for o in self.out[b]] for b in bl], np.uint64).reshape(len(bl), self.rows)
        n = np.array([self.lens[b] for b in bl] if lens is None else lens, np.int32)
        return d, c, n

    def aligned(self, b):
        return all(self.addr(n) % 16 == 0 for n in self.src[b] + self.out[b])

    def written(self, blocks, lens=None):
        """[0, len) of every output row of `blocks`: what a call may write."""
        out = []
        for i, b in enumerate(blocks):
            n = self.lens[b] if lens is None else lens[i]
            if n > 0:
                out += [(self.lay[o].start, self.lay[o].start + n) for o in self.out[b]]
        return out

    def expected(self, c, noise, orc, blocks=None):
        """{(b, r): bytes} of every output row, from the oracle block by block;
        noise: the arena's bytes before the call."""
        g = orc.init_tables(self.k, self.rows, c)
        want = {}
        for b in (range(self.B) if blocks is None else blocks):
            n = self.lens[b]
            outs = [np.zeros(n, np.uint8) for _ in range(self.rows)]
            if n:
                srcs = [np.ascontiguousarray(noise[self.lay[s].start: self.lay[s].start + n]) for s in self.src[b]]
                orc.encode_data(n, self.k, self.rows, g, srcs, outs)
            for r in range(self.rows):
                want[(b, r)] = outs[r]
        return want


@functools.lru_cache(maxsize=None)
def plan(k, rows):
    return Plan(k, rows)
