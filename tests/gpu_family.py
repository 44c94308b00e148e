"""What the GPU suites of the scrub family share (tests/test_gpu_scrub.py,
test_gpu_repair.py, test_gpu_update.py, test_gpu_degraded.py,
test_gpu_rebuild.py): the context of a module, synthetic blocks and their
parity on the device, the timing records of a call, the comparison of reports
with a model's tuples, and the
stripes, lists and damage of the degraded scrub, which the rebuild suite runs
on as well.  Not a test module; the suites import torch before they import
this one."""
import numpy as np
import torch

import degraded_model as dm
import rsgpu
import scrub_model as sm

SCRUB_FIELDS = ("bad_columns", "status", "row")
REPAIR_FIELDS = ("bad_columns", "repaired_columns", "status", "row")
SCRUB_DT = rsgpu.SCRUB_REPORT_DTYPE
POISON = 0xA5  # a report buffer before the call


def device_context(reset_scrub_kernel=False):
    """The body of a suite's module-scoped `ctx` fixture."""
    assert torch.cuda.is_available(), "GPU test needs a HIP device"
    c = rsgpu.Context(0)
    c.set_torch_stream()
    yield c
    torch.cuda.synchronize()
    if reset_scrub_kernel:
        c.set_scrub_kernel("auto")
    c.close()


def recorded(ctx, call, blocks=False):
    """The names of the timing records that call() leaves, in order; with
    `blocks`, (name, blocks) per record."""
    ctx.timing_enable(True)
    try:
        ctx.timing_read()
        call()
        return [(n, b) if blocks else n for n, _, b in ctx.timing_read()]
    finally:
        ctx.timing_enable(False)


def matrix(k, e, kind):
    return sm.rs_matrix(k, e) if kind == "rs" else sm.cauchy_matrix(k, e)


def pitch_of(L, mode):
    """eq: pitch == len; plus48: len + 48; mis1: rows one byte past the
    allocation's alignment; tail: a 16-byte aligned pitch around a len that
    is no multiple of 16 (vector body, byte tail)."""
    if mode == "plus48":
        return L + 48, 0
    if mode == "mis1":
        return L, 1
    if mode == "tail":
        return (L + 255) // 256 * 256, 0
    return L, 0


def same(rep, want, fields=SCRUB_FIELDS):
    """rep: structured reports; want: the model's tuples of `fields`."""
    got = [tuple(int(r[f]) for f in fields) for r in rep]
    assert got == [tuple(w) for w in want], [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != tuple(w)]


class DeviceBlocks:
    """B synthetic blocks and their parity on the device.  Every allocation is
    filled with 0x6B first, so the padding is not zero; `offset`: rows that
    start that many bytes past the allocation's alignment.  coef is None for
    the built-in RS matrix, c the matrix either way."""

    def __init__(self, ctx, k, e, L, B, pitch, offset=0, kind="rs", c=None, seed=11, encode=True):
        self.ctx, self.k, self.e, self.L, self.B, self.pitch, self.offset = ctx, k, e, L, B, pitch, offset
        self.c = matrix(k, e, kind) if c is None else np.ascontiguousarray(c, np.uint8)
        self.coef = None if kind == "rs" and c is None else self.c
        self.dev = torch.device("cuda", 0)
        self.src_all, self.par_all = self.alloc(k), self.alloc(e)
        self.src, self.par = self.src_all[offset:], self.par_all[offset:]
        ctx.fill_synthetic(self.src, B * k, L, pitch, seed, 0)
        if encode:
            ctx.encode_blocks(k, e, L, pitch, B, self.src, self.par, coef=self.coef)

    def alloc(self, rows):  # at least a byte, so that the pointer is not null
        t = torch.empty(max(1, self.B * rows * self.pitch) + self.offset, dtype=torch.uint8, device=self.dev)
        t.fill_(0x6B)
        return t

    def view(self, t, rows):
        return t[: self.B * rows * self.pitch].view(self.B, rows, self.pitch)

    def rows(self, row):
        """[B, L] view of row `row` (source, or parity from k on) of every block."""
        if row < self.k:
            return self.view(self.src, self.k)[:, row, : self.L]
        return self.view(self.par, self.e)[:, row - self.k, : self.L]

    def row(self, blk, row):
        return self.rows(row)[blk]

    def xor(self, blk, row, col, x):
        self.rows(row)[blk, col] ^= x

    def snapshot(self):
        return self.src_all.clone(), self.par_all.clone()

    def host(self, t, rows):
        """[B, rows, L] of the rows of `t` on the host."""
        return self.view(t, rows)[:, :, : self.L].contiguous().cpu().numpy()

    def host_block(self, blk):
        s = self.view(self.src, self.k)[blk, :, : self.L].cpu().numpy()
        p = self.view(self.par, self.e)[blk, :, : self.L].cpu().numpy()
        return s, p


class DegradedStripe(DeviceBlocks):
    """B consistent synthetic blocks on the device, a list of lost rows per block."""

    def __init__(self, ctx, k, e, L, B, u, kind="rs", mode="eq", seed=11, c=None):
        pitch, offset = pitch_of(L, mode)
        super().__init__(ctx, k, e, L, B, pitch, offset, kind, c, seed)
        self.u = u
        self.lost = np.full((B, u), dm.NONE, np.uint8)
        self.rep = torch.empty(B * SCRUB_DT.itemsize, dtype=torch.uint8, device=self.dev)
        torch.cuda.synchronize()

    def fill_lost(self, seed):
        """Every listed row of every well-formed list: zero (seed None) or noise."""
        g = torch.Generator(device="cpu").manual_seed(seed or 0)
        for b in range(self.B):
            for r in dm.list_rows(self.lost[b], self.k, self.e) or []:
                if seed is None:
                    self.row(b, r).zero_()
                else:
                    self.row(b, r).copy_(torch.randint(0, 256, (self.L,), dtype=torch.uint8, generator=g))

    def scrub(self, locate=True):
        d_lost = torch.from_numpy(self.lost).to(self.dev)
        self.rep.fill_(POISON)
        before = self.src_all.clone(), self.par_all.clone()
        self.ctx.scrub_degraded_blocks(self.k, self.e, self.L, self.pitch, self.B, self.src, self.par, self.u,
                                       d_lost, self.rep, coef=self.coef, locate=locate)
        torch.cuda.synchronize()
        assert torch.equal(self.src_all, before[0]), "source allocation written"
        assert torch.equal(self.par_all, before[1]), "parity allocation written"
        assert (d_lost.cpu().numpy() == self.lost).all(), "lists written"
        return self.rep.cpu().numpy().view(SCRUB_DT).copy()

    def model(self, orc, locate=True):
        """The model's reports on the blocks as they are on the device now."""
        hs = self.host(self.src, self.k)
        hp = self.host(self.par, self.e)
        g = orc.init_tables(self.k, self.e, self.c) if self.e else None
        out = []
        for b in range(self.B):
            syn = hp[b].copy()
            if self.e and self.L:
                calc = [np.zeros(self.L, np.uint8) for _ in range(self.e)]
                orc.encode_data(self.L, self.k, self.e, g, [np.ascontiguousarray(r) for r in hs[b]], calc)
                syn ^= np.stack(calc)
            out.append(dm.report_syn(self.c, syn, self.lost[b], locate))
        return out


def mixed_lists(k, e, u, B, seed=5):
    """Per block n = b mod (min(u, e) + 1) lost rows, n == e included where u
    allows; data only, parity only and both by turns; block 0 holds the first
    rows, block 1 the last ones."""
    rng = np.random.default_rng(seed)
    nmax = min(u, e)
    lost = np.full((B, u), dm.NONE, np.uint8)
    for b in range(B):
        n = b % (nmax + 1) if B > 1 else min(nmax, max(1, e - 2))
        kind = (b // (nmax + 1)) % 3
        if kind == 0:  # data only
            rows = rng.choice(k, min(n, k), replace=False)
        elif kind == 1:  # parity only
            rows = k + rng.choice(e, n, replace=False)
        else:
            rows = rng.choice(k + e, n, replace=False)
        lost[b] = dm.pad(np.sort(rows), u)
    if B > 2:
        n = min(nmax, max(1, e - 2))
        lost[0] = dm.pad(np.arange(n), u)
        lost[1] = dm.pad(np.arange(k + e - n, k + e), u)
    return lost


def band_members(k, e):
    """The rows around the 64-row bands of a wave's strided loops that a
    (k, e) block has: both sides of every band's edge, the last data row, the
    first parity row, the parity rows 63 and 64, the last row."""
    want = (63, 64, 65, 127, 128, 129, 191, 192, k - 1, k, k + 63, k + 64, k + e - 1)
    return sorted({r for r in want if 0 <= r < k + e})


def band_lists(k, e, u, B):
    """The lists of blocks 2..5 of a wide case, (4, u): each min(u, e) - 1 of
    band_members (all of them where there are fewer), ascending, dealt out so
    that a list has rows of several bands and the four hold every member."""
    assert B >= 6
    have = band_members(k, e)
    n = min(min(u, e) - 1, len(have))
    assert 1 <= n and 4 * n >= len(have)
    out = np.full((4, u), dm.NONE, np.uint8)
    for i in range(4):
        rows = have[i::4]
        rows += [r for r in have[i + 1:] + have[:i] if r not in rows]
        out[i] = dm.pad(sorted(rows[:n]), u)
    assert {int(r) for r in out.ravel()} - {dm.NONE} == set(have)
    return out


def wide_lists(k, e, u, B):
    """mixed_lists with band_lists in blocks 2..5."""
    lost = mixed_lists(k, e, u, B)
    lost[2:6] = band_lists(k, e, u, B)
    return lost


def wide_row(k, e):
    """The row of a wide case's deliberate ONE_ROW block: the last data row
    where k > 64, the last parity row where only e is."""
    return max(64, k - 1) if k > 64 else k + e - 1


def wide_plan(lost, k, e, L):
    """The deliberate damage of a wide case, [(block, row, column, x)], and
    its two blocks, both among the blocks 0..4 that damage() leaves alone: one
    byte of wide_row in the first of 2, 3, 4, 0 whose list does not hold it
    (ONE_ROW; block 0 lists the first rows), and in another one a byte of its
    first and of its last survivor, in different columns (DAMAGED)."""
    row = wide_row(k, e)
    one = next(b for b in (2, 3, 4, 0) if row not in dm.list_rows(lost[b], k, e))
    two = next(b for b in range(2, 5) if b != one)
    surv = [r for r in range(k + e) if r not in dm.list_rows(lost[two], k, e)]
    return [(one, row, L // 2, 0x5A), (two, surv[0], 1, 0x21), (two, surv[-1], L - 1, 0x84)], one, two


def wide_damage(st, seed=9):
    """damage(), whose kind is 0 in blocks 0..4 (min(u, e) >= 4), then
    wide_plan; returns wide_plan's two blocks."""
    assert min(st.u, st.e) >= 4
    damage(st, seed)
    hits, one, two = wide_plan(st.lost, st.k, st.e, st.L)
    for b, row, col, x in hits:
        st.xor(b, row, col, x)
    torch.cuda.synchronize()
    return one, two


def damage(st, seed=9):
    """Block b gets damage kind (b // (min(u, e) + 1)) mod 7, so that every
    kind meets every n: none; one byte of a survivor; one survivor in several
    columns, the first and the last included; two survivors in different
    columns; two survivors in one column; a byte of the first surviving parity
    row (a pivot row when data rows are lost); a byte of the last surviving
    parity row (a rest row)."""
    rng = np.random.default_rng(seed)
    k, e, L = st.k, st.e, st.L
    nmax = min(st.u, e)
    for b in range(st.B):
        lost = dm.list_rows(st.lost[b], k, e) or []
        surv = [r for r in range(k + e) if r not in lost]
        spar = [r for r in surv if r >= k]
        kind = (b // (nmax + 1)) % 7 if st.B > 1 else 2
        x = lambda: int(rng.integers(1, 256))  # noqa: E731
        pick = lambda n: [int(r) for r in rng.choice(surv, n, replace=False)]  # noqa: E731
        if kind == 1:
            st.xor(b, pick(1)[0], int(rng.integers(0, L)), x())
        elif kind == 2:
            r = pick(1)[0]
            for col in sorted({0, L - 1, L // 2, (L // 3) | 1 if L > 1 else 0, min(17, L - 1)}):
                st.xor(b, r, col, x())
        elif kind == 3:
            r1, r2 = pick(2)
            st.xor(b, r1, 0, x())
            st.xor(b, r2, L - 1 if L > 1 else 0, x())
        elif kind == 4:
            r1, r2 = pick(2)
            col = int(rng.integers(0, L))
            st.xor(b, r1, col, x())
            st.xor(b, r2, col, x())
        elif kind == 5 and spar:
            st.xor(b, spar[0], int(rng.integers(0, L)), x())
        elif kind == 6 and spar:
            st.xor(b, spar[-1], int(rng.integers(0, L)), x())
    torch.cuda.synchronize()


# codes (5, 4) (16, 4) (20, 7) (64, 32) RS and Cauchy (10, 4); len in {1, 31,
# 32, 2080, 4176} and 4099 (a 16-byte body with a 3-byte tail); the three
# pitches; blocks in {1, 67}; u in {1, 2, 4, 8}.  WIDE_CASES below: more than
# 64 source rows, (65, 6) (129, 9) (245, 5) Cauchy and (100, 20) (213, 37) RS,
# and more than 64 parity rows, (9, 70) RS
CASES = [
    (5, 4, "rs", 4176, 67, 4, "plus48"),
    (5, 4, "rs", 1, 67, 1, "eq"),
    (5, 4, "rs", 31, 67, 2, "eq"),
    (5, 4, "rs", 4099, 67, 2, "tail"),
    (16, 4, "rs", 32, 67, 8, "eq"),
    (16, 4, "rs", 2080, 1, 2, "plus48"),
    (16, 4, "rs", 2080, 67, 4, "mis1"),
    (20, 7, "rs", 4176, 67, 8, "eq"),
    (20, 7, "rs", 31, 1, 4, "plus48"),
    (64, 32, "rs", 2080, 67, 8, "eq"),
    (64, 32, "rs", 4176, 1, 1, "plus48"),
    (64, 32, "rs", 32, 67, 2, "mis1"),
    (10, 4, "cauchy", 2080, 67, 4, "plus48"),
    (10, 4, "cauchy", 4176, 1, 8, "eq"),
    (10, 4, "cauchy", 1, 1, 1, "mis1"),
]

# more rows than a wave has lanes, where the strided loops of the prepare
# kernels (for r = lane; r < k; r += 64) take a second, ragged trip; lists
# from wide_lists, damage from wide_damage
WIDE_CASES = [
    (65, 6, "cauchy", 2080, 67, 4, "plus48"),  # one lane on the second trip
    (100, 20, "rs", 2080, 67, 8, "eq"),        # the C5 code
    (129, 9, "cauchy", 4099, 23, 8, "tail"),   # three trips, the last with one lane; byte tail
    (213, 37, "rs", 2080, 23, 8, "mis1"),      # the scrub's and the repair's large shape, byte kernels
    (245, 5, "cauchy", 2080, 23, 4, "eq"),     # k + e = 250 = RSGPU_MAX_SOURCES
    (9, 70, "rs", 2080, 23, 8, "plus48"),      # e > 64: more than 64 rest rows in the degraded prepare
]
