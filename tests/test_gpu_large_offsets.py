"""64-bit addressing on the GPU: buffers, pitches and rows beyond 4 GiB.

Every other GPU suite keeps every byte offset below 2^32; the shape the
project exists for (C3: 1024 blocks x 96 rows x 1 MB in one call) does not.
Here the address space is large and the work small: rows of a few KB at a
pitch of 1 MiB + 64 in a thousand blocks (deep), or two or three blocks at a
pitch of 2^31 + 64 down to 2^28 + 64 (wide), so that a call moves a few MB
while its buffers span 4 to 16 GiB (tests/large_offset_cases.py has the
geometries and, in tests/test_large_offset_cases.py, the proof by arithmetic
that a 32-bit block base, row index, row * pitch or int pitch at these shapes
reads or writes a byte these tests compare).

What is compared: [0, len) of every row of every block with the oracle
(encode, decode, the row-pointer batch) or with the numpy model of the call's
contract, on the host; every other byte of every allocation with the 0x6B
fill it started from, on the device.  Damage and lists sit in the first and
the last block and in the block whose rows straddle byte 2^32 of the source or
of the parity buffer and its two neighbours.  Each test names the kernel it
means and reads it back from the call's timing records.

The flat tiling of the compiled encode runs on both sides of its guard, with
lane offsets past 2^31 and up to 2^32 (flat); rows longer than 2^31 bytes are
compared with a periodic reference, and rows longer than RSGPU_MAX_LEN must be
refused with nothing written (long).

Memory: no test holds more than 24 GiB (room(), the one place that may skip);
a context lives for one test, so its scratch goes with it.

The 32-bit offsets of csrc/ and the test that takes each to its upper range:
  bitslice.h glds32 / glds32_nt (SGPR base + 32-bit VGPR offset, unsigned)
      every caller below
  rs_bitsliced.hip run_group (uint32_t)loff: k_rs_bs and the fused scrub,
  repair, locate, degraded and correct kernels built on it
      flat tiles, db * K * pitch + o up to 4.1e9: test_flat_edge[64-16-32-70-*]
      inside a row, 2^31 + 2080: test_long_rows_encode[5-4-compiled],
      test_long_rows_scrub[5-4-rs-fused]; nine rows of 4 GiB do not fit 24 GiB
  rs_bitsliced.hip tile_pos (int x, int L; len < 65536 by the flat guard) and
  launch()'s guard (2048 / len + 2) * K * pitch < 2^32
      both sides and the first pitch at which flat tiles would pass 2^32:
      test_flat_edge.  (5, 4) at the block counts the guard is checked with
      runs k_rs_bs_split on per-block tiles: the (64, 16) cases reach the guard
  rs_tc.hip (uint32_t)loff: k_rs_tc, k_rs_tc_split, k_rs_tc_fused
      2^32 - 32: test_long_rows_encode[2-2-threaded-*],
      test_long_rows_decode[one_matrix-*]
  rs_jit.hip (uint32_t)loff / inb ? (uint32_t)off : 0u: k_rs_jit and the
  generated scrub, repair, locate and correct epilogues
      2^32 - 32: test_long_rows_encode[2-2-generated-*],
      test_long_rows_decode[generated-*]; 2^31 + 2080:
      test_long_rows_scrub[2-2-cauchy-generated].
      k_rs_jitw and k_rs_kara (e > 16) share the operand; 17 rows of 2 GiB do
      not fit 24 GiB, their row addresses are covered by deep and wide
  rs_jit.hip batch_past (unsigned compare): the lengths of the row-pointer
  batch are ints, below 2^31 by the call's types
  the launchers' len < 2^32 guards (rsgpu_scrub.cpp fused_rows, generated_rows,
  the threaded rebuild; rs_bitsliced.hip family_rows; rs_jit.hip): unreachable
  behind check_geom now, test_rows_beyond_the_limit_are_refused_everywhere

Mutations, none built or run; the byte each would touch is computed in
tests/test_large_offset_cases.py and is one these tests compare:
  rs_update.hip `a.upd + b * a.u * a.pitch` (and src, par) in unsigned: from
      block 820 / 1024 on every row is a row of an earlier block ->
      test_update[deep-*] (test_deep_mutations_land_in_compared_bytes)
  rs_kernels.hip k_row_ptrs `base + i * pitch` in 32 bits: the same for every
      kernel on row pointers -> test_encode[deep-*-generated / threaded /
      karatsuba], the generated scrub family, test_decode (row_index_u32)
  a 32-bit row * pitch beside a 64-bit block base: row 4 of a (5, 4) block at
      pitch 2^30 + 64 is its row 0 at column 256 -> every wide30 case
  an int pitch: negative at 2^31 + 64, leaves the buffer (a fault, not a
      wrong byte) -> the wide31 cases, which every call has in its form for
      any (k, e) (two-pass, lanes, threaded, generated, k_dot_generic); the
      compiled and fused kernels start at (5, 4), whose two blocks fit the
      cap up to 2^30 + 64, and correct's two-pass form needs e >= 3 (26 GiB)
  launch()'s flat guard widened by 2: flat tiles at pitch 1065248 read an earlier
      block's bytes -> test_flat_edge[64-16-32-70-1065248-False]"""
import gc
from typing import NamedTuple

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import correct_model as cm  # noqa: E402
import degraded_model as dm  # noqa: E402
import gpu_family as gf  # noqa: E402
import large_offset_cases as lo  # noqa: E402
import locate_model as lm  # noqa: E402
import rebuild_model as rbm  # noqa: E402
import repair_model as rm  # noqa: E402
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402
import update_model as um  # noqa: E402
from oracle_lib import Oracle  # noqa: E402

T31, T32, FILL = lo.T31, lo.T32, lo.FILL
GiB = 1 << 30
SDT, RDT, CDT = rsgpu.SCRUB_REPORT_DTYPE, rsgpu.REPAIR_REPORT_DTYPE, rsgpu.CORRECT_REPORT_DTYPE
N = dm.NONE
POISON = gf.POISON


@pytest.fixture
def ctx():
    """A context per test: what a call leaves in it (up to 4 GiB of two-pass
    scratch at the wide pitch) is freed with it."""
    torch.cuda.reset_peak_memory_stats()
    yield from gf.device_context()
    print(f"large offsets: peak of the test's tensors {torch.cuda.max_memory_allocated() / GiB:.2f} GiB")
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def room(need):
    """The one place that may skip: `need` bytes of device memory, at most
    lo.CAP, against what the device has free now."""
    free, total = torch.cuda.mem_get_info()
    print(f"large offsets: need {need / GiB:.2f} GiB, free {free / GiB:.2f} of {total / GiB:.2f} GiB")
    assert need <= lo.CAP, need
    if free < need + GiB:
        pytest.skip(f"needs {need / GiB:.1f} GiB of device memory, {free / GiB:.1f} free")


class Geo(NamedTuple):
    name: str
    k: int
    e: int
    kind: str
    L: int
    B: int
    pitch: int
    offset: int

    def __str__(self):
        return self.name

    def bytes(self, rows):
        return self.B * rows * self.pitch + self.offset

    def check(self, extra=()):
        """The arithmetic the geometry stands for."""
        k, e, p, B = self.k, self.e, self.pitch, self.B
        assert p >= self.L and p % 16 == 0 and p & (p - 1) != 0
        wide31 = self.name.startswith("wide31")
        if wide31:  # the pitch itself does not fit a signed int
            assert p >= T31 and B == 2
        for rows in (k, e) + tuple(extra):
            if wide31 and rows == 1:
                # one row per block: the buffer ends at 2 p = 2^32 + 128, and
                # what the case pins there is the pitch
                assert B * p > T32
                continue
            # the last block's rows lie wholly past byte 2^32 of their buffer
            assert lo.row_offset(B - 1, 0, rows, p) >= T32, (self.name, rows)
            s = lo.straddler(rows, p)
            assert s < B - 1 and lo.row_offset(s, 0, rows, p) < T32 <= lo.row_offset(s + 1, 0, rows, p)
        if self.name.startswith("wide"):
            assert (k + e - 1) * p >= T31  # row * pitch inside one block is large, too
        return self


def deep(k, e, L, offset=0, kind="rs"):
    B = lo.deep_blocks(e)
    g = Geo(f"deep-{k}.{e}{kind[0]}-L{L}" + (f"+{offset}" if offset else ""), k, e, kind, L, B, lo.DEEP_PITCH, offset)
    assert B * e * g.pitch >= T32 + 2 * e * g.pitch
    return g


def wide(k, e, L, bits, B=2, kind="rs", offset=0):
    return Geo(f"wide{bits}-{k}.{e}{kind[0]}-L{L}x{B}" + (f"+{offset}" if offset else ""), k, e, kind, L, B,
               (1 << bits) + 64, offset)


def two_pass_scratch(g):
    """rsgpu_scrub.cpp two_pass: the computed parity of a slice of blocks."""
    per = g.e * g.pitch
    return 16384 + max(1, min(g.B, (128 << 20) // per)) * per


class Stripe(gf.DeviceBlocks):
    """gf.DeviceBlocks at a geometry, after room() has looked at the device."""

    def __init__(self, ctx, g, encode=True, more=0, extra=(), checked=True):
        if checked:
            g.check(extra)
        # the buffers, what the caller adds, and the largest temporary of the
        # device-side comparisons (whole(): one row index of every block, or
        # one row, as bools)
        room(g.bytes(g.k) + g.bytes(g.e) + more + (g.B * g.pitch if g.B * g.pitch <= 2 * GiB else g.pitch))
        super().__init__(ctx, g.k, g.e, g.L, g.B, g.pitch, g.offset, g.kind, encode=encode)
        self.g = g
        torch.cuda.synchronize()
        self.special = lo.special_blocks(g.k, g.e, g.pitch, g.B, extra)

    def hosts(self):
        return self.host(self.src, self.k), self.host(self.par, self.e)

    def buffer(self, rows):
        """Another [B][rows] buffer of this geometry, filled with FILL: (whole
        allocation, the rows from `offset` on)."""
        t = self.alloc(rows)
        return t, t[self.offset:]

    def whole(self, t_all, rows, want, what):
        """The whole allocation `t_all` of [B][rows] rows: [0, L) of every row
        is want (B, rows, L) from the host, every other byte is FILL."""
        B, L, p, off = self.B, self.L, self.pitch, self.offset
        v = self.view(t_all[off:], rows)
        if L and rows:
            w = torch.from_numpy(np.ascontiguousarray(want)).to(self.dev)
            if not torch.equal(v[:, :, :L], w):
                bad = (v[:, :, :L] != w).any(dim=2).nonzero()[:8].tolist()
                raise AssertionError(f"{what}: rows (block, row) differ from the model: {bad}")
        assert bool((t_all[:off] == FILL).all()) and bool((t_all[off + B * rows * p:] == FILL).all()), what
        for r in range(rows):
            for b in ([slice(None)] if B * p <= 2 * GiB else range(B)):
                assert bool((v[b, r, L:] == FILL).all()), f"{what}: padding of row {r} written"

    def unchanged(self, hs, hp):
        self.whole(self.src_all, self.k, hs, "source allocation")
        self.whole(self.par_all, self.e, hp, "parity allocation")


def syndromes(c, hs, hp):
    """sm.syndromes of every block at once: hs (B, k, L), hp (B, e, L)."""
    syn = hp.copy()
    for j in range(c.shape[1]):
        syn ^= sm.gf_mul(c[:, j][None, :, None], hs[:, j][:, None, :])
    return syn


def oracle_parity(orc, c, hs):
    """The oracle's parity of every block: hs (B, k, L) -> (B, e, L)."""
    B, k, L = hs.shape
    e = c.shape[0]
    g = orc.init_tables(k, e, np.ascontiguousarray(c))
    out = np.zeros((B, e, L), np.uint8)
    for b in range(B):
        rows = [out[b, i] for i in range(e)]
        orc.encode_data(L, k, e, g, [np.ascontiguousarray(r) for r in hs[b]], rows)
    return out


def damage(st, pairs=False, first=0):
    """Deliberate damage in every special block, a kind per block by turns:
    a byte of a source row; a parity row in three columns, the first and the
    last included; two rows in different columns; the last source row's first
    byte; with `pairs`, two rows in one column."""
    k, e, L = st.k, st.e, st.L
    kinds = 5 if pairs else 4
    hits = []
    for i, b in enumerate(st.special):
        kind = (i + first) % kinds
        if kind == 0:
            hits += [(b, i % k, L - 1, 0x5A)]
        elif kind == 1:
            r = k + i % e
            hits += [(b, r, 0, 0x01), (b, r, L // 2, 0x80), (b, r, L - 1, 0xC3)]
        elif kind == 2:
            hits += [(b, 0, 5, 0x21), (b, k + e - 1, L - 3, 0x9D)]
        elif kind == 3:
            hits += [(b, k - 1, 0, 0xFF)]
        else:
            hits += [(b, 1, 7, 0x17), (b, k, 7, 0xE0)]
    for b, r, col, x in hits:
        st.xor(b, r, col, x)
    torch.cuda.synchronize()
    return hits


def names_of(ctx, call, *want):
    """call() with its timing records read back: every name of `want` ran."""
    names = gf.recorded(ctx, call)
    torch.cuda.synchronize()
    for w in want:
        assert w in names, (w, names)
    return names


# ---- encode ---------------------------------------------------------------------

# (geometry, encode kernel, the record meant).  The kernels of 32-byte lanes
# take len = 4160 (two tiles and two lanes); 4176 = 4160 + 16 is the nibble
# kernel's, 4099 k_dot_generic's on vectors with a byte tail and on bytes.
# deep (5, 4): the compiled kernel on flat tiles (len % 2048 != 0) and on
# per-block tiles, the split kernel below 2048 (tile, block) pairs, the shared
# generated program, threaded code.
# wide: an int pitch or a 32-bit row * pitch; the compiled kernel there needs
# 2048 pairs in two blocks, so 1025 tiles per row.
ENCODE = [
    (deep(5, 4, 4160), "compiled", "k_rs_bs(encode)"),
    (deep(5, 4, 4096), "compiled", "k_rs_bs(encode)"),
    (deep(5, 4, 2016), "compiled", "k_rs_bs_split(encode)"),
    (deep(5, 4, 4160), "generated", "k_rs_jit(encode)"),
    (deep(5, 4, 4160), "threaded", "k_rs_tc(encode)"),
    (deep(5, 4, 4176), "compiled", "k_rs_encode_lh"),
    (deep(5, 4, 4099), "auto", "k_dot_generic"),
    (deep(5, 4, 4099, offset=1), "auto", "k_dot_generic"),
    (deep(10, 4, 4160, kind="cauchy"), "auto", "k_rs_jit(encode)"),
    (deep(64, 32, 2080), "karatsuba", "k_rs_jit(encode)"),
    (wide(2, 2, 4160, 31), "generated", "k_rs_jit(encode)"),
    (wide(2, 2, 4160, 31), "threaded", "k_rs_tc(encode)"),
    (wide(2, 2, 4099, 31, offset=1), "auto", "k_dot_generic"),
    (wide(5, 4, 4160, 30), "compiled", "k_rs_bs_split(encode)"),
    (wide(5, 4, 1024 * 2048 + 2080, 30), "compiled", "k_rs_bs(encode)"),
    (wide(64, 32, 4160, 26, B=3), "karatsuba", "k_rs_jit(encode)"),
]


@pytest.mark.parametrize("g,kernel,name", ENCODE, ids=str)
def test_encode(ctx, orc, g, kernel, name):
    st = Stripe(ctx, g, encode=False)
    hs = st.host(st.src, st.k)
    assert (hs[0] != FILL).any() and (hs[-1] != FILL).any() and not (hs[0] == hs[-1]).all()
    ctx.set_encode_kernel(kernel)
    names_of(ctx, lambda: ctx.encode_blocks(g.k, g.e, g.L, g.pitch, g.B, st.src, st.par, coef=st.coef), name)
    st.whole(st.par_all, g.e, oracle_parity(orc, st.c, hs), "parity allocation")
    st.whole(st.src_all, g.k, hs, "source allocation")


# ---- decode, general decode, verify -------------------------------------------------

# the generated and the threaded-code decode of a batch, and below 2048 (tile,
# block) pairs the two one-launch decodes of short rows: the compiled
# syndromes with the solve in the launch (AUTO) and threaded code (ONE_MATRIX)
DECODE = [
    (deep(5, 4, 4160), "generated", "k_rs_jit(decode)"),
    (deep(5, 4, 4160), "one_matrix", "k_rs_tc(decode)"),
    (deep(5, 4, 2016), "auto", "k_rs_syn_split(decode)"),
    (deep(5, 4, 2016), "one_matrix", "k_rs_tc_fused(decode)"),
    (deep(5, 4, 4099, offset=1), "auto", "k_dot_generic(decode)"),
    (wide(2, 2, 4160, 30, B=3), "generated", "k_rs_jit(decode)"),
    (wide(2, 2, 4160, 30, B=3), "one_matrix", "k_rs_tc_fused(decode)"),
    (wide(5, 4, 4160, 29, B=3), "auto", "k_rs_syn_split(decode)"),
    (wide(5, 4, 1024 * 2048 + 2080, 29, B=3), "one_matrix", "k_rs_tc(decode)"),
    (wide(2, 1, 4160, 31), "generated", "k_rs_jit(decode)"),
    (wide(2, 1, 4160, 31), "one_matrix", "k_rs_tc_fused(decode)"),
    (wide(2, 1, 4099, 31, offset=1), "auto", "k_dot_generic(decode)"),
]


def erase(st, err, value=0xEE):
    """The rows err[b] names (source or, from k on, parity) overwritten on the
    device: a decode must not read them."""
    for i in range(err.shape[1]):
        for rows, t, r0 in ((st.k, st.src, 0), (st.e, st.par, st.k)):
            b = np.flatnonzero((err[:, i] >= r0) & (err[:, i] < r0 + rows))
            if len(b):
                v = st.view(t, rows)
                v[torch.from_numpy(b).to(st.dev), torch.from_numpy(err[b, i].astype(np.int64) - r0).to(st.dev),
                  : st.L] = value
    torch.cuda.synchronize()


@pytest.mark.parametrize("g,kernel,name", DECODE, ids=str)
def test_decode(ctx, orc, g, kernel, name):
    k, e, L, B = g.k, g.e, g.L, g.B
    st = Stripe(ctx, g, more=g.bytes(e), extra=(e,))
    hs, hp = st.hosts()
    err = rsgpu.erasure_patterns(7, 0, B, k, e)
    erase(st, err)
    es = hs.copy()
    es[np.arange(B)[:, None], err] = 0xEE
    out_all, out = st.buffer(e)
    ws = torch.empty(rsgpu.decode_workspace_bytes(k, e, B), dtype=torch.uint8, device=st.dev)
    status = torch.full((B,), -1, dtype=torch.int32, device=st.dev)
    d_err = torch.from_numpy(err.copy()).to(st.dev)
    ctx.set_decode_kernel(kernel)
    names_of(ctx, lambda: ctx.decode_blocks(k, e, L, g.pitch, B, st.src, st.par, d_err, out, ws, status), name)
    assert (status.cpu().numpy() == 0).all()
    want = hs[np.arange(B)[:, None], err]  # (B, e, L): the rows as they were
    for b in st.special:  # and the oracle's own decode of the survivors
        rc, rec = orc.decode_block(list(es[b]), list(hp[b]), err[b])
        assert rc == 0 and (np.stack(rec) == want[b]).all()
    st.whole(out_all, e, want, "output allocation")
    st.unchanged(es, hp)
    assert (d_err.cpu().numpy() == err).all()


@pytest.mark.parametrize("g,name", [(deep(5, 4, 4160), "k_rs_tc(decode)"), (deep(5, 4, 4176), "k_dot_generic(decode)"),
                                    (deep(10, 4, 4099, kind="cauchy", offset=1), "k_dot_generic(decode)"),
                                    (wide(5, 4, 4160, 29, B=3), "k_rs_tc(decode)"),
                                    (wide(2, 1, 4160, 31), "k_rs_tc(decode)"),
                                    (wide(2, 1, 4099, 31, offset=1), "k_dot_generic(decode)")], ids=str)
def test_decode_general(ctx, orc, g, name):
    """Any e rows, data and parity: k_decode_prepare and the threaded-code
    apply (k_dot_generic where len % 32 != 0 or the rows are unaligned)."""
    k, e, L, B, nerrs = g.k, g.e, g.L, g.B, g.e
    st = Stripe(ctx, g, more=g.bytes(nerrs), extra=(nerrs,))
    hs, hp = st.hosts()
    rng = np.random.default_rng(3)
    matrix = None if st.coef is None else np.concatenate([np.eye(k, dtype=np.uint8), st.c])
    full = orc.gen_rs_matrix(k + e, k) if matrix is None else matrix

    def draw():
        while True:  # a list the survivors determine
            lst = np.sort(rng.choice(k + e, nerrs, replace=False)).astype(np.uint8)
            if orc.gen_decode_matrix(full, lst)[0] == 0:
                return lst

    err = np.stack([draw() for _ in range(B)])
    first, last = np.array([0, k - 1, k, k + e - 1], np.uint8), np.array([1, k, k + 1, k + e - 1], np.uint8)
    if nerrs == 4 and orc.gen_decode_matrix(full, first)[0] == 0 and orc.gen_decode_matrix(full, last)[0] == 0:
        err[0], err[-1] = first, last
    erase(st, err)
    rows = np.concatenate([hs, hp], axis=1)
    want = rows[np.arange(B)[:, None], err]
    gone = rows.copy()
    gone[np.arange(B)[:, None], err] = 0xEE
    out_all, out = st.buffer(nerrs)
    ws = torch.empty(rsgpu.decode_general_workspace_bytes(k, k + e, nerrs, B), dtype=torch.uint8, device=st.dev)
    status = torch.full((B,), -1, dtype=torch.int32, device=st.dev)
    d_err = torch.from_numpy(err.copy()).to(st.dev)
    names_of(ctx, lambda: ctx.decode_general(k, k + e, L, g.pitch, B, matrix, st.src, st.par, d_err, nerrs, out, ws,
                                             status),
             "k_decode_prepare", name)
    assert (status.cpu().numpy() == 0).all()
    for b in st.special:
        rc, rec = orc.decode_general(full, [np.ascontiguousarray(r) for r in gone[b]], err[b])
        assert rc == 0 and (np.stack(rec) == want[b]).all()
    st.whole(out_all, nerrs, want, "output allocation")
    st.unchanged(gone[:, :k], gone[:, k:])


@pytest.mark.parametrize("g", [deep(5, 4, 4176), deep(5, 4, 4099, offset=1), wide(2, 2, 4176, 30, B=3),
                               wide(2, 2, 4176, 31), wide(2, 2, 4099, 31, offset=1)], ids=str)
def test_verify(ctx, g):
    """verify_blocks counts, per block, the bytes of the recovered rows that
    differ from the source rows they stand for: none, then a known number in
    every special block."""
    k, e, L, B = g.k, g.e, g.L, g.B
    st = Stripe(ctx, g, encode=False, more=0, extra=(e,))
    hs = st.host(st.src, k)
    err = rsgpu.erasure_patterns(9, 0, B, k, e)
    want = hs[np.arange(B)[:, None], err]
    st.view(st.par, e)[:, :, :L] = torch.from_numpy(want).to(st.dev)  # the parity buffer as the output rows
    count = np.zeros(B, np.int64)
    for i, b in enumerate(st.special):
        cols = sorted({0, L - 1, L // 2, 17 + i})[: 1 + i % 4]
        for c in cols:
            st.xor(b, k + i % e, c, 0x40)
        count[b] = len(cols)
    d_err = torch.from_numpy(err.copy()).to(st.dev)
    mism = torch.full((B,), 5, dtype=torch.int64, device=st.dev)
    ctx.verify_blocks(k, e, L, g.pitch, B, st.src, st.par, d_err, mism)
    torch.cuda.synchronize()
    assert (mism.cpu().numpy() - 5 == count).all(), np.flatnonzero(mism.cpu().numpy() - 5 != count)[:8]
    st.whole(st.src_all, k, hs, "source allocation")


# ---- scrub and repair ------------------------------------------------------------

SCRUB = [
    (deep(5, 4, 4176), "two_pass", "k_scrub_compare"),
    (deep(5, 4, 4160), "two_pass", "k_scrub_compare"),
    (deep(5, 4, 4099, offset=1), "auto", "k_scrub_compare"),
    (deep(5, 4, 4160), "fused", "k_rs_bs_scrub"),
    (deep(10, 4, 4160, kind="cauchy"), "generated", "k_rs_jit_scrub"),
    (wide(2, 2, 4176, 31), "two_pass", "k_scrub_compare"),
    (wide(2, 2, 4160, 31, kind="cauchy"), "generated", "k_rs_jit_scrub"),
    (wide(5, 4, 4160, 30), "fused", "k_rs_bs_scrub"),
]


def scratch_of(g, name):
    return two_pass_scratch(g) if "compare" in name or "span" in name else 0


@pytest.mark.parametrize("locate", [True, False], ids=["locate", "detect"])
@pytest.mark.parametrize("g,kernel,name", SCRUB, ids=str)
def test_scrub(ctx, g, kernel, name, locate):
    st = Stripe(ctx, g, more=scratch_of(g, name))
    damage(st)
    hs, hp = st.hosts()
    syn = syndromes(st.c, hs, hp)
    want = [sm.report(st.c, s, locate) for s in syn]
    dirty = [b for b, w in enumerate(want) if w[1] != sm.CLEAN]
    assert dirty == st.special
    rep = torch.full((g.B * SDT.itemsize,), POISON, dtype=torch.uint8, device=st.dev)
    ctx.set_scrub_kernel(kernel)
    names_of(ctx, lambda: ctx.scrub_blocks(g.k, g.e, g.L, g.pitch, g.B, st.src, st.par, rep, coef=st.coef,
                                           locate=locate), name)
    gf.same(rep.cpu().numpy().view(SDT), want)
    st.unchanged(hs, hp)


REPAIR = [
    (deep(5, 4, 4176), "two_pass", "auto", "k_repair_compare"),
    (deep(5, 4, 4099, offset=1), "auto", "auto", "k_repair_compare"),
    (deep(5, 4, 4160), "fused", "auto", "k_rs_bs_repair"),
    (deep(10, 4, 4160, kind="cauchy"), "auto", "generated", "k_rs_jit_repair"),
    (wide(5, 4, 4176, 30), "two_pass", "auto", "k_repair_compare"),
    (wide(5, 4, 4160, 30), "fused", "auto", "k_rs_bs_repair"),
    (wide(5, 4, 4160, 30, kind="cauchy"), "auto", "generated", "k_rs_jit_repair"),
    (wide(2, 2, 4176, 31), "two_pass", "auto", "k_repair_compare"),
    (wide(2, 2, 4160, 31, kind="cauchy"), "auto", "generated", "k_rs_jit_repair"),
]
# COLUMNS needs e >= 3, and ten rows of 2 GiB with 6 GiB of scratch do not fit the cap
REPAIR_MODES = [c + (mode,) for c in REPAIR for mode in (("one_row", "columns") if c[0].e >= 3 else ("one_row",))]


@pytest.mark.parametrize("g,scrub,repair,name,mode", REPAIR_MODES, ids=str)
def test_repair(ctx, g, scrub, repair, name, mode):
    st = Stripe(ctx, g, more=scratch_of(g, name))
    damage(st)
    hs, hp = st.hosts()
    syn = syndromes(st.c, hs, hp)
    assert [b for b in range(g.B) if syn[b].any()] == st.special
    want = [(0, 0, rm.CLEAN, -1)] * g.B
    for b in st.special:
        hs[b], hp[b], want[b] = rm.repair(st.c, hs[b], hp[b], mode)
    assert rm.REPAIRED in {w[2] for w in want}
    rep = torch.full((g.B * RDT.itemsize,), POISON, dtype=torch.uint8, device=st.dev)
    ctx.set_scrub_kernel(scrub)
    ctx.set_repair_kernel(repair)
    names_of(ctx, lambda: ctx.repair_blocks(g.k, g.e, g.L, g.pitch, g.B, st.src, st.par, rep, coef=st.coef, mode=mode),
             name, *([name + "_gated"] if mode == "one_row" else []))
    gf.same(rep.cpu().numpy().view(RDT), want, gf.REPAIR_FIELDS)
    st.unchanged(hs, hp)


# ---- update ---------------------------------------------------------------------

UPDATE = [
    (deep(5, 4, 4176), False, ["k_update_blocks"]),
    (deep(5, 4, 4099), False, ["k_update_blocks", "k_update_blocks(tail)"]),
    (deep(5, 4, 4099, offset=1), False, ["k_update_blocks(bytes)"]),
    (deep(5, 4, 4176), True, ["k_update_blocks"]),
    (wide(2, 2, 4176, 30, B=3), False, ["k_update_blocks"]),
    (wide(5, 4, 4099, 29, B=3, offset=1), True, ["k_update_blocks(bytes)"]),
    (wide(2, 2, 4176, 31), False, ["k_update_blocks"]),
    (wide(2, 2, 4099, 31, offset=1), True, ["k_update_blocks(bytes)"]),
]


@pytest.mark.parametrize("g,delta,names", UPDATE, ids=str)
def test_update(ctx, g, delta, names):
    """Every block has a list: the special blocks the first rows, the last
    rows, a NONE-padded list and none at all by turns, the others random rows.
    The update rows are a third buffer that passes 2^32."""
    k, e, L, B = g.k, g.e, g.L, g.B
    u = min(4, k) if g.pitch < T31 else 1  # one update row of 2 GiB + 64 per block is what the cap leaves
    st = Stripe(ctx, g, more=g.bytes(u), extra=(u,))
    upd_all, upd = st.buffer(u)
    ctx.fill_synthetic(upd, B * u, L, g.pitch, 1011, 0)
    rng = np.random.default_rng(5)
    cols = np.stack([np.sort(rng.choice(k, u, replace=False)) for _ in range(B)]).astype(np.uint8)
    for i, b in enumerate(st.special):
        cols[b] = [np.arange(u), np.arange(k - u, k), um.pad([k - 1], u), um.pad([], u)][i % 4]
    hs, hp = st.hosts()
    hu = st.host(upd, u)
    status = []
    for b in range(B):
        hs[b], hp[b], s = um.update(st.c, hs[b], hp[b], cols[b], hu[b], delta=delta)
        status.append(s)
    assert status == [0] * B
    d_cols = torch.from_numpy(cols.copy()).to(st.dev)
    d_status = torch.full((B,), 0x5A5A5A5A, dtype=torch.int32, device=st.dev)
    got = names_of(ctx, lambda: ctx.update_blocks(k, e, L, g.pitch, B, u, d_cols, upd, None if delta else st.src,
                                                  st.par, d_status, coef=st.coef, delta=delta))
    assert got == names
    assert d_status.cpu().numpy().tolist() == status
    st.unchanged(hs, hp)
    st.whole(upd_all, u, hu, "update rows")
    assert (d_cols.cpu().numpy() == cols).all()


# ---- degraded scrub and rebuild ------------------------------------------------------

def lists_for(st, u, seed=5):
    """(B, u) lists: empty everywhere but in the special blocks, which take
    gf.mixed_lists' turns (no row, data only, parity only, both; the first and
    the last rows)."""
    mixed = gf.mixed_lists(st.k, st.e, u, max(len(st.special), 3), seed)
    lost = np.full((st.B, u), N, np.uint8)
    for i, b in enumerate(st.special):
        lost[b] = mixed[i]
    return lost


def noise_in(st, lost, seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    for b in range(st.B):
        for r in dm.list_rows(lost[b], st.k, st.e) or []:
            st.row(b, r).copy_(torch.randint(0, 256, (st.L,), dtype=torch.uint8, generator=g))
    torch.cuda.synchronize()


DEGRADED = [
    (deep(5, 4, 4176), "two_pass", "k_degraded_compare"),
    (deep(5, 4, 4099, offset=1), "two_pass", "k_degraded_compare(bytes)"),
    (deep(5, 4, 4160), "fused", "k_rs_bs_degraded"),
    (wide(5, 4, 4176, 30), "two_pass", "k_degraded_compare"),
    (wide(5, 4, 4160, 30), "fused", "k_rs_bs_degraded"),
    (wide(2, 2, 4176, 31), "two_pass", "k_degraded_compare"),
]


@pytest.mark.parametrize("g,kernel,name", DEGRADED, ids=str)
def test_scrub_degraded(ctx, g, kernel, name):
    """Lists in the special blocks, noise in the lost rows, then damage in a
    survivor of every second special block."""
    k, e, L, B, u = g.k, g.e, g.L, g.B, 2
    st = Stripe(ctx, g, more=scratch_of(g, name))
    lost = lists_for(st, u)
    noise_in(st, lost)
    for i, b in enumerate(st.special[::2]):
        surv = [r for r in range(k + e) if r not in dm.list_rows(lost[b], k, e)]
        st.xor(b, surv[i % len(surv)], (L - 1) if i % 2 else 3, 0x31)
    torch.cuda.synchronize()
    hs, hp = st.hosts()
    syn = syndromes(st.c, hs, hp)
    want = [dm.report_syn(st.c, syn[b], lost[b]) for b in range(B)]
    assert {w[1] for w in want} >= ({dm.CLEAN, dm.ONE_ROW} if e >= 4 else {dm.CLEAN}) and len({w[1] for w in want}) > 1
    assert all(want[b] == (0, dm.CLEAN, -1) for b in range(B) if b not in st.special)
    d_lost = torch.from_numpy(lost.copy()).to(st.dev)
    rep = torch.full((B * SDT.itemsize,), POISON, dtype=torch.uint8, device=st.dev)
    ctx.set_degraded_kernel(kernel)
    names_of(ctx, lambda: ctx.scrub_degraded_blocks(k, e, L, g.pitch, B, st.src, st.par, u, d_lost, rep, coef=st.coef),
             "k_degraded_prepare", name, "k_degraded_finalise")
    gf.same(rep.cpu().numpy().view(SDT), want)
    st.unchanged(hs, hp)
    assert (d_lost.cpu().numpy() == lost).all()


REBUILD = [
    (deep(5, 4, 4176), "lanes", "k_rebuild_blocks"),
    (deep(5, 4, 4099, offset=1), "lanes", "k_rebuild_blocks(bytes)"),
    (deep(5, 4, 4176), "threaded", "k_rs_tc(rebuild)"),
    (wide(5, 4, 4176, 30), "lanes", "k_rebuild_blocks"),
    (wide(5, 4, 4176, 30), "threaded", "k_rs_tc(rebuild)"),
    (wide(2, 2, 4176, 31), "lanes", "k_rebuild_blocks"),
    (wide(2, 2, 4160, 31), "threaded", "k_rs_tc(rebuild)"),
]


@pytest.mark.parametrize("check", [False, True], ids=["unchecked", "checked"])
@pytest.mark.parametrize("g,kernel,name", REBUILD, ids=str)
def test_rebuild(ctx, g, kernel, name, check):
    """Lists in the special blocks with noise in the listed rows; with the
    check a damaged survivor in every second one, which the call locates and
    rebuilds as well."""
    k, e, L, B, u = g.k, g.e, g.L, g.B, 2
    st = Stripe(ctx, g, more=two_pass_scratch(g) if check else 0)
    lost = lists_for(st, u)
    noise_in(st, lost)
    if check:
        for i, b in enumerate(st.special[::2]):
            surv = [r for r in range(k + e) if r not in dm.list_rows(lost[b], k, e)]
            st.xor(b, surv[-1 - i % len(surv)], L // 2, 0x6E)
        torch.cuda.synchronize()
    hs, hp = st.hosts()
    want = [(0, dm.CLEAN, -1)] * B
    empty = dm.pad([], u)
    for b in range(B):
        if b in st.special:
            want[b], hs[b], hp[b] = rbm.call(st.c, hs[b], hp[b], lost[b], check)
        else:
            assert (lost[b] == empty).all()
    # a block with an empty list and consistent rows: the model once
    for b in [b for b in range(B) if b not in st.special][:1]:
        assert rbm.call(st.c, hs[b], hp[b], empty, check)[0] == (0, dm.CLEAN, -1)
    assert not syndromes(st.c, hs, hp)[[b for b in range(B) if b not in st.special]].any()
    d_lost = torch.from_numpy(lost.copy()).to(st.dev)
    rep = torch.full((B * SDT.itemsize,), POISON, dtype=torch.uint8, device=st.dev)
    ctx.set_rebuild_kernel(kernel)
    names_of(ctx, lambda: ctx.rebuild_blocks(k, e, L, g.pitch, B, st.src, st.par, u, d_lost, rep, coef=st.coef,
                                             check=check), name)
    gf.same(rep.cpu().numpy().view(SDT), want)
    st.unchanged(hs, hp)
    assert (d_lost.cpu().numpy() == lost).all()


# ---- locate and correct ------------------------------------------------------------

LOCATE = [
    (deep(5, 4, 4176), "two_pass", "auto", "k_locate_span"),
    (deep(5, 4, 4099, offset=1), "two_pass", "auto", "k_locate_span(bytes)"),
    (deep(5, 4, 4160), "fused", "auto", "k_rs_bs_locate"),
    (deep(10, 4, 4160, kind="cauchy"), "fused", "generated", "k_rs_jit_locate"),
    (wide(5, 4, 4176, 30), "two_pass", "auto", "k_locate_span"),
    (wide(5, 4, 4160, 30), "fused", "auto", "k_rs_bs_locate"),
    (wide(5, 4, 4160, 30, kind="cauchy"), "fused", "generated", "k_rs_jit_locate"),
    (wide(2, 2, 4176, 31), "two_pass", "auto", "k_locate_span"),
    (wide(2, 2, 4160, 31, kind="cauchy"), "fused", "generated", "k_rs_jit_locate"),
]


@pytest.mark.parametrize("g,locate,scrub,name", LOCATE, ids=str)
def test_locate(ctx, g, locate, scrub, name):
    k, e, L, B, u = g.k, g.e, g.L, g.B, 3
    st = Stripe(ctx, g, more=scratch_of(g, name))
    damage(st)
    hs, hp = st.hosts()
    syn = syndromes(st.c, hs, hp)
    want = [lm.report_syn(st.c, s, u) for s in syn]
    assert [b for b, w in enumerate(want) if w[0][1] != lm.CLEAN] == st.special
    if B > 3:
        assert {w[0][1] for w in want} >= {lm.CLEAN, lm.ONE_ROW, lm.ROWS}
    rep = torch.full((B * SDT.itemsize,), POISON, dtype=torch.uint8, device=st.dev)
    rows = torch.full((B * u,), POISON, dtype=torch.uint8, device=st.dev)
    ctx.set_locate_kernel(locate)
    ctx.set_scrub_kernel(scrub)
    names_of(ctx, lambda: ctx.locate_blocks(k, e, L, g.pitch, B, st.src, st.par, u, rows, rep, coef=st.coef),
             name, "k_locate_finish")
    gf.same(rep.cpu().numpy().view(SDT), [w[0] for w in want])
    assert rows.cpu().numpy().reshape(B, u).tolist() == [list(map(int, w[1])) for w in want]
    st.unchanged(hs, hp)


# t = 2 needs e >= 5: two-pass on (9, 5), the compiled kernel on (16, 8), the
# generated one on a Cauchy (9, 5)
CORRECT = [
    (deep(5, 4, 4176), 1, "two_pass", "auto", "k_correct_compare"),
    (deep(5, 4, 4099, offset=1), 1, "auto", "auto", "k_correct_compare"),
    (deep(5, 4, 4160), 1, "fused", "auto", "k_rs_bs_correct"),
    (deep(10, 4, 4160, kind="cauchy"), 1, "fused", "generated", "k_rs_jit_correct"),
    (deep(9, 5, 4176), 2, "two_pass", "auto", "k_correct_compare"),
    (deep(16, 8, 4160), 2, "fused", "auto", "k_rs_bs_correct"),
    (deep(9, 5, 4160, kind="cauchy"), 2, "fused", "generated", "k_rs_jit_correct"),
    (wide(5, 4, 4176, 30), 1, "two_pass", "auto", "k_correct_compare"),
    (wide(5, 4, 4160, 30), 1, "fused", "auto", "k_rs_bs_correct"),
    (wide(16, 8, 4160, 28, B=3), 2, "fused", "auto", "k_rs_bs_correct"),
    (wide(9, 5, 4160, 29, B=3, kind="cauchy"), 2, "fused", "generated", "k_rs_jit_correct"),
    # e >= 3: five rows of 2 GiB per block; the two-pass form's 6 GiB of scratch would pass the cap
    (wide(2, 3, 4160, 31, kind="cauchy"), 1, "fused", "generated", "k_rs_jit_correct"),
]


@pytest.mark.parametrize("g,t,correct,scrub,name", CORRECT, ids=str)
def test_correct(ctx, g, t, correct, scrub, name):
    st = Stripe(ctx, g, more=scratch_of(g, name))
    damage(st, pairs=True, first=0 if g.B > 3 else 4)
    hs, hp = st.hosts()
    syn = syndromes(st.c, hs, hp)
    assert [b for b in range(g.B) if syn[b].any()] == st.special
    want = [(0, 0, 0, cm.rm.CLEAN, -1)] * g.B
    for b in st.special:
        hs[b], hp[b], want[b] = cm.correct(st.c, hs[b], hp[b], t)
    if t == 2:
        assert any(w[2] for w in want)  # a column that took two rows
    rep = torch.full((g.B * CDT.itemsize,), POISON, dtype=torch.uint8, device=st.dev)
    ctx.set_correct_kernel(correct)
    ctx.set_scrub_kernel(scrub)
    names_of(ctx, lambda: ctx.correct_blocks(g.k, g.e, g.L, g.pitch, g.B, st.src, st.par, rep, coef=st.coef, t=t),
             name, "k_correct_finalise")
    gf.same(rep.cpu().numpy().view(CDT), want, ("bad_columns", "corrected_columns", "two_row_columns", "status", "row"))
    st.unchanged(hs, hp)


# ---- the row-pointer batch ------------------------------------------------------------

@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("kernel,aligned,flag,name", [("auto", True, True, "k_rs_jit(ec_batch)"),
                                                      ("auto", False, False, "k_dot_bytes(ec_batch)"),
                                                      ("threaded", True, False, "k_dot_bytes(ec_batch)")], ids=str)
def test_ec_encode_data_batch(ctx, orc, kernel, aligned, flag, name, order):
    """One arena of 16 GiB + 64 KiB; any two rows of a block lie more than
    4 GiB apart in it (slot s of block b at s x (4 GiB + 4160) + b x 8 KiB),
    in ascending or descending address order; lengths with 0, a multiple of
    32, and (unaligned) a tail and odd starts.  The program kernel under
    RSGPU_BATCH_ALIGNED32, the byte kernel on unaligned rows and under
    THREADED."""
    k, rows, B = 3, 2, 6
    stride, slot = T32 + 4160, 8192
    span = (k + rows - 1) * stride + B * slot
    assert stride > T32 and stride % 16 == 0 and span > 3 * T32
    room(span + 2 * GiB)
    dev = torch.device("cuda", 0)
    arena = torch.empty(span, dtype=torch.uint8, device=dev)
    arena.fill_(FILL)
    lens = [4160, 0, 2080, 32, 4096, 4160] if aligned else [4099, 0, 2081, 31, 4160, 1]
    skew = 0 if aligned else 3
    rng = np.random.default_rng(12)
    c = sm.cauchy_matrix(k, rows)
    g = orc.init_tables(k, rows, c)
    slots = list(range(k + rows))
    if order == "descending":
        slots.reverse()
    data, coding, want = [], [], []
    for b in range(B):
        at = [s * stride + b * slot + skew for s in slots]
        src = rng.integers(0, 256, (k, lens[b]), dtype=np.uint8)
        for j in range(k):
            arena[at[j]: at[j] + lens[b]] = torch.from_numpy(src[j]).to(dev)
        data.append([arena[a: a + lens[b]] for a in at[:k]])
        coding.append([arena[a: a + lens[b]] for a in at[k:]])
        out = [np.zeros(lens[b], np.uint8) for _ in range(rows)]
        if lens[b]:
            orc.encode_data(lens[b], k, rows, g, [np.ascontiguousarray(r) for r in src], out)
        want.append((at, src, out))
    assert min(abs(a - b) for at, _, _ in want for a in at for b in at if a != b) > T32
    d_data, d_coding, d_len, max_len = rsgpu.row_tables(data, coding, dev)
    status = torch.full((B,), 9, dtype=torch.int32, device=dev)
    ctx.set_encode_kernel(kernel)
    names_of(ctx, lambda: ctx.ec_encode_data_batch(k, rows, g, B, d_data, d_coding, d_len, max_len, status,
                                                   aligned32=flag), "classify(ec_batch)", name)
    assert status.cpu().numpy().tolist() == [0] * B
    # every row where it belongs, then the rows put back to FILL: nothing else was written
    for b, (at, src, out) in enumerate(want):
        for a, row in zip(at, list(src) + out):
            assert (arena[a: a + lens[b]].cpu().numpy() == row).all(), (b, a)
            arena[a: a + lens[b]] = FILL
    for s in range(0, span, GiB):
        assert bool((arena[s: s + GiB] == FILL).all()), s


# ---- the flat tiling of the compiled encode ----------------------------------------------

def flat_cases():
    """(5, 4) as far as four blocks of 2080 bytes or seventy of 32 go: fewer
    than 2048 (tile, block) pairs, which the split kernel serves on per-block
    tiles whatever the guard says.  (64, 16) has no split kernel: the same
    lengths and block counts reach k_rs_bs and its flat tiles."""
    out = []
    for K, E, name in ((5, 4, "k_rs_bs_split(encode)"), (64, 16, "k_rs_bs(encode)")):
        for L, B in ((32, 70), (2080, 4)):
            below, above = lo.flat_pitches(L, K)
            out += [(K, E, L, B, below, True, name), (K, E, L, B, above, False, name)]
        out.append((K, E, 32, 70, lo.flat_true_edge(32, K), False, name))
    return out


@pytest.mark.parametrize("K,E,L,B,pitch,flat,name", flat_cases(), ids=str)
def test_flat_edge(ctx, orc, K, E, L, B, pitch, flat, name):
    """The compiled encode on both sides of the guard of its flat tiling
    (rs_bitsliced.hip launch): below it a lane's 32-bit offset from its tile's
    first block reaches 63 x K x pitch = 4.1e9 at len 32 and passes 2^31 at len
    2080; above it the tiles are per block.  The third pitch at len 32 is the
    first at which flat tiles would pass 2^32."""
    assert lo.flat_guard(L, K, pitch, B) == flat
    if flat:
        assert (T31 if L == 32 else T31 - 2048) <= lo.flat_lane_offsets(L, K, pitch, B)[0].max() < T32
    st = Stripe(ctx, Geo(f"flat-L{L}-p{pitch}", K, E, "rs", L, B, pitch, 0), encode=False, checked=False)
    assert B * K * pitch > T32
    hs = st.host(st.src, K)
    ctx.set_encode_kernel("compiled")
    recs = gf.recorded(ctx, lambda: ctx.encode_blocks(K, E, L, pitch, B, st.src, st.par), blocks=True)
    torch.cuda.synchronize()
    assert recs == [(name, B)]
    st.whole(st.par_all, E, oracle_parity(orc, st.c, hs), "parity allocation")
    st.whole(st.src_all, K, hs, "source allocation")


# ---- long rows ----------------------------------------------------------------------

class LongRows:
    """One block of k + e rows of n bytes at pitch n + 64, each source row a
    period of lo.PERIOD random bytes tiled to n; FILL elsewhere."""

    def __init__(self, ctx, orc, k, e, n, more=0, kind="rs"):
        self.k, self.e, self.n, self.pitch = k, e, n, (n + 64 + 15) // 16 * 16
        assert self.pitch % 16 == 0
        room((k + e) * self.pitch + more + 3 * GiB)
        self.dev = torch.device("cuda", 0)
        self.c = gf.matrix(k, e, kind)
        self.coef = None if kind == "rs" else self.c
        self.pat = lo.patterns(k)
        self.par_pat = lo.parity_period(orc, self.c, self.pat)
        self.src = self.alloc(k)
        self.par = self.alloc(e)
        for j in range(k):
            self.tile(self.src, j, self.pat[j])

    def alloc(self, rows):
        t = torch.empty(rows * self.pitch, dtype=torch.uint8, device=self.dev)
        t.fill_(FILL)
        return t

    def tile(self, t, r, period):
        """Row r of t := `period` tiled to n bytes."""
        p = len(period)
        row = t[r * self.pitch: r * self.pitch + self.n]
        d = torch.from_numpy(np.ascontiguousarray(period)).to(self.dev)
        chunks, (t0, tn) = lo.chunks(self.n)
        for a, c in chunks:
            row[a: a + c * p].view(c, p)[:] = d
        row[t0: t0 + tn] = d[:tn]

    def is_tiled(self, t, r, period, what):
        """Row r of t is `period` tiled to n bytes and FILL behind them, in
        pieces of at most 1 GiB."""
        p = len(period)
        row = t[r * self.pitch: r * self.pitch + self.n]
        d = torch.from_numpy(np.ascontiguousarray(period)).to(self.dev)
        chunks, (t0, tn) = lo.chunks(self.n)
        for a, c in chunks:
            ok = (row[a: a + c * p].view(c, p) == d).all(dim=1)
            if not bool(ok.all()):
                first = a + int((~ok).nonzero()[0]) * p
                raise AssertionError(f"{what}: row {r} differs from the reference in the period at byte {first}")
        assert bool((row[t0: t0 + tn] == d[:tn]).all()), f"{what}: the tail of row {r}"
        assert bool((t[r * self.pitch + self.n: (r + 1) * self.pitch] == FILL).all()), f"{what}: padding of row {r}"

    def is_fill(self, t, rows, what):
        for r in range(rows):
            for a in range(0, self.pitch, GiB):
                assert bool((t[r * self.pitch + a: min((r + 1) * self.pitch, r * self.pitch + a + GiB)] == FILL).all()), what

    def sources_intact(self):
        for j in range(self.k):
            self.is_tiled(self.src, j, self.pat[j], "source")


LEN_A = T31 + 2048 + 32      # lane offsets past 2^31, legal everywhere
LEN_MAX = T32 - 32           # the longest row of 32-byte pieces the calls accept
LEN_B = T32 + 2048 + 32      # beyond RSGPU_MAX_LEN: refused


# the compiled codes start at (5, 4): nine rows of 4 GiB do not fit the cap, so
# k_rs_bs runs the shorter length only (test_flat_edge takes the same 32-bit
# operand to 4.1e9)
@pytest.mark.parametrize("k,e,kernel,name,n", [(2, 2, "generated", "k_rs_jit(encode)", LEN_A),
                                               (2, 2, "threaded", "k_rs_tc(encode)", LEN_A),
                                               (5, 4, "compiled", "k_rs_bs(encode)", LEN_A),
                                               (2, 2, "generated", "k_rs_jit(encode)", LEN_MAX),
                                               (2, 2, "threaded", "k_rs_tc(encode)", LEN_MAX),
                                               (2, 1, "auto", "k_dot_generic", lo.MAX_LEN)], ids=str)
def test_long_rows_encode(ctx, orc, k, e, kernel, name, n):
    """A lane's offset inside its row at and past 2^31, up to the longest row
    of 32-byte pieces the call accepts; and RSGPU_MAX_LEN itself, the longest
    row there is, which k_dot_generic takes (vectors and a 15-byte tail):
    the accepting side of the limit, one byte from the refusal."""
    assert T31 < n <= lo.MAX_LEN and (n == LEN_A or n + 32 > lo.MAX_LEN) and (n % 32 == 0 or n == lo.MAX_LEN)
    lr = LongRows(ctx, orc, k, e, n)
    ctx.set_encode_kernel(kernel)
    names_of(ctx, lambda: ctx.encode_blocks(k, e, n, lr.pitch, 1, lr.src, lr.par), name)
    for i in range(e):
        lr.is_tiled(lr.par, i, lr.par_pat[i], "parity")
    lr.sources_intact()


@pytest.mark.parametrize("n", [LEN_A, LEN_MAX], ids=["2^31+2080", "2^32-32"])
@pytest.mark.parametrize("kernel,name", [("generated", "k_rs_jit(decode)"), ("one_matrix", "k_rs_tc(decode)")], ids=str)
def test_long_rows_decode(ctx, orc, kernel, name, n):
    k, e = 2, 1
    lr = LongRows(ctx, orc, k, e, n, more=n + 80)
    ctx.encode_blocks(k, e, n, lr.pitch, 1, lr.src, lr.par)
    lr.is_tiled(lr.par, 0, lr.par_pat[0], "parity")
    lr.src[lr.pitch: lr.pitch + n] = 0xEE  # row 1 is lost
    out = lr.alloc(e)
    d_err = torch.tensor([1], dtype=torch.uint8, device=lr.dev)
    ws = torch.empty(rsgpu.decode_workspace_bytes(k, e, 1), dtype=torch.uint8, device=lr.dev)
    status = torch.full((1,), -1, dtype=torch.int32, device=lr.dev)
    ctx.set_decode_kernel(kernel)
    names_of(ctx, lambda: ctx.decode_blocks(k, e, n, lr.pitch, 1, lr.src, lr.par, d_err, out, ws, status), name)
    assert int(status.item()) == 0
    lr.is_tiled(out, 0, lr.pat[1], "recovered row")
    lr.is_tiled(lr.src, 0, lr.pat[0], "source")
    lr.is_tiled(lr.par, 0, lr.par_pat[0], "parity")


@pytest.mark.parametrize("k,e,kind,kernel,name", [(5, 4, "rs", "fused", "k_rs_bs_scrub"),
                                                 (2, 2, "cauchy", "generated", "k_rs_jit_scrub")], ids=str)
def test_long_rows_scrub(ctx, orc, k, e, kind, kernel, name):
    """Clean, then one byte of a source row past 2^31 and one of a parity row
    at the very end."""
    n = LEN_A
    lr = LongRows(ctx, orc, k, e, n, kind=kind)
    ctx.encode_blocks(k, e, n, lr.pitch, 1, lr.src, lr.par, coef=lr.coef)
    rep = torch.full((SDT.itemsize,), POISON, dtype=torch.uint8, device=lr.dev)
    ctx.set_scrub_kernel(kernel)
    scrub = lambda: ctx.scrub_blocks(k, e, n, lr.pitch, 1, lr.src, lr.par, rep, coef=lr.coef)  # noqa: E731
    names_of(ctx, scrub, name)
    gf.same(rep.cpu().numpy().view(SDT), [(0, sm.CLEAN, -1)])
    lr.src[(k - 1) * lr.pitch + T31 + 5] ^= 0x10
    scrub()
    torch.cuda.synchronize()
    gf.same(rep.cpu().numpy().view(SDT), [(1, sm.ONE_ROW, k - 1)])
    lr.par[n - 1] ^= 0x01
    scrub()
    torch.cuda.synchronize()
    gf.same(rep.cpu().numpy().view(SDT), [(2, sm.DAMAGED, -1)])


def test_long_rows_update(ctx, orc):
    """Row 1 of (2, 2) replaced by another periodic row: the parity follows
    along the whole length."""
    k, e, n = 2, 2, LEN_A
    lr = LongRows(ctx, orc, k, e, n, more=n + 64)
    ctx.encode_blocks(k, e, n, lr.pitch, 1, lr.src, lr.par)
    new = lo.patterns(1, seed=99)[0]
    upd = lr.alloc(1)
    lr.tile(upd, 0, new)
    pat = np.stack([lr.pat[0], new])
    d_cols = torch.tensor([1], dtype=torch.uint8, device=lr.dev)
    status = torch.full((1,), -1, dtype=torch.int32, device=lr.dev)
    names_of(ctx, lambda: ctx.update_blocks(k, e, n, lr.pitch, 1, 1, d_cols, upd, lr.src, lr.par, status),
             "k_update_blocks")
    assert int(status.item()) == 0
    par = lo.parity_period(orc, lr.c, pat)
    for i in range(e):
        lr.is_tiled(lr.par, i, par[i], "parity")
    lr.is_tiled(lr.src, 0, pat[0], "source")
    lr.is_tiled(lr.src, 1, pat[1], "source")
    lr.is_tiled(upd, 0, new, "update row")


REFUSED = "RSGPU_ERR_ARG.*len must be below 4 GiB"


def refused(ctx, call):
    """RSGPU_ERR_ARG with the limit's text, and nothing enqueued."""
    def run():
        with pytest.raises(rsgpu.RsGpuError, match=REFUSED):
            call()
    assert gf.recorded(ctx, run) == []


@pytest.mark.parametrize("kernel", ["auto", "compiled", "generated", "threaded"])
def test_rows_beyond_the_limit_are_refused_encode(ctx, kernel):
    """len = 2^32 + 2080 > RSGPU_MAX_LEN through rsgpu_encode_blocks under
    every encode kernel: RSGPU_ERR_ARG with its text, and not a byte of the
    parity buffer written.  (Before the limit the call returned RSGPU_OK with
    every parity byte past 4 GiB computed from the sources at off mod 2^32.)"""
    k, e, n = 2, 1, LEN_B
    assert n > lo.MAX_LEN
    pitch = n + 64
    room((k + e) * pitch + GiB)
    dev = torch.device("cuda", 0)
    src = torch.empty(k * pitch, dtype=torch.uint8, device=dev)
    par = torch.empty(e * pitch, dtype=torch.uint8, device=dev)
    src.fill_(0x11)
    par.fill_(FILL)
    ctx.set_encode_kernel(kernel)
    refused(ctx, lambda: ctx.encode_blocks(k, e, n, pitch, 1, src, par))
    refused(ctx, lambda: ctx.encode_blocks(k, e, lo.MAX_LEN + 1, pitch, 1, src, par))
    torch.cuda.synchronize()
    for a in range(0, e * pitch, GiB):
        assert bool((par[a: a + GiB] == FILL).all())


def test_rows_beyond_the_limit_are_refused_everywhere(ctx):
    """The same rule in every block-batched call: refused before anything is
    enqueued, the outputs as they were.  Small buffers: a refused call reads
    and writes nothing.

    Hazard: the buffers are 4 KiB because a refused call must touch none of
    them.  Should an entry point ever lose its check_geom, its call here would
    walk 4 GiB over a 4 KiB allocation, a fault on the device, not a clean
    failure: whoever changes check_geom or adds an entry point runs
    test_rows_beyond_the_limit_are_refused_encode (real buffers) first and
    reads the entry point's first statement before this test."""
    k, e, n = 2, 2, LEN_B
    pitch = n + 64
    dev = torch.device("cuda", 0)
    t = {name: torch.full((4096,), FILL, dtype=torch.uint8, device=dev)
         for name in ("src", "par", "out", "ws", "rep", "lst", "upd")}
    status = torch.full((8,), 7, dtype=torch.int32, device=dev)
    mism = torch.full((8,), 7, dtype=torch.int64, device=dev)
    a = (k, e, n, pitch, 1)
    calls = {
        "decode_blocks": lambda: ctx.decode_blocks(*a, t["src"], t["par"], t["lst"], t["out"], t["ws"], status),
        "decode_prepare": lambda: ctx.decode_prepare(*a, t["src"], t["par"], t["lst"], t["out"], t["ws"], status),
        "decode_apply": lambda: ctx.decode_apply(*a, t["src"], t["par"], t["out"], t["ws"], status),
        "decode_general": lambda: ctx.decode_general(k, k + e, n, pitch, 1, None, t["src"], t["par"], t["lst"], 1,
                                                     t["out"], t["ws"], status),
        "verify_blocks": lambda: ctx.verify_blocks(*a, t["src"], t["out"], t["lst"], mism),
        "scrub_blocks": lambda: ctx.scrub_blocks(*a, t["src"], t["par"], t["rep"]),
        "repair_blocks": lambda: ctx.repair_blocks(*a, t["src"], t["par"], t["rep"]),
        "correct_blocks": lambda: ctx.correct_blocks(*a, t["src"], t["par"], t["rep"], t=1),
        "update_blocks": lambda: ctx.update_blocks(*a, 1, t["lst"], t["upd"], t["src"], t["par"], status),
        "scrub_degraded_blocks": lambda: ctx.scrub_degraded_blocks(*a, t["src"], t["par"], 1, t["lst"], t["rep"]),
        "rebuild_blocks": lambda: ctx.rebuild_blocks(*a, t["src"], t["par"], 1, t["lst"], t["rep"]),
        "locate_blocks": lambda: ctx.locate_blocks(*a, t["src"], t["par"], 1, t["lst"], t["rep"]),
    }
    for kernel in ("auto", "two_pass"):
        ctx.set_scrub_kernel(kernel)
        for call in calls.values():
            refused(ctx, call)
    torch.cuda.synchronize()
    assert all(bool((v == FILL).all()) for v in t.values())
    assert bool((status == 7).all()) and bool((mism == 7).all())
    # the host-resident calls refuse before they stage anything
    h = np.zeros(16, np.uint8)
    with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_ARG"):
        ctx.encode_blocks_host(k, e, n, pitch, 1, h, h)
    with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_ARG"):
        ctx.decode_blocks_host(k, e, n, pitch, 1, h, h, h, h)
    assert (h == 0).all()
