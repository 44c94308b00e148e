"""rsgpu_locate_blocks under rsgpu_set_locate_kernel FUSED with the scrub kernel
GENERATED (k_rs_jit_locate, k_rs_jitw_locate; include/rsgpu.h): the blocks and
the model of tests/test_gpu_locate.py and the checks of
tests/test_gpu_locate_fused.py, on matrices that have no compiled kernel.
Every call is compared field by field with the numpy model
(tests/locate_model.py), must leave both allocations as they were, must have
run the kernel the case expects (the timing records say which), and a second
call under "two_pass" must give the same bytes, reports and lists.

A tile is 2048 bytes, a lane's share 32: L0 = 3 * 2048 + 5 * 32 gives three
full tiles and one whose last 59 lanes are idle; with two or three tiles per
workgroup the last workgroup also owns tiles past the row end.

More than 64 source rows: tests/test_gpu_family_generated_wide.py."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import degraded_model as dm  # noqa: E402
import gpu_family as gf  # noqa: E402
import locate_model as lm  # noqa: E402
import rsgpu  # noqa: E402
from test_gpu_locate import Blocks, columns, hooks  # noqa: E402
from test_gpu_locate_fused import damage_every_code, records  # noqa: E402

N = dm.NONE
TILE = 2048
L0 = 3 * TILE + 5 * 32
GENERATED = "k_rs_jit_locate"
COMPILED = "k_rs_bs_locate"
SPAN = "k_locate_span"
LOCATED = (lm.ONE_ROW, lm.ROWS)
# one and two waves of 8 rows; 2 x 10 / 12 / 16 rows; four waves of 10 / 12 / 16; e = 3
MATRICES = [(10, 4), (11, 12), (13, 20), (13, 24), (14, 32), (9, 34), (9, 44), (8, 56), (6, 3), (12, 4), (17, 3)]
LENGTHS = [32, 2112, 4160, 6144]  # tests/test_gpu_scrub_generated.py


def set_tiles(ctx, n):
    H = hooks()
    H.rsgpu_internal_set_jitw_tiles.argtypes = [C.c_void_p, C.c_int]
    assert H.rsgpu_internal_set_jitw_tiles(ctx.handle, n) == 0


@pytest.fixture(scope="module")
def ctx():
    for c in gf.device_context(reset_scrub_kernel=True):
        c.set_locate_kernel("fused")
        c.set_scrub_kernel("generated")
        yield c
        c.set_locate_kernel("auto")
        c.set_scrub_kernel("auto")
        hooks().rsgpu_internal_set_locate_group(c.handle, 0)
        set_tiles(c, 0)


class GenBlocks(Blocks):
    ran = GENERATED  # the kernel that is expected to serve these blocks

    def check(self, u, syn=None):
        """The call under "fused" + "generated" against the model, the kernel
        that ran, and the same bytes under "two_pass"; returns the model's
        reports and lists."""
        syn = self.syndromes() if syn is None else syn
        want = [lm.report_syn(self.c, s, u) for s in syn]
        (rep, lists), names = records(self.ctx, lambda: self.locate(u))
        gf.same(rep, [w[0] for w in want])
        assert lists.tolist() == [list(map(int, w[1])) for w in want]
        ran = {n for n in (GENERATED, COMPILED, SPAN) if any(m.startswith(n) for m in names)}
        assert ran == {self.ran}, names
        self.ctx.set_locate_kernel("two_pass")
        try:
            rep2, lists2 = self.locate(u)
        finally:
            self.ctx.set_locate_kernel("fused")
        assert rep.tobytes() == rep2.tobytes() and lists.tobytes() == lists2.tobytes()
        return [w[0] for w in want], [list(map(int, w[1])) for w in want]


@pytest.mark.parametrize("kind", ["cauchy", "rs"])
@pytest.mark.parametrize("k,e", MATRICES, ids=str)
def test_every_layout(ctx, k, e, kind):
    """damage_every_code's blocks on every layout of the generated kernels.
    A Cauchy matrix is MDS: every block damaged in n <= min(u, e - 1) rows
    lists exactly the planted rows.  The gf_gen_rs_matrix codes are not all
    MDS, so beyond the model only this is asserted: of those blocks at least
    three quarters are located, which keeps the comparison from being one of
    DAMAGED with DAMAGED."""
    B = 8
    st = GenBlocks(ctx, k, e, L0, B, L0, kind=kind)
    rows = damage_every_code(st, np.random.default_rng(100 * k + e), k, e, L0)
    syn = st.syndromes()
    for u in (1, 3, 8):
        want, lists = st.check(u, syn)
        assert want[0] == want[7] == (0, lm.CLEAN, -1)
        within = [b for b in range(1, 6) if len(rows[b]) <= min(u, e - 1)]
        assert within
        if kind == "cauchy":
            for b in within:
                assert want[b][1:] == (lm.ONE_ROW if len(rows[b]) == 1 else lm.ROWS, rows[b][0]), (u, b)
                assert lists[b] == rows[b] + [N] * (u - len(rows[b])), (u, b)
        else:
            located = [b for b in within if want[b][1] in LOCATED]
            assert 4 * len(located) >= 3 * len(within), (u, within, located)
        # more rows than min(u, e - 1); two rows that share their only column
        assert want[5][1] == want[6][1] == lm.DAMAGED


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k,e", [(10, 4), (13, 20)], ids=str)
def test_lengths(ctx, k, e, L):
    """One live lane; a second tile with 2 live lanes; 3 tiles, so that with
    two tiles per workgroup the last workgroup owns a tile that does not
    exist; 3 full tiles.  The first and the last byte carry damage."""
    B = 4
    st = GenBlocks(ctx, k, e, L, B, L + 48, kind="cauchy")
    rng = np.random.default_rng(L + e)
    st.hit(rng, 1, 2, sorted({0, L - 1, *columns(rng, L, 20)}))
    for r in (1, k + 1):
        st.hit(rng, 2, r, sorted({0, L - 1, *columns(rng, L, 20)}))
    for r in (0, 5, k + 3):
        st.hit(rng, 3, r, columns(rng, L, 20))
    want, lists = st.check(8)
    assert [w[1:] for w in want] == [(lm.CLEAN, -1), (lm.ONE_ROW, 2), (lm.ROWS, 1), (lm.ROWS, 0)]
    assert lists[3][:4] == [0, 5, k + 3, N]
    st.check(2)


@pytest.mark.parametrize("k,e", [(10, 4), (9, 34)], ids=str)
def test_every_byte_of_a_lane_and_the_edges(ctx, k, e):
    """Rows 3 and k + 1 hit at all 32 bytes of lane 5 of tile 1, at byte 0 and
    at byte L0 - 1: every position of a lane's eight passes, the first lane
    of the first tile and the last live lane of the last one."""
    B = 2
    st = GenBlocks(ctx, k, e, L0, B, L0, kind="cauchy")
    rng = np.random.default_rng(3)
    cols = [0, *range(TILE + 5 * 32, TILE + 6 * 32), L0 - 1]
    for r in (3, k + 1):
        st.hit(rng, 1, r, cols)
    for u in (2, 8):
        want, lists = st.check(u)
        assert want == [(0, lm.CLEAN, -1), (34, lm.ROWS, 3)]
        assert lists[1][:2] == [3, k + 1]
    assert st.check(1)[0][1] == (34, lm.DAMAGED, -1)


@pytest.mark.parametrize("tpw,cap", [(0, 0), (0, 3), (1, 0), (2, 0), (3, 0)])
def test_the_merge_across_tiles_and_workgroups(ctx, tpw, cap):
    """(13, 20), two waves of 10 rows: row a is hit only in tile 0, row b only
    in tile 1, row c only in the 160-byte last tile.  With two or three tiles
    per workgroup (0: the library's choice, two) tiles 0 and 1 share a
    workgroup, whose wave 0 merges their bases into one slot, and the finish
    merges that slot with tile 3's; with one tile per workgroup the finish
    merges three.  All three rows are listed.  Again in groups of 3 blocks."""
    k, e, B = 13, 20, 8
    st = GenBlocks(ctx, k, e, L0, B, L0, kind="cauchy")
    rng = np.random.default_rng(8)
    truth = []
    for b in range(B):
        a_, b_, c_ = sorted(int(r) for r in rng.choice(k + e, 3, replace=False))
        st.hit(rng, b, a_, columns(rng, TILE, 30))
        st.hit(rng, b, b_, TILE + columns(rng, TILE, 30))
        st.hit(rng, b, c_, 3 * TILE + columns(rng, 160, 1 + b % 5))
        truth.append([a_, b_, c_])
    set_tiles(ctx, tpw)
    assert hooks().rsgpu_internal_set_locate_group(ctx.handle, cap) == 0
    try:
        for u in (3, 8):
            want, lists = st.check(u)
            assert [w[1:] for w in want] == [(lm.ROWS, t[0]) for t in truth]
            assert [l[:3] for l in lists] == truth
    finally:
        hooks().rsgpu_internal_set_locate_group(ctx.handle, 0)
        set_tiles(ctx, 0)


def test_more_claimed_slots_than_the_finish_reads_at_once(ctx):
    """(6, 3), 140 tiles, one bad column in every tile, rows 1 and 7 by turns:
    140 claimed slots of one vector each, read 64 headers at a time."""
    k, e, B, T = 6, 3, 2, 140
    L = T * TILE
    st = GenBlocks(ctx, k, e, L, B, L, kind="cauchy")
    rng = np.random.default_rng(140)
    for b in range(B):
        at = rng.integers(0, TILE, T)
        for r in (1, 7):
            tiles = np.arange(T)[(np.arange(T) % 2) == (r == 7)]
            st.hit(rng, b, r, tiles * TILE + at[tiles])
    syn = st.syndromes()
    want, lists = st.check(8, syn)
    assert want == [(T, lm.ROWS, 1)] * B and [l[:3] for l in lists] == [[1, 7, N]] * B
    assert st.check(1, syn)[0] == [(T, lm.DAMAGED, -1)] * B


def test_overflow(ctx):
    """(9, 34), four waves, one tile: blocks 0 and 1 damaged in 8 rows (ROWS
    at u = 8, DAMAGED at u = 7), blocks 2 and 3 in 9 (DAMAGED)."""
    k, e, L, B = 9, 34, TILE, 4
    st = GenBlocks(ctx, k, e, L, B, L, kind="cauchy")
    rng = np.random.default_rng(k)
    truth = []
    for b in range(B):
        rows = sorted(int(r) for r in rng.choice(k + e, 8 if b < 2 else 9, replace=False))
        for r in rows:
            st.hit(rng, b, r, columns(rng, L, 12))
        truth.append(rows)
    syn = st.syndromes()
    want, lists = st.check(8, syn)
    assert [w[1:] for w in want] == [(lm.ROWS, truth[0][0]), (lm.ROWS, truth[1][0])] + [(lm.DAMAGED, -1)] * 2
    assert lists[:2] == truth[:2]
    assert all(w[1:] == (lm.DAMAGED, -1) for w in st.check(7, syn)[0])


def test_two_groups(ctx):
    """65535 + 5 blocks of (6, 3), one lane each: two consecutive groups;
    damage on both sides of the seam."""
    k, e, L = 6, 3, 32
    B = 65535 + 5
    st = GenBlocks(ctx, k, e, L, B, L, kind="cauchy")
    rng = np.random.default_rng(6)
    truth = {0: [1], 65534: [0, 4], 65535: [2, 7], 65536: [3], B - 1: [1, 6]}
    for b, rows in truth.items():
        for r in rows:
            st.hit(rng, b, r, columns(rng, L, 6))
    want, lists = st.check(8)
    for b, rows in truth.items():
        assert want[b][1:] == (lm.ONE_ROW if len(rows) == 1 else lm.ROWS, rows[0])
        assert lists[b][:len(rows)] == rows
    assert sum(w[1] != lm.CLEAN for w in want) == len(truth)


FALLBACKS = [(10, 4, "cauchy", 4099, 4352, 0, SPAN), (10, 4, "cauchy", L0, L0, 3, SPAN),
             (16, 4, "rs", L0, L0, 0, COMPILED)]


@pytest.mark.parametrize("k,e,kind,L,pitch,offset,ran", FALLBACKS, ids=str)
def test_fallback(ctx, k, e, kind, L, pitch, offset, ran):
    """Under both settings: a len that is no multiple of 32 and misaligned
    rows run TWO_PASS; a compiled code without `coef` runs k_rs_bs_locate,
    which takes precedence.  The outputs are the model's."""
    B = 4
    st = GenBlocks(ctx, k, e, L, B, pitch, offset, kind=kind)
    st.ran = ran
    rng = np.random.default_rng(L + offset)
    st.hit(rng, 1, 2, sorted({0, L - 1, *columns(rng, L, 20)}))
    for r in (1, k + 1):
        st.hit(rng, 2, r, columns(rng, L, 20))
    for r in (0, 5, k + 3):
        st.hit(rng, 3, r, columns(rng, L, 20))
    want, _ = st.check(8)
    assert [w[1:] for w in want] == [(lm.CLEAN, -1), (lm.ONE_ROW, 2), (lm.ROWS, 1), (lm.ROWS, 0)]
    st.check(2)


def test_e_above_64_is_unsupported(ctx):
    st = GenBlocks(ctx, 4, 65, 64, 2, 64)
    rep = torch.full((2 * rsgpu.SCRUB_REPORT_DTYPE.itemsize,), gf.POISON, dtype=torch.uint8, device=st.dev)
    rows = torch.full((2 * 8,), gf.POISON, dtype=torch.uint8, device=st.dev)
    with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_UNSUPPORTED"):
        ctx.locate_blocks(4, 65, 64, 64, 2, st.src, st.par, 8, rows, rep)
    torch.cuda.synchronize()
    assert (rep.cpu().numpy() == gf.POISON).all() and (rows.cpu().numpy() == gf.POISON).all()


def test_timing_records(ctx):
    """The generated form needs both settings; with both, a call after the
    first leaves k_rs_jit_locate and k_locate_finish and nothing else."""
    st = GenBlocks(ctx, 10, 4, L0, 2, L0)
    st.locate(8)  # warm-up: the program is built
    _, names = records(ctx, lambda: st.locate(8))
    assert names == {GENERATED, "k_locate_finish"}
    for locate, scrub in (("fused", "auto"), ("auto", "generated"), ("two_pass", "generated")):
        ctx.set_locate_kernel(locate)
        ctx.set_scrub_kernel(scrub)
        try:
            _, names = records(ctx, lambda: st.locate(8))
        finally:
            ctx.set_locate_kernel("fused")
            ctx.set_scrub_kernel("generated")
        assert {SPAN, "k_locate_finish"} <= names and GENERATED not in names and COMPILED not in names, \
            (locate, scrub, names)


def test_heal(ctx):
    """GpuEncoder.heal follows the context's settings: (10, 4) Cauchy, blocks
    with 0 to 3 damaged rows are the originals again over their whole pitch,
    the degenerate block stays as it was."""
    k, e, L, B = 10, 4, 4096, 6
    enc = rsgpu.GpuEncoder(k, L, e, blocks=B, seed=5, ctx=ctx, coef=gf.matrix(k, e, "cauchy"))
    enc.src.fill_(0x6B)
    enc.par.fill_(0x6B)
    ctx.fill_synthetic(enc.src, B * k, L, enc.pitch, 5, 0)
    enc.encode_all()
    torch.cuda.synchronize()
    orig = enc.src.clone(), enc.par.clone()
    vs, vp = enc.src.view(B, k, enc.pitch), enc.par.view(B, e, enc.pitch)
    rng = np.random.default_rng(77)

    def hit(b, r, cols):
        t = vs[b, r] if r < k else vp[b, r - k]
        x = torch.from_numpy(rng.integers(1, 256, len(cols)).astype(np.uint8)).to(t.device)
        t[torch.from_numpy(np.asarray(cols, np.int64)).to(t.device)] ^= x

    truth = []
    for b in range(B - 1):
        rows = sorted(int(r) for r in rng.choice(k + e, b % 4, replace=False))
        for r in rows:
            hit(b, r, sorted({0, L - 1, *columns(rng, L, 40)}))
        truth.append(rows)
    hit(B - 1, 2, [100])
    hit(B - 1, k + 1, [100])
    torch.cuda.synchronize()
    damaged = enc.src.clone(), enc.par.clone()
    (found, rebuilt), names = records(ctx, enc.heal)
    assert GENERATED in names and not any(n.startswith(SPAN) for n in names)
    status = {0: lm.CLEAN, 1: lm.ONE_ROW, 2: lm.ROWS, 3: lm.ROWS}
    assert [(int(r["status"]), int(r["row"])) for r in found] == \
        [(status[len(t)], t[0] if t else -1) for t in truth] + [(lm.DAMAGED, -1)]
    gf.same(rebuilt, [(0, dm.CLEAN, -1)] * B)
    want_s, want_p = orig[0].clone(), orig[1].clone()
    want_s.view(B, k, enc.pitch)[B - 1] = damaged[0].view(B, k, enc.pitch)[B - 1]
    want_p.view(B, e, enc.pitch)[B - 1] = damaged[1].view(B, e, enc.pitch)[B - 1]
    assert torch.equal(enc.src, want_s) and torch.equal(enc.par, want_p)
    rep, lists = enc.locate(u=3)
    assert [int(s) for s in rep["status"]] == [lm.CLEAN] * (B - 1) + [lm.DAMAGED] and (lists == N).all()


def test_the_encode_and_the_locate_share_one_program(ctx):
    """A matrix this context has not met: after an encode under
    set_encode_kernel("generated") the first locate records its two kernels
    and nothing that builds a program, and lists what the model lists."""
    k, e, L, B = 7, 5, L0, 3
    c = gf.matrix(k, e, "cauchy")
    st = GenBlocks(ctx, k, e, L, B, L, c=c)
    spare = st.alloc(e)
    ctx.set_encode_kernel("generated")
    try:
        _, enc = records(ctx, lambda: ctx.encode_blocks(k, e, L, L, B, st.src, spare, coef=c))
    finally:
        ctx.set_encode_kernel("auto")
    assert "k_rs_jit(encode)" in enc
    torch.cuda.synchronize()
    assert torch.equal(spare[: B * e * L], st.par[: B * e * L])
    rng = np.random.default_rng(75)
    for r in (2, k + 4):
        st.hit(rng, 1, r, columns(rng, L, 25))
    _, names = records(ctx, lambda: st.locate(8))
    assert names == {GENERATED, "k_locate_finish"}
    want, lists = st.check(8)
    assert want[1][1:] == (lm.ROWS, 2) and lists[1][:3] == [2, k + 4, N]
