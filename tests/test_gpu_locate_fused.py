"""rsgpu_locate_blocks under rsgpu_set_locate_kernel FUSED (k_rs_bs_locate,
include/rsgpu.h): the blocks and the model of tests/test_gpu_locate.py, the
context set to "fused".  Every call is compared field by field with the numpy
model (tests/locate_model.py), must leave both allocations as they were, must
have run the kernel the case expects (the timing records say which), and a
second call under "two_pass" must give the same bytes, reports and lists.

The fused kernel's tile is 2048 bytes, a lane's share 32: L0 = 3 * 2048 + 5 *
32 gives three full tiles and one whose last 59 lanes are idle."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import degraded_model as dm  # noqa: E402
import gpu_family as gf  # noqa: E402
import locate_model as lm  # noqa: E402
import rsgpu  # noqa: E402
from test_gpu_locate import Blocks, columns, hooks  # noqa: E402

N = dm.NONE
DT = rsgpu.SCRUB_REPORT_DTYPE
POISON = gf.POISON
TILE = 2048
L0 = 3 * TILE + 5 * 32
CODES = [(16, 4), (16, 8), (64, 32), (64, 16), (100, 20), (5, 4), (20, 7)]
LOCATED = (lm.ONE_ROW, lm.ROWS)


@pytest.fixture(scope="module")
def ctx():
    for c in gf.device_context():
        c.set_locate_kernel("fused")
        yield c
        c.set_locate_kernel("auto")
        hooks().rsgpu_internal_set_locate_group(c.handle, 0)


def records(ctx, call):
    """call()'s result and the names of the timing records it left."""
    out = []
    names = gf.recorded(ctx, lambda: out.append(call()))
    return out[0], set(names)


class FusedBlocks(Blocks):
    fused = True  # the fused kernel is expected to serve these blocks

    def check(self, u, syn=None):
        """The call under "fused" against the model, the kernel that ran, and
        the same bytes under "two_pass"; returns the model's reports."""
        syn = self.syndromes() if syn is None else syn
        want = [lm.report_syn(self.c, s, u) for s in syn]
        (rep, lists), names = records(self.ctx, lambda: self.locate(u))
        gf.same(rep, [w[0] for w in want])
        assert lists.tolist() == [list(map(int, w[1])) for w in want]
        span = any(n.startswith("k_locate_span") for n in names)
        assert ("k_rs_bs_locate" in names, span) == (self.fused, not self.fused), names
        self.ctx.set_locate_kernel("two_pass")
        try:
            rep2, lists2 = self.locate(u)
        finally:
            self.ctx.set_locate_kernel("fused")
        assert rep.tobytes() == rep2.tobytes() and lists.tobytes() == lists2.tobytes()
        return [w[0] for w in want]


def damage_every_code(st, rng, k, e, L):
    """Block 0 clean; blocks 1 to 4: 1, 2, 3 and min(8, e - 1) rows of data and
    parity together, 40 columns each; block 5 one row more than that; block 6
    two rows hit only in one shared column; block 7 clean.  Returns the rows."""
    most = min(8, e - 1)
    plan = {1: 1, 2: 2, 3: 3, 4: most, 5: most + 1}
    rows = {}
    for b, n in plan.items():
        rows[b] = sorted(int(r) for r in rng.choice(k + e, n, replace=False))
        for r in rows[b]:
            st.hit(rng, b, r, columns(rng, L, 40))
    rows[6] = sorted(int(r) for r in rng.choice(k + e, 2, replace=False))
    col = [int(rng.integers(0, L))]
    for r in rows[6]:
        st.hit(rng, 6, r, col)
    return rows


@pytest.mark.parametrize("k,e", CODES, ids=str)
def test_every_compiled_code(ctx, k, e):
    """Statuses are the model's; the gf_gen_rs_matrix codes are not all MDS
    ((16, 8): some draws of 7 rows come out DAMAGED), so beyond the model only
    this is asserted: of the blocks damaged in at most min(u, e - 1) rows, at
    least three quarters are located, which keeps the comparison from being
    one of DAMAGED with DAMAGED."""
    B = 8
    st = FusedBlocks(ctx, k, e, L0, B, L0)
    rows = damage_every_code(st, np.random.default_rng(100 * k + e), k, e, L0)
    syn = st.syndromes()
    for u in (1, 3, 8):
        want = st.check(u, syn)
        assert want[0] == want[7] == (0, lm.CLEAN, -1)
        within = [b for b, r in rows.items() if len(r) <= min(u, e - 1)]
        located = [b for b in within if want[b][1] in LOCATED]
        assert within and 4 * len(located) >= 3 * len(within), (u, within, located)
        assert want[5][1] == want[6][1] == lm.DAMAGED  # more rows than min(u, e - 1); one shared column


@pytest.mark.parametrize("cap", [0, 3])
def test_the_merge_across_tiles(ctx, cap):
    """(16, 4): row a is hit only in tile 0, row b only in tile 2, row c only
    in the 160-byte last tile, so that no workgroup sees more than one of
    them and the finish merges three claimed slots; all three are listed.
    Again with groups of 3 blocks."""
    k, e, B = 16, 4, 8
    st = FusedBlocks(ctx, k, e, L0, B, L0)
    rng = np.random.default_rng(8)
    truth = []
    for b in range(B):
        a_, b_, c_ = sorted(int(r) for r in rng.choice(k + e, 3, replace=False))
        st.hit(rng, b, a_, columns(rng, TILE, 30))
        st.hit(rng, b, b_, 2 * TILE + columns(rng, TILE, 30))
        st.hit(rng, b, c_, 3 * TILE + columns(rng, 160, 1 + b % 5))
        truth.append((a_, b_, c_))
    assert hooks().rsgpu_internal_set_locate_group(ctx.handle, cap) == 0
    try:
        for u in (3, 8):
            want = st.check(u)
            assert [w[1:] for w in want] == [(lm.ROWS, t[0]) for t in truth]
            rep, lists = st.locate(u)
            assert [tuple(l[:3]) for l in lists.tolist()] == truth
    finally:
        hooks().rsgpu_internal_set_locate_group(ctx.handle, 0)


def test_every_byte_of_a_lane_and_the_edges(ctx):
    """(16, 4): rows 3 and 17 hit at all 32 bytes of lane 5 of tile 1, at
    byte 0 and at byte L0 - 1: every position of a lane's four passes, the
    first lane of the first tile and the last live lane of the last one."""
    k, e, B = 16, 4, 2
    st = FusedBlocks(ctx, k, e, L0, B, L0)
    rng = np.random.default_rng(3)
    cols = [0, *range(TILE + 5 * 32, TILE + 6 * 32), L0 - 1]
    for r in (3, 17):
        st.hit(rng, 1, r, cols)
    for u in (2, 8):
        want = st.check(u)
        assert want == [(0, lm.CLEAN, -1), (34, lm.ROWS, 3)]
        assert st.locate(u)[1][1, :2].tolist() == [3, 17]
    assert st.check(1)[1] == (34, lm.DAMAGED, -1)


def test_more_dirty_tiles_than_the_finish_reads_at_once(ctx):
    """(5, 4), 70 tiles, one bad column in every tile, rows 1 and 7 by turns:
    70 claimed slots of one vector each, read 64 headers at a time."""
    k, e, B = 5, 4, 2
    L = 70 * TILE
    st = FusedBlocks(ctx, k, e, L, B, L)
    rng = np.random.default_rng(70)
    for b in range(B):
        at = rng.integers(0, TILE, 70)
        for r in (1, 7):
            tiles = np.arange(70)[(np.arange(70) % 2) == (r == 7)]
            st.hit(rng, b, r, tiles * TILE + at[tiles])
    syn = st.syndromes()
    assert st.check(8, syn) == [(70, lm.ROWS, 1)] * B
    assert st.locate(8)[1][:, :3].tolist() == [[1, 7, N]] * B
    assert st.check(1, syn) == [(70, lm.DAMAGED, -1)] * B


@pytest.mark.parametrize("k,e", [(64, 32), (100, 20)], ids=str)
def test_four_waves_and_wide_e(ctx, k, e):
    """One tile, four waves with 8 and 5 rows each: blocks 0 and 1 damaged in
    8 rows (ROWS at u = 8, DAMAGED at u = 7), blocks 2 and 3 in 9 (DAMAGED)."""
    L, B = TILE, 4
    st = FusedBlocks(ctx, k, e, L, B, L)
    rng = np.random.default_rng(k)
    truth = []
    for b in range(B):
        rows = sorted(int(r) for r in rng.choice(k + e, 8 if b < 2 else 9, replace=False))
        for r in rows:
            st.hit(rng, b, r, columns(rng, L, 12))
        truth.append(rows)
    syn = st.syndromes()
    want = st.check(8, syn)
    assert [w[1:] for w in want] == [(lm.ROWS, truth[0][0]), (lm.ROWS, truth[1][0])] + [(lm.DAMAGED, -1)] * 2
    assert st.locate(8)[1][:2].tolist() == truth[:2]
    want = st.check(7, syn)
    assert all(w[1:] == (lm.DAMAGED, -1) for w in want)


def test_two_slices(ctx):
    """65535 + 5 blocks of (5, 4), one lane each: two consecutive groups;
    damage on both sides of the seam."""
    k, e, L = 5, 4, 32
    B = 65535 + 5
    st = FusedBlocks(ctx, k, e, L, B, L)
    rng = np.random.default_rng(6)
    truth = {0: [1], 65534: [0, 4], 65535: [2, 5], 65536: [3], B - 1: [1, 2]}
    for b, rows in truth.items():
        for r in rows:
            st.hit(rng, b, r, columns(rng, L, 6))
    want = st.check(8)
    for b, rows in truth.items():
        assert want[b][1:] == (lm.ONE_ROW if len(rows) == 1 else lm.ROWS, rows[0])
    assert sum(w[1] != lm.CLEAN for w in want) == len(truth)


FALLBACKS = [(10, 4, "rs", L0, L0, 0), (16, 4, "cauchy", L0, L0, 0), (16, 4, "rs", 4099, 4352, 0),
             (16, 4, "rs", L0, L0, 3)]


@pytest.mark.parametrize("k,e,kind,L,pitch,offset", FALLBACKS, ids=str)
def test_fallback(ctx, k, e, kind, L, pitch, offset):
    """A code that is not compiled, a `coef`, a len that is no multiple of 32,
    misaligned rows: TWO_PASS runs under "fused" (k_locate_span in the
    records, no k_rs_bs_locate) and the outputs are the model's."""
    B = 4
    st = FusedBlocks(ctx, k, e, L, B, pitch, offset, kind=kind)
    st.fused = False
    rng = np.random.default_rng(L + offset)
    st.hit(rng, 1, 2, sorted({0, L - 1, *columns(rng, L, 20)}))
    for r in (1, k + 1):
        st.hit(rng, 2, r, columns(rng, L, 20))
    for r in (0, 5, k + 3):
        st.hit(rng, 3, r, columns(rng, L, 20))
    want = st.check(8)
    assert [w[1:] for w in want] == [(lm.CLEAN, -1), (lm.ONE_ROW, 2), (lm.ROWS, 1), (lm.ROWS, 0)]
    st.check(2)


def test_timing_records(ctx):
    """Under "fused" a call leaves k_rs_bs_locate and k_locate_finish and
    nothing else; under "auto" what it left before the setter existed."""
    st = FusedBlocks(ctx, 16, 4, L0, 2, L0)
    _, names = records(ctx, lambda: st.locate(8))
    assert names == {"k_rs_bs_locate", "k_locate_finish"}
    ctx.set_locate_kernel("auto")
    try:
        _, names = records(ctx, lambda: st.locate(8))
    finally:
        ctx.set_locate_kernel("fused")
    assert {"k_locate_span", "k_locate_finish"} <= names and "k_rs_bs_locate" not in names
    assert all(n.startswith(("k_locate", "k_rs_bs")) for n in names), names


def test_heal(ctx):
    """GpuEncoder.heal follows the context's setting: blocks with 0 to 3
    damaged rows are the originals again over their whole pitch, the
    degenerate block stays as it was."""
    k, e, L, B = 16, 4, 4096, 6
    enc = rsgpu.GpuEncoder(k, L, e, blocks=B, seed=5, ctx=ctx)
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
    assert "k_rs_bs_locate" in names and not any(n.startswith("k_locate_span") for n in names)
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


def test_setter(ctx):
    """An unknown name raises; an unknown value is RSGPU_ERR_ARG and leaves
    the setting ("fused", the fixture's) as it was."""
    with pytest.raises(KeyError):
        ctx.set_locate_kernel("nonsense")
    L = rsgpu.lib()
    for bad in (3, -1):
        assert L.rsgpu_set_locate_kernel(ctx.handle, bad) == -1
    st = FusedBlocks(ctx, 16, 4, L0, 2, L0)
    _, names = records(ctx, lambda: st.locate(8))
    assert "k_rs_bs_locate" in names
