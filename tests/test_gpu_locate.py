"""Locating several damaged rows per block on the GPU (include/rsgpu.h
rsgpu_locate_blocks): synthetic blocks (tests/gpu_family.py DeviceBlocks)
damaged on the device, reports and lists compared field by field with the numpy
model of the contract (tests/locate_model.py) on the blocks as read back.
Every call is checked to leave the source and parity allocations as they
were.  Every allocation is filled with 0x6B first."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import degraded_model as dm  # noqa: E402
import gpu_family as gf  # noqa: E402
import locate_model as lm  # noqa: E402
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402

N = dm.NONE
DT = rsgpu.SCRUB_REPORT_DTYPE
POISON = gf.POISON


def hooks():
    H = rsgpu.testhooks()
    H.rsgpu_internal_set_locate_group.argtypes = [C.c_void_p, C.c_longlong]
    return H


@pytest.fixture(scope="module")
def ctx():
    for c in gf.device_context():
        yield c
        hooks().rsgpu_internal_set_locate_group(c.handle, 0)


class Blocks(gf.DeviceBlocks):
    def hit(self, rng, blk, row, cols):
        """Random non-zero values XORed into bytes `cols` (distinct) of a row."""
        cols = np.asarray(cols, np.int64)
        x = rng.integers(1, 256, len(cols)).astype(np.uint8)
        self.rows(row)[blk, torch.from_numpy(cols).to(self.dev)] ^= torch.from_numpy(x).to(self.dev)

    def locate(self, u):
        """(reports, lists (B, u)) of the call; the rows must stay as they are."""
        rep = torch.full((self.B * DT.itemsize,), POISON, dtype=torch.uint8, device=self.dev)
        rows = torch.full((self.B * u,), POISON, dtype=torch.uint8, device=self.dev)
        before = self.snapshot()
        self.ctx.locate_blocks(self.k, self.e, self.L, self.pitch, self.B, self.src, self.par, u, rows, rep,
                               coef=self.coef)
        torch.cuda.synchronize()
        assert torch.equal(self.src_all, before[0]), "source allocation written"
        assert torch.equal(self.par_all, before[1]), "parity allocation written"
        return rep.cpu().numpy().view(DT).copy(), rows.cpu().numpy().reshape(self.B, u).copy()

    def syndromes(self):
        """Per block the syndromes (e, L) of the rows as they are on the device."""
        hs, syn = self.host(self.src, self.k), self.host(self.par, self.e).copy()
        for j in range(self.k):  # sm.syndromes, every block at once
            syn ^= sm.gf_mul(self.c[:, j][None, :, None], hs[:, j][:, None, :])
        return list(syn)

    def check(self, u, syn=None):
        """The call against the model; returns the model's reports."""
        syn = self.syndromes() if syn is None else syn
        want = [lm.report_syn(self.c, s, u) for s in syn]
        rep, lists = self.locate(u)
        gf.same(rep, [w[0] for w in want])
        assert lists.tolist() == [list(map(int, w[1])) for w in want]
        return [w[0] for w in want]


def columns(rng, L, n):
    return rng.choice(L, min(n, L), replace=False)


@pytest.mark.parametrize("kind", ["rs", "cauchy"])
def test_mixed_verdicts_in_one_call(ctx, kind):
    """(10, 4), 16 blocks: clean ones, 1, 2 and 3 damaged rows, a pair of
    parity rows, a data and a parity row, more rows than any u takes, two rows
    hit in the same single column; at u = 1, 3 and 8."""
    k, e, L, B = 10, 4, 4096, 16
    st = Blocks(ctx, k, e, L, B, L, kind=kind)
    rng = np.random.default_rng(21)
    plan = {1: [4], 2: [2, 9], 3: [0, 5, 13], 4: [k, k + 2], 5: [3, k + 1], 9: [k + 3], 15: [1, 8]}
    for b, rows in plan.items():
        for r in rows:
            st.hit(rng, b, r, columns(rng, L, 40))
    for r in rng.choice(k + e, 9, replace=False):  # block 6: 9 rows
        st.hit(rng, 6, int(r), columns(rng, L, 40))
    st.hit(rng, 7, 2, [1234])  # block 7: the degenerate column
    st.hit(rng, 7, 6, [1234])
    st.hit(rng, 15, 1, [0])  # block 15 also in the first and the last column
    st.hit(rng, 15, 8, [L - 1])
    for b in (10, 11, 12, 13):
        for r in rng.choice(k + e, b - 10, replace=False):
            st.hit(rng, b, int(r), columns(rng, L, 40))
    syn = st.syndromes()
    for u in (1, 3, 8):
        want = st.check(u, syn)
        statuses = [w[1] for w in want]
        assert want[0] == (0, lm.CLEAN, -1) and want[1][1:] == (lm.ONE_ROW, 4)
        assert statuses[6] == statuses[7] == lm.DAMAGED
        for b in (2, 3, 4, 5, 15):
            assert statuses[b] == (lm.ROWS if len(plan[b]) <= u else lm.DAMAGED)
            assert want[b][2] == (plan[b][0] if len(plan[b]) <= u else -1)


LAYOUTS = [(4099, 4352, 0), (4099, 4101, 3), (15, 15, 0), (1, 1, 0)]


@pytest.mark.parametrize("L,pitch,offset", LAYOUTS, ids=str)
def test_layouts(ctx, L, pitch, offset):
    """A 16-byte body with a 3-byte tail; the same unaligned (the byte kernel
    alone); rows shorter than a vector; one byte.  The first and the last
    byte carry damage."""
    k, e, B = 10, 4, 6
    st = Blocks(ctx, k, e, L, B, pitch, offset)
    rng = np.random.default_rng(L)
    st.hit(rng, 1, 7, [L - 1])
    st.hit(rng, 2, 0, [0])
    st.hit(rng, 2, k + 1, [L - 1])
    for r in (2, 6, 12):
        st.hit(rng, 3, r, sorted({0, L - 1, *columns(rng, L, 20)}))
    st.hit(rng, 4, 1, [L // 2])
    st.hit(rng, 4, 9, [L // 2])
    st.hit(rng, 5, k + 3, [0])
    want = st.check(8)
    assert [w[1] for w in want][:2] == [lm.CLEAN, lm.ONE_ROW]
    if L > 1:
        assert want[2][1:] == (lm.ROWS, 0) and want[4][1] == lm.DAMAGED
    st.check(2)


@pytest.mark.parametrize("cap", [0, 3])
def test_the_merge(ctx, cap):
    """Four workgroups per block and a 5-byte tail: row a is damaged only in
    the first workgroup's columns, row b only in the last one's, row c only in
    the tail, so that no workgroup sees more than one of them; all three are
    listed.  Again with groups of 3 blocks."""
    k, e, B = 10, 4, 8
    L = 4 * 256 * 16 + 5
    st = Blocks(ctx, k, e, L, B, (L + 255) // 256 * 256)
    rng = np.random.default_rng(8)
    truth = []
    for b in range(B):
        a_, b_, c_ = sorted(int(r) for r in rng.choice(k + e, 3, replace=False))
        st.hit(rng, b, a_, columns(rng, 4096, 30))
        st.hit(rng, b, b_, 3 * 4096 + columns(rng, 4096, 30))
        st.hit(rng, b, c_, [L - 1 - (b % 5)])
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


def test_more_blocks_than_a_grid(ctx):
    """65535 + 5 blocks of (3, 3), 16 bytes each: two consecutive slices;
    damage on both sides of the seam."""
    k, e, L = 3, 3, 16
    B = 65535 + 5
    st = Blocks(ctx, k, e, L, B, L)
    rng = np.random.default_rng(6)
    truth = {0: [1], 65534: [0, 4], 65535: [2, 5], 65536: [3], B - 1: [1, 2]}
    for b, rows in truth.items():
        for r in rows:
            st.hit(rng, b, r, columns(rng, L, 6))
    want = st.check(8)
    for b, rows in truth.items():
        assert want[b][1:] == (lm.ONE_ROW if len(rows) == 1 else lm.ROWS, rows[0])
    assert sum(w[1] != lm.CLEAN for w in want) == len(truth)


def test_every_lane_carries_a_coordinate(ctx):
    """(8, 64): e is the wave's width; the last parity row is lane 63."""
    k, e, L, B = 8, 64, 512, 3
    st = Blocks(ctx, k, e, L, B, L)
    rng = np.random.default_rng(64)
    for r in (1, 6, k + 40):
        st.hit(rng, 0, r, columns(rng, L, 6))
    st.hit(rng, 1, 0, columns(rng, L, 6))
    st.hit(rng, 1, k + 63, columns(rng, L, 6))
    want = st.check(8)
    assert [w[1:] for w in want] == [(lm.ROWS, 1), (lm.ROWS, 0), (lm.CLEAN, -1)]


def test_eight_rows_of_64_32(ctx):
    k, e, L, B = 64, 32, 2048, 4
    st = Blocks(ctx, k, e, L, B, L)
    rng = np.random.default_rng(32)
    truth = []
    for b in range(B):
        rows = sorted(int(r) for r in rng.choice(k + e, 8, replace=False))
        for r in rows:
            st.hit(rng, b, r, columns(rng, L, 12))
        truth.append(rows)
    syn = st.syndromes()
    want = st.check(8, syn)
    assert [w[1:] for w in want] == [(lm.ROWS, t[0]) for t in truth]
    want = st.check(7, syn)
    assert all(w[1:] == (lm.DAMAGED, -1) for w in want)


WIDE = [(100, 20, "rs"), (245, 5, "cauchy"), (213, 37, "rs")]


def wide_rows(k, e):
    """The damaged rows of the six blocks of a wide shape: none; one row past
    the first 64-row band; two rows of different bands; min(8, e - 1) rows
    that go round the 64-row bands of the k + e rows, the last of them the
    first parity row (in the last band); a data row and the last parity row;
    nine rows, more than any u takes."""
    n = min(8, e - 1)
    bands = (k + e + 63) // 64
    spread = sorted((i % bands) * 64 + 1 + 2 * i for i in range(n - 1))
    assert len(set(spread)) == n - 1 and spread[-1] < k
    return [[], [k - 2], [5, 64 + (k - 64) // 2], spread + [k], [65, k + e - 1],
            sorted({3, 40, 63, 64, 70, k - 1, k, k + 1, k + e - 1})]


@pytest.mark.parametrize("k,e,kind", WIDE, ids=str)
def test_more_rows_than_a_wave_has_lanes(ctx, k, e, kind):
    """k > 64 under the TWO_PASS kernel: k_locate_finish walks the members of
    all k + e rows against the basis k_locate_span left.  The model must name
    exactly the planned rows of blocks 1..4."""
    L, B = 2048, 6
    st = Blocks(ctx, k, e, L, B, L, kind=kind)
    rng = np.random.default_rng(k)
    plan = wide_rows(k, e)
    for b, rows in enumerate(plan):
        for r in rows:
            st.hit(rng, b, r, columns(rng, L, 12))
    syn = st.syndromes()
    ctx.set_locate_kernel("two_pass")
    try:
        for u in (8, 2):
            want = [lm.report_syn(st.c, s, u) for s in syn]
            for b in range(1, 5):
                if len(plan[b]) <= u:
                    assert want[b][0][1:] == (lm.ONE_ROW if len(plan[b]) == 1 else lm.ROWS, plan[b][0]), (u, b)
                    assert list(want[b][1][: len(plan[b])]) == plan[b], (u, b)
                else:
                    assert want[b][0][1:] == (lm.DAMAGED, -1), (u, b)
            assert want[0][0] == (0, lm.CLEAN, -1) and want[5][0][1:] == (lm.DAMAGED, -1)
            assert st.check(u, syn) == [w[0] for w in want]
    finally:
        ctx.set_locate_kernel("auto")
    assert plan[1][0] >= 64 and plan[2][0] // 64 != plan[2][1] // 64 and len(plan[3]) == min(8, e - 1)
    assert {r // 64 for r in plan[3]} == set(range((k + e + 63) // 64)) and plan[3][-1] == k


def test_heal_above_64_sources(ctx):
    """GpuEncoder.heal at (100, 20): rows 70, 99 and the last parity row of
    block 1 are located and rebuilt, the blocks are the original encode."""
    k, e, L, B = 100, 20, 4096, 3
    enc = rsgpu.GpuEncoder(k, L, e, blocks=B, seed=9, ctx=ctx)
    enc.encode_all()
    torch.cuda.synchronize()
    orig = enc.src.clone(), enc.par.clone()
    rng = np.random.default_rng(100)
    rows = [70, 99, 100 + 19]
    for r in rows:
        t = enc.src.view(B, k, enc.pitch)[1, r] if r < k else enc.par.view(B, e, enc.pitch)[1, r - k]
        cols = sorted({0, L - 1, *columns(rng, L, 20)})
        x = torch.from_numpy(rng.integers(1, 256, len(cols)).astype(np.uint8)).to(t.device)
        t[torch.from_numpy(np.asarray(cols, np.int64)).to(t.device)] ^= x
    torch.cuda.synchronize()
    assert not torch.equal(enc.src, orig[0]) and not torch.equal(enc.par, orig[1])
    found, rebuilt = enc.heal()
    assert [(int(r["status"]), int(r["row"])) for r in found] == [(lm.CLEAN, -1), (lm.ROWS, 70), (lm.CLEAN, -1)]
    gf.same(rebuilt, [(0, dm.CLEAN, -1)] * B)
    assert torch.equal(enc.src, orig[0]) and torch.equal(enc.par, orig[1])


def test_edges_of_e_and_len(ctx):
    rng = np.random.default_rng(1)
    one = Blocks(ctx, 6, 1, 256, 2, 256)
    one.hit(rng, 1, 3, [17])
    assert one.check(8) == [(0, lm.CLEAN, -1), (1, lm.DAMAGED, -1)]
    # e == 0 and len == 0: every block CLEAN, every list empty
    for k, e, L in ((6, 0, 64), (6, 4, 0)):
        st = Blocks(ctx, k, e, L, 3, 64, encode=False)
        rep, lists = st.locate(4)
        gf.same(rep, [(0, lm.CLEAN, -1)] * 3)
        assert (lists == N).all()
    # e == 65: refused, nothing enqueued, both outputs keep their fill
    st = Blocks(ctx, 8, 65, 64, 1, 64, encode=False)
    rep = torch.full((DT.itemsize,), POISON, dtype=torch.uint8, device=st.dev)
    rows = torch.full((8,), POISON, dtype=torch.uint8, device=st.dev)
    with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_UNSUPPORTED"):
        ctx.locate_blocks(8, 65, 64, 64, 1, st.src, st.par, 8, rows, rep)
    for u in (0, 9):
        with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_ARG"):
            ctx.locate_blocks(8, 4, 64, 64, 1, st.src, st.par, u, rows, rep)
    with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_ARG"):
        ctx.locate_blocks(8, 4, 64, 64, 1, st.src, st.par, 8, rows, rep[4:])
    torch.cuda.synchronize()
    assert (rep.cpu().numpy() == POISON).all() and (rows.cpu().numpy() == POISON).all()


@pytest.mark.parametrize("k,e,kind", [(16, 4, "rs"), (10, 4, "cauchy")], ids=str)
def test_equal_to_the_scrub(ctx, k, e, kind):
    """Locatable matrices, clean blocks and blocks with one damaged row: the
    reports are rsgpu_scrub_blocks' with LOCATE, byte for byte."""
    L, B = 2080, 8
    st = Blocks(ctx, k, e, L, B, L + 48, kind=kind)
    assert sm.locatable(st.c)
    rng = np.random.default_rng(k)
    for b, r in ((1, 0), (2, k - 1), (3, k), (5, k + e - 1), (6, 7)):
        st.hit(rng, b, r, sorted({0, L - 1, *columns(rng, L, b)}))
    rep, lists = st.locate(8)
    srep = torch.full((B * DT.itemsize,), POISON, dtype=torch.uint8, device=st.dev)
    ctx.scrub_blocks(k, e, L, st.pitch, B, st.src, st.par, srep, coef=st.coef, locate=True)
    torch.cuda.synchronize()
    assert rep.tobytes() == srep.cpu().numpy().tobytes()
    assert [int(s) for s in rep["status"]] == [0, 1, 1, 1, 0, 1, 1, 0]
    assert lists[:, 0].tolist() == [N, 0, k - 1, k, N, k + e - 1, 7, N] and (lists[:, 1:] == N).all()


def test_heal_end_to_end(ctx):
    """GpuEncoder.heal on blocks with 0 to 3 damaged rows and one DAMAGED
    block: every located block is the original again, over its whole pitch;
    the DAMAGED block stays as it was."""
    k, e, L, B = 10, 4, 4099, 9
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
    found, rebuilt = enc.heal()
    status = {0: lm.CLEAN, 1: lm.ONE_ROW, 2: lm.ROWS, 3: lm.ROWS}
    assert [(int(r["status"]), int(r["row"])) for r in found] == \
        [(status[len(t)], t[0] if t else -1) for t in truth] + [(lm.DAMAGED, -1)]
    gf.same(rebuilt, [(0, dm.CLEAN, -1)] * B)
    want_s, want_p = orig[0].clone(), orig[1].clone()
    want_s.view(B, k, enc.pitch)[B - 1] = damaged[0].view(B, k, enc.pitch)[B - 1]
    want_p.view(B, e, enc.pitch)[B - 1] = damaged[1].view(B, e, enc.pitch)[B - 1]
    assert torch.equal(enc.src, want_s) and torch.equal(enc.par, want_p)
    # locate alone: the lists as the rebuild takes them
    rep, lists = enc.locate(u=3)
    assert [int(s) for s in rep["status"]] == [lm.CLEAN] * (B - 1) + [lm.DAMAGED] and (lists == N).all()


def test_timing_records(ctx):
    """k_locate_span, its (tail) and (bytes) forms and k_locate_finish."""
    seen = set()
    ctx.timing_enable(True)
    try:
        for L, pitch, offset in LAYOUTS[:2]:
            st = Blocks(ctx, 10, 4, L, 2, pitch, offset)
            ctx.timing_read()
            st.locate(8)
            seen.update(n for n, _, nb in ctx.timing_read() if n.startswith("k_locate") and nb == 2)
    finally:
        ctx.timing_enable(False)
    assert seen == {"k_locate_span", "k_locate_span(tail)", "k_locate_span(bytes)", "k_locate_finish"}
