"""Correction per byte column on the GPU (include/rsgpu.h
rsgpu_correct_blocks): data from fill_synthetic, parity from encode_blocks,
rows then damaged with torch indexing as tests/correct_cases.py plans it.

As in tests/test_gpu_repair.py every case keeps a clone of the whole source
and parity allocations (padding included).  What the call must do comes from
the numpy model of the contract (tests/correct_model.py) run on each block as
read back from the device: the device's reports are compared with its verdicts
field by field, and the whole allocations with the damaged state patched by
the model's rows -- so a byte written anywhere it should not be (another row,
another block, the sentinels in [len, pitch)) fails the comparison."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import correct_cases as cc  # noqa: E402
import correct_model as cm  # noqa: E402
import gpu_family as gf  # noqa: E402
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402

DT = rsgpu.CORRECT_REPORT_DTYPE
FIELDS = ("bad_columns", "corrected_columns", "two_row_columns", "status", "row")
CLEAN = (0, 0, 0, cm.CLEAN, -1)


@pytest.fixture(scope="module")
def ctx():
    yield from gf.device_context(reset_scrub_kernel=True)


class Blocks(gf.DeviceBlocks):
    """B synthetic blocks and their parity on the device."""

    def __init__(self, ctx, k, e, kind, L, mode, B=cc.BLOCKS):
        pitch, offset = gf.pitch_of(L, mode)
        super().__init__(ctx, k, e, L, B, pitch, offset, kind)
        self.rep = torch.empty(B * DT.itemsize, dtype=torch.uint8, device=self.dev)
        torch.cuda.synchronize()
        self.pristine = self.snapshot()

    def equals(self, snap):
        return torch.equal(self.src_all, snap[0]) and torch.equal(self.par_all, snap[1])

    def restore(self, snap):
        self.src_all.copy_(snap[0])
        self.par_all.copy_(snap[1])

    def hit(self, b, hits, col):
        for row, x in hits:
            self.xor(b, row, col, x)

    def model(self, t, blocks=None):
        """The model on every block (on `blocks`, the others being clean) as
        it is now: ([verdict per block], the allocations as the call must
        leave them)."""
        want = [CLEAN] * self.B
        src, par = self.snapshot()
        sv = self.view(src[self.offset:], self.k)
        pv = self.view(par[self.offset:], self.e)
        for b in range(self.B) if blocks is None else blocks:
            s, p = self.host_block(b)
            s2, p2, want[b] = cm.correct(self.c, s, p, t)
            sv[b, :, : self.L] = torch.from_numpy(s2).to(sv.device)
            pv[b, :, : self.L] = torch.from_numpy(p2).to(pv.device)
        return want, (src, par)

    def correct(self, t, poison=gf.POISON):
        if poison is not None:
            self.rep.fill_(poison)
        self.ctx.correct_blocks(self.k, self.e, self.L, self.pitch, self.B, self.src, self.par, self.rep,
                                coef=self.coef, t=t)
        torch.cuda.synchronize()
        return self.rep.cpu().numpy().view(DT).copy()


def run(blk, t, want, after, poison=gf.POISON):
    gf.same(blk.correct(t, poison), want, FIELDS)
    assert torch.equal(blk.src_all, after[0]), "source allocation"
    assert torch.equal(blk.par_all, after[1]), "parity allocation"


@pytest.mark.parametrize("L,mode", cc.LAYOUTS, ids=str)
@pytest.mark.parametrize("k,e,kind", cc.SHAPES, ids=str)
def test_planned_damage(ctx, k, e, kind, L, mode):
    """Blocks 0 .. B - 2 damaged as planned (clean, one-row, every kind of
    pair, three-row columns), the last one clean."""
    blk = Blocks(ctx, k, e, kind, L, mode)
    for b in range(blk.B - 1):
        for _, col, hits in cc.plan(k, e, L, b):
            blk.hit(b, hits, col)
    damaged = blk.snapshot()
    want, after = blk.model(2)
    assert want[-1] == CLEAN and all(w[2] >= 9 and w[3] in (cm.REPAIRED, cm.PARTIAL) for w in want[:-1]), want
    run(blk, 2, want, after)
    # a second call on the result, into the report buffer the first one filled
    want2, after2 = blk.model(2)
    assert all(w[1] == 0 and w[3] in (cm.CLEAN, cm.DAMAGED) for w in want2) and blk.equals(after2)
    run(blk, 2, want2, after2, poison=None)
    # t = 1: the model, and rsgpu_repair_blocks' COLUMNS on a copy
    blk.restore(damaged)
    want1, after1 = blk.model(1)
    assert all(w[2] == 0 for w in want1)
    run(blk, 1, want1, after1)
    blk.restore(damaged)
    rep = torch.empty(blk.B * rsgpu.REPAIR_REPORT_DTYPE.itemsize, dtype=torch.uint8, device=blk.dev)
    ctx.repair_blocks(k, e, L, blk.pitch, blk.B, blk.src, blk.par, rep, coef=blk.coef, mode="columns")
    torch.cuda.synchronize()
    gf.same(rep.cpu().numpy().view(rsgpu.REPAIR_REPORT_DTYPE), [(w[0], w[1], w[3], w[4]) for w in want1],
            gf.REPAIR_FIELDS)
    assert blk.equals(after1)


@pytest.mark.parametrize("L,mode", [(4128, "plus48"), (4128, "mis1")], ids=str)
@pytest.mark.parametrize("k,e,kind", cc.BAND_SHAPES, ids=str)
def test_pairs_across_bands(ctx, k, e, kind, L, mode):
    """k > 64, block 1 of 3 damaged in pairs of rows inside a 64-row band,
    across bands and on both sides of every band's edge, a column each: all
    of them two-row corrections, the block the original encode again; t = 1
    leaves every byte; a second call finds the block clean."""
    blk = Blocks(ctx, k, e, kind, L, mode, B=3)
    todo = cc.band_pairs(k, e)
    for col, hits in todo:
        blk.hit(1, hits, col)
    damaged = blk.snapshot()
    n = len(todo)
    want, after = blk.model(2, [1])
    assert want == [CLEAN, (n, n, n, cm.REPAIRED, -1), CLEAN]
    assert torch.equal(after[0], blk.pristine[0]) and torch.equal(after[1], blk.pristine[1])
    want1, after1 = blk.model(1, [1])
    assert want1 == [CLEAN, (n, 0, 0, cm.DAMAGED, -1), CLEAN]
    assert torch.equal(after1[0], damaged[0]) and torch.equal(after1[1], damaged[1])
    run(blk, 1, want1, damaged)
    run(blk, 2, want, blk.pristine)
    run(blk, 2, [CLEAN] * 3, blk.pristine, poison=None)


@pytest.mark.parametrize("L,mode", [(4128, "plus48"), (4128, "mis1")], ids=str)
def test_three_rows_of_three_bands_are_left_alone(ctx, L, mode):
    """(245, 5) Cauchy: a column damaged in data rows of three different
    bands stays byte for byte, the column beside it in row 244 alone is
    corrected."""
    k, e = 245, 5
    blk = Blocks(ctx, k, e, "cauchy", L, mode, B=3)
    (col3, hits3), (col1, hits1) = cc.three_bands(k)
    blk.hit(1, hits3, col3)
    want_after = blk.snapshot()  # what the call must leave: the three-row column alone
    blk.hit(1, hits1, col1)
    want, after = blk.model(2, [1])
    assert want == [CLEAN, (2, 1, 0, cm.PARTIAL, 244), CLEAN]
    assert torch.equal(after[0], want_after[0]) and torch.equal(after[1], want_after[1])
    run(blk, 2, want, after)
    run(blk, 2, [CLEAN, (1, 0, 0, cm.DAMAGED, -1), CLEAN], after, poison=None)


@pytest.mark.parametrize("k,e,kind", [(12, 6, "cauchy"), (64, 32, "rs"), (245, 5, "cauchy"), (100, 20, "rs")], ids=str)
def test_scattered_damage_that_locate_calls_damaged(ctx, k, e, kind):
    """What the call exists for: block 1 damaged in 12 distinct rows, two per
    column.  rsgpu_locate_blocks gives it up; every column comes back."""
    L = 4128
    blk = Blocks(ctx, k, e, kind, L, "plus48", B=3)
    for col, hits in cc.scattered(k, e, L):
        blk.hit(1, hits, col)
    rows = torch.empty(blk.B * 8, dtype=torch.uint8, device=blk.dev)
    srep = torch.empty(blk.B * gf.SCRUB_DT.itemsize, dtype=torch.uint8, device=blk.dev)
    ctx.locate_blocks(k, e, L, blk.pitch, blk.B, blk.src, blk.par, 8, rows, srep, coef=blk.coef)
    torch.cuda.synchronize()
    gf.same(srep.cpu().numpy().view(gf.SCRUB_DT), [(0, sm.CLEAN, -1), (12, sm.DAMAGED, -1), (0, sm.CLEAN, -1)])
    want, after = blk.model(2)
    assert want == [CLEAN, (12, 12, 12, cm.REPAIRED, -1), CLEAN]
    assert torch.equal(after[0], blk.pristine[0]) and torch.equal(after[1], blk.pristine[1])
    run(blk, 2, want, blk.pristine)
    run(blk, 2, [CLEAN] * 3, blk.pristine, poison=None)


@pytest.mark.parametrize("L,mode", [(4128, "plus48"), (4128, "mis1")], ids=str)
def test_two_matching_pairs_leave_the_column_alone(ctx, L, mode):
    """A caller's matrix with four dependent columns of [C | I]: the columns
    two pairs explain stay byte for byte, the one beside them is corrected."""
    c = cc.dependent_matrix()
    pitch, offset = gf.pitch_of(L, mode)
    blk = Blocks.__new__(Blocks)
    gf.DeviceBlocks.__init__(blk, ctx, 12, 6, L, 2, pitch, offset, "cauchy", c=c)
    blk.rep = torch.empty(2 * DT.itemsize, dtype=torch.uint8, device=blk.dev)
    torch.cuda.synchronize()
    for col, hits in cc.AMBIGUOUS + cc.UNIQUE:
        blk.hit(1, hits, col)
    want, after = blk.model(2)
    assert want == [CLEAN, (6, 1, 1, cm.PARTIAL, -1)]
    run(blk, 2, want, after)
    run(blk, 2, [CLEAN, (5, 0, 0, cm.DAMAGED, -1)], after, poison=None)


@pytest.mark.parametrize("L,mode", [(4128, "plus48"), (4128, "mis1")], ids=str)
def test_two_matching_pairs_in_different_bands(ctx, L, mode):
    """(129, 7) with dependent columns of [C | I] in one 64-row band, in two
    neighbouring ones and in the last, one-row band: the data-pair search
    stops after the band that holds both pairs, or meets the second pair in a
    lane of a later trip; either way the column stays byte for byte."""
    c = cc.dependent_wide_matrix()
    pitch, offset = gf.pitch_of(L, mode)
    blk = Blocks.__new__(Blocks)
    gf.DeviceBlocks.__init__(blk, ctx, 129, 7, L, 2, pitch, offset, "cauchy", c=c)
    blk.rep = torch.empty(2 * DT.itemsize, dtype=torch.uint8, device=blk.dev)
    torch.cuda.synchronize()
    for col, hits in cc.AMBIGUOUS_WIDE + cc.UNIQUE_WIDE:
        blk.hit(1, hits, col)
    n = len(cc.AMBIGUOUS_WIDE)
    want, after = blk.model(2)
    assert want == [CLEAN, (n + 2, 2, 2, cm.PARTIAL, -1)]
    run(blk, 2, want, after)
    run(blk, 2, [CLEAN, (n, 0, 0, cm.DAMAGED, -1)], after, poison=None)


def test_more_blocks_than_a_grid_holds(ctx):
    """65539 blocks run as two slices: damage at the end of the first and in
    the second."""
    B = 65536 + 3
    blk = Blocks(ctx, 6, 5, "cauchy", 32, "eq", B=B)
    blk.hit(65534, [(2, 0x31), (7, 0x07)], 31)
    blk.hit(65535, [(4, 0x80)], 0)
    blk.hit(65537, [(0, 0x01), (5, 0xFE)], 16)
    blk.hit(B - 1, [(6, 0x11), (10, 0x22)], 1)
    want, after = blk.model(2, [65534, 65535, 65537, B - 1])
    assert [want[b] for b in (65534, 65535, 65537, B - 1)] == [
        (1, 1, 1, cm.REPAIRED, -1), (1, 1, 0, cm.REPAIRED, 4), (1, 1, 1, cm.REPAIRED, -1), (1, 1, 1, cm.REPAIRED, -1)]
    rep = blk.correct(2)
    assert (rep["status"] == cm.CLEAN).sum() == B - 4
    gf.same(rep[65530:], want[65530:], FIELDS)
    assert blk.equals(after) and blk.equals(blk.pristine)


def test_refusals(ctx):
    """t outside {1, 2}: RSGPU_ERR_ARG; t = 2 with e = 4, t = 1 with e = 2, a
    matrix that is not locatable: RSGPU_ERR_UNSUPPORTED.  Nothing runs: the
    report keeps its poison and the rows their damage."""
    blk = Blocks(ctx, 12, 6, "cauchy", 2048, "eq", B=2)
    blk.hit(1, [(3, 0x44)], 99)
    blk.hit(0, [(2, 0x11), (14, 0x22)], 7)
    damaged = blk.snapshot()
    for t in (0, 3, -1):
        with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_ARG"):
            blk.correct(t)
        torch.cuda.synchronize()
        assert (blk.rep.cpu().numpy() == gf.POISON).all() and blk.equals(damaged)
    bad = blk.c.copy()
    bad[1, 3] = 0
    blk.rep.fill_(gf.POISON)
    with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_UNSUPPORTED"):
        ctx.correct_blocks(12, 6, 2048, blk.pitch, 2, blk.src, blk.par, blk.rep, coef=bad, t=2)
    with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_ARG"):
        ctx.correct_blocks(12, 6, 2048, blk.pitch, 2, blk.src, blk.par, blk.rep[1:], coef=blk.coef, t=2)
    h, lib = ctx._h, rsgpu.lib()
    s, p, r = blk.src.data_ptr(), blk.par.data_ptr(), blk.rep.data_ptr()
    for src, par, rep in ((None, p, r), (s, None, r), (s, p, None)):
        assert lib.rsgpu_correct_blocks(h, 12, 6, 2048, blk.pitch, 2, src, par, blk.c.ctypes.data, 2, rep) == -1
    torch.cuda.synchronize()
    assert (blk.rep.cpu().numpy() == gf.POISON).all() and blk.equals(damaged)
    for k, e, t in ((12, 4, 2), (12, 2, 1)):
        four = Blocks(ctx, k, e, "cauchy", 2048, "eq", B=2)
        four.hit(1, [(3, 0x44)], 99)
        damaged = four.snapshot()
        with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_UNSUPPORTED"):
            four.correct(t)
        torch.cuda.synchronize()
        assert (four.rep.cpu().numpy() == gf.POISON).all() and four.equals(damaged)
    # e = 4 is enough for t = 1
    four = Blocks(ctx, 12, 4, "cauchy", 2048, "eq", B=2)
    four.hit(1, [(3, 0x44)], 99)
    run(four, 1, [CLEAN, (1, 1, 0, cm.REPAIRED, 3)], four.pristine)


def test_nothing_to_check_is_clean(ctx):
    """len == 0 and e == 0: every block CLEAN, whatever the report held."""
    for k, e, L in ((6, 5, 0), (6, 0, 64)):
        blk = Blocks.__new__(Blocks)
        gf.DeviceBlocks.__init__(blk, ctx, k, e, L, 3, max(L, 16), 0, "rs", encode=False)
        blk.rep = torch.empty(3 * DT.itemsize, dtype=torch.uint8, device=blk.dev)
        torch.cuda.synchronize()
        before = blk.snapshot()
        for t in (1, 2):
            gf.same(blk.correct(t), [CLEAN] * 3, FIELDS)
            assert blk.equals(before)


def test_encoder_correct(ctx):
    enc = rsgpu.GpuEncoder(20, 4096, 7, blocks=2, seed=4, ctx=ctx)
    enc.encode_all()
    torch.cuda.synchronize()
    src0, par0 = enc.src.clone(), enc.par.clone()
    rep = enc.correct()
    assert rep.dtype == DT and len(rep) == 2
    gf.same(rep, [CLEAN, CLEAN], FIELDS)
    enc.src.view(2, 20, enc.pitch)[1, 5, 77] ^= 0x10
    enc.par.view(2, 7, enc.pitch)[1, 6, 77] ^= 0x01
    enc.src.view(2, 20, enc.pitch)[1, 9, 4095] ^= 0xFF
    gf.same(enc.correct(t=1), [CLEAN, (2, 1, 0, cm.PARTIAL, 9)], FIELDS)
    gf.same(enc.correct(), [CLEAN, (1, 1, 1, cm.REPAIRED, -1)], FIELDS)
    assert torch.equal(enc.src, src0) and torch.equal(enc.par, par0)
