"""In-place repair on the GPU (include/rsgpu.h rsgpu_repair_blocks) under
every scrub kernel choice and both modes: data from fill_synthetic, parity
from encode_blocks, rows then damaged with torch indexing.

Every case keeps a clone of the whole source and parity allocations (padding
included) from before the damage and one of the damaged state.  What the call
must do comes from the numpy model of the contract (tests/repair_model.py) run
on each damaged block as read back from the device: its verdict is asserted
first, then the device's reports are compared with it field by field, and the
whole allocations with the damaged state patched by the model's rows -- so a
byte written anywhere it should not be (another row, another block, the
padding) fails the comparison."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import gpu_family as gf  # noqa: E402
import repair_model as rm  # noqa: E402
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402

KERNELS = ["auto", "fused", "two_pass"]
MODES = ["one_row", "columns"]
FUSED_NAME = "k_rs_bs_repair"
# the compiled codes (rs_bitsliced.hip's plans)
COMPILED = [(16, 4), (16, 8), (64, 32), (64, 16), (100, 20), (5, 4), (20, 7)]
CODES = [(k, e, "rs") for k, e in COMPILED] + [(24, 12, "cauchy"), (9, 40, "rs"), (213, 37, "rs")]
DT = rsgpu.REPAIR_REPORT_DTYPE
CLEAN = (0, 0, rm.CLEAN, -1)
# two full 2 KB tiles and a 64-byte tail tile with 62 idle lanes
L0 = 4160
_OWN = object()  # Blocks.repair: the matrix the blocks were encoded with


@pytest.fixture(scope="module")
def ctx():
    yield from gf.device_context(reset_scrub_kernel=True)


class Blocks(gf.DeviceBlocks):
    """B synthetic blocks and their parity on the device."""

    def __init__(self, ctx, k, e, L, B, kind="rs", pitch=None, offset=0, seed=11):
        super().__init__(ctx, k, e, L, B, pitch or (L + 255) // 256 * 256, offset, kind, seed=seed)
        self.rep = torch.empty(B * DT.itemsize, dtype=torch.uint8, device=self.dev)
        self.srep = torch.empty(B * rsgpu.SCRUB_REPORT_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        torch.cuda.synchronize()
        self.pristine = self.snapshot()

    def equals(self, snap):
        return torch.equal(self.src_all, snap[0]) and torch.equal(self.par_all, snap[1])

    def model(self, mode, damaged):
        """The model on the blocks `damaged` as they are now: ([verdict per
        block of the batch], the allocations as the call must leave them)."""
        want = [CLEAN] * self.B
        src, par = self.snapshot()
        sv = self.view(src[self.offset:], self.k)
        pv = self.view(par[self.offset:], self.e)
        for b in damaged:
            s, p = self.host_block(b)
            s2, p2, want[b] = rm.repair(self.c, s, p, mode)
            sv[b, :, : self.L] = torch.from_numpy(s2).to(sv.device)
            pv[b, :, : self.L] = torch.from_numpy(p2).to(pv.device)
        return want, (src, par)

    def repair(self, kernel, mode, poison=0xA5, coef=_OWN):
        self.ctx.set_scrub_kernel(kernel)
        if poison is not None:
            self.rep.fill_(poison)
        try:
            self.ctx.repair_blocks(self.k, self.e, self.L, self.pitch, self.B, self.src, self.par, self.rep,
                                   coef=self.coef if coef is _OWN else coef, mode=mode)
        finally:
            self.ctx.set_scrub_kernel("auto")
        torch.cuda.synchronize()
        return self.rep.cpu().numpy().view(DT)

    def scrub_is_clean(self, kernel):
        self.ctx.set_scrub_kernel(kernel)
        try:
            self.ctx.scrub_blocks(self.k, self.e, self.L, self.pitch, self.B, self.src, self.par, self.srep,
                                  coef=self.coef)
        finally:
            self.ctx.set_scrub_kernel("auto")
        torch.cuda.synchronize()
        r = self.srep.cpu().numpy().view(rsgpu.SCRUB_REPORT_DTYPE)
        return (r["status"] == sm.CLEAN).all() and (r["bad_columns"] == 0).all() and (r["row"] == -1).all()


def same(rep, want):
    """rep: structured reports; want: [(bad, repaired, status, row)] from the model."""
    gf.same(rep, want, gf.REPAIR_FIELDS)


def run(blk, kernel, mode, want, after):
    same(blk.repair(kernel, mode), want)
    assert torch.equal(blk.src_all, after[0]), "source allocation"
    assert torch.equal(blk.par_all, after[1]), "parity allocation"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k,e,kind", CODES, ids=str)
def test_clean_blocks(ctx, kernel, mode, k, e, kind):
    blk = Blocks(ctx, k, e, L0, 3, kind)
    s, p = blk.host_block(1)
    assert rm.repair(blk.c, s, p, mode)[2] == CLEAN
    run(blk, kernel, mode, [CLEAN] * 3, blk.pristine)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k,e", COMPILED, ids=str)
def test_one_damaged_row(ctx, kernel, mode, k, e):
    """The tiles' first and last bytes, the tail tile's, and one byte in each
    of the four 8-byte groups of lane 5's 32 bytes (160 ..  191)."""
    blk = Blocks(ctx, k, e, L0, 3)
    cols = [0, 2047, 2048, 4095, 4096, 4159, 163, 169, 182, 191]
    xors = [0x01, 0x80, 0xFF, 0x5C, 0x02, 0xC3, 0x10, 0x7E, 0x99, 0x44]
    for row in (0, k - 1, k, k + e - 1):
        for col, x in zip(cols, xors):
            blk.xor(1, row, col, x)
        assert not blk.equals(blk.pristine)
        want, after = blk.model(mode, [1])
        assert want == [CLEAN, (10, 10, rm.REPAIRED, row), CLEAN]
        assert torch.equal(after[0], blk.pristine[0]) and torch.equal(after[1], blk.pristine[1])
        run(blk, kernel, mode, want, blk.pristine)
        assert blk.scrub_is_clean(kernel)
        # a second repair, into the report buffer that still says REPAIRED
        same(blk.repair(kernel, mode, poison=None), [CLEAN] * 3)
        assert blk.equals(blk.pristine)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k,e", COMPILED, ids=str)
def test_two_rows_in_different_columns(ctx, kernel, mode, k, e):
    """Block 0: two rows, one column each, in different tiles; block 2: the
    same row in both tiles; blocks 1 and 3 clean."""
    blk = Blocks(ctx, k, e, L0, 4)
    for b, row, col, x in [(0, 2, 5, 0x21), (0, k + e - 1, 3000, 0x9D), (2, k + 1, 5, 0x21), (2, k + 1, 3000, 0x9D)]:
        blk.xor(b, row, col, x)
    damaged = blk.snapshot()
    want, after = blk.model(mode, [0, 2])
    assert want[2] == (2, 2, rm.REPAIRED, k + 1)
    if mode == "one_row":
        assert want[0] == (2, 0, rm.DAMAGED, -1)
        b0 = slice(0, k * blk.pitch), slice(0, e * blk.pitch)
        assert torch.equal(after[0][b0[0]], damaged[0][b0[0]]) and torch.equal(after[1][b0[1]], damaged[1][b0[1]])
    else:
        assert want[0] == (2, 2, rm.REPAIRED, -1)
        assert torch.equal(after[0], blk.pristine[0]) and torch.equal(after[1], blk.pristine[1])
    run(blk, kernel, mode, want, after)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k,e", COMPILED, ids=str)
def test_two_rows_in_one_column(ctx, kernel, mode, k, e):
    """Block 1: rows 1 and 3 damaged in column 100 (e >= 3: distance >= 4, no
    single row explains two errors) and row k - 1 in column 2500."""
    blk = Blocks(ctx, k, e, L0, 3)
    blk.xor(1, 1, 100, 0x17)
    blk.xor(1, 3, 100, 0xE0)
    blk.xor(1, k - 1, 2500, 0x3A)
    damaged = blk.snapshot()
    want, after = blk.model(mode, [1])
    if mode == "one_row":
        assert want == [CLEAN, (2, 0, rm.DAMAGED, -1), CLEAN]
        assert torch.equal(after[0], damaged[0]) and torch.equal(after[1], damaged[1])
    else:
        assert want == [CLEAN, (2, 1, rm.PARTIAL, k - 1), CLEAN]
        diff = torch.nonzero(after[0] != damaged[0]).flatten().tolist()
        assert diff == [(1 * k + k - 1) * blk.pitch + 2500] and torch.equal(after[1], damaged[1])
        assert after[0][diff[0]] == blk.pristine[0][diff[0]]
    run(blk, kernel, mode, want, after)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k,e", COMPILED, ids=str)
def test_source_and_parity_row_in_one_column(ctx, kernel, mode, k, e):
    blk = Blocks(ctx, k, e, L0, 3)
    blk.xor(1, 0, 2050, 0x01)
    blk.xor(1, k + e - 1, 2050, 0x01)
    damaged = blk.snapshot()
    want, after = blk.model(mode, [1])
    # the model's verdict: two errors in one column of a distance >= 5 code
    assert want == [CLEAN, (1, 0, rm.DAMAGED, -1), CLEAN]
    assert torch.equal(after[0], damaged[0]) and torch.equal(after[1], damaged[1])
    run(blk, kernel, mode, want, after)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_caller_matrix_and_wide_codes(ctx, kernel, mode):
    """The two-pass path with a Cauchy matrix and with more parity than
    source rows: a source and a parity row each, at the last column."""
    for k, e, kind in ((24, 12, "cauchy"), (9, 40, "rs")):
        blk = Blocks(ctx, k, e, L0, 3, kind)
        for row in (0, k - 1, k, k + e - 1):
            blk.xor(1, row, L0 - 1, 0xC3)
            blk.xor(1, row, 17, 0x01)
            want, after = blk.model(mode, [1])
            assert want == [CLEAN, (2, 2, rm.REPAIRED, row), CLEAN]
            ctx.timing_enable(True)
            try:
                run(blk, kernel, mode, want, blk.pristine)
                names = [n for n, _, _ in ctx.timing_read()]
            finally:
                ctx.timing_enable(False)
            assert FUSED_NAME not in names and "k_repair_compare" in names
            assert blk.scrub_is_clean(kernel)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shape", ["unaligned", "tailed"])
def test_unaligned_and_tailed_rows_run_two_pass(ctx, kernel, mode, shape):
    """unaligned: every row starts 1 past a 16-byte boundary.  tailed: L =
    1001 at pitch 1008, the compare walks 992 bytes 16 at a time and the last
    9 one by one; damage on both sides of that seam."""
    if shape == "unaligned":
        blk = Blocks(ctx, 16, 4, 1000, 3, pitch=1000, offset=1)
        assert blk.src.data_ptr() % 16 == 1 and blk.par.data_ptr() % 16 == 1
        cols, xors = [0, 500, 999], [0x80, 0x11, 0xFE]
    else:
        blk = Blocks(ctx, 16, 4, 1001, 3, pitch=1008)
        cols, xors = [0, 7, 991, 992, 1000], [0x01, 0xFF, 0x80, 0x33, 0x02]
    for row in (3, 15, 16, 19):
        for col, x in zip(cols, xors):
            blk.xor(1, row, col, x)
        want, after = blk.model(mode, [1])
        assert want == [CLEAN, (len(cols), len(cols), rm.REPAIRED, row), CLEAN]
        ctx.timing_enable(True)
        try:
            run(blk, kernel, mode, want, blk.pristine)
            names = [n for n, _, _ in ctx.timing_read()]
        finally:
            ctx.timing_enable(False)
        assert FUSED_NAME not in names and FUSED_NAME + "_gated" not in names
        assert "k_repair_compare" in names


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_more_blocks_than_a_grid_holds(ctx, kernel, mode):
    B = 65536 + 3
    blk = Blocks(ctx, 5, 4, 32, B, pitch=32)
    blk.xor(65537, 6, 31, 0xFF)
    blk.xor(65537, 6, 0, 0x01)
    want, after = blk.model(mode, [65537])
    assert want[65537] == (2, 2, rm.REPAIRED, 6)
    rep = blk.repair(kernel, mode)
    assert int((rep["status"] != rm.CLEAN).sum()) == 1 and int(rep["bad_columns"].sum()) == 2
    assert int(rep["repaired_columns"].sum()) == 2
    assert (rep["row"][rep["status"] == rm.CLEAN] == -1).all()
    assert tuple(int(v) for v in rep[65537]) == want[65537]
    assert blk.equals(blk.pristine)
    assert blk.scrub_is_clean(kernel)


@pytest.mark.parametrize("mode", MODES)
def test_slices(ctx, mode):
    """(2, 8) with 1 MiB rows through the two-pass path: 8 MiB of parity per
    block, so the 128 MiB scratch holds 16 blocks and 17 blocks run as two
    slices; one damaged row in the last block of the first slice, another in
    the only block of the second.  The model runs on the damaged columns and a
    few others (the full rows are consistent by construction: encode_blocks,
    tested on its own); the rows come back as they were before the damage."""
    k, e, L, B = 2, 8, 1 << 20, 17
    assert rsgpu.scrub_locatable(k, e)
    blk = Blocks(ctx, k, e, L, B, pitch=L)
    for b, row, col, x in [(15, 1, 0, 0x10), (15, 1, L - 1, 0xEE), (16, k + 3, 12345, 0x02), (16, k + 3, 777, 0x03)]:
        blk.xor(b, row, col, x)
    assert not blk.equals(blk.pristine)
    cols = torch.tensor([0, 1, 777, 12345, L - 2, L - 1], device=blk.src.device)
    hs = blk.src.view(B, k, L)[:, :, cols].cpu().numpy()
    hp = blk.par.view(B, e, L)[:, :, cols].cpu().numpy()
    fixed = [rm.repair(blk.c, hs[b], hp[b], mode) for b in range(B)]
    want = [f[2] for f in fixed]
    assert want == [CLEAN] * 15 + [(2, 2, rm.REPAIRED, 1), (2, 2, rm.REPAIRED, k + 3)]
    # the model's rows are the undamaged ones
    ps = blk.pristine[0].view(B, k, L)[:, :, cols].cpu().numpy()
    pp = blk.pristine[1].view(B, e, L)[:, :, cols].cpu().numpy()
    assert all((f[0] == ps[b]).all() and (f[1] == pp[b]).all() for b, f in enumerate(fixed))
    ctx.timing_enable(True)
    try:
        run(blk, "two_pass", mode, want, blk.pristine)
        slices = [(n, nb) for n, _, nb in ctx.timing_read() if n.startswith("k_repair_compare")]
    finally:
        ctx.timing_enable(False)
    if mode == "one_row":
        assert slices == [("k_repair_compare", 16), ("k_repair_compare_gated", 16),
                          ("k_repair_compare", 1), ("k_repair_compare_gated", 1)]
    else:
        assert slices == [("k_repair_compare", 16), ("k_repair_compare", 1)]
    assert blk.scrub_is_clean("two_pass")


@pytest.mark.parametrize("kernel", KERNELS)
def test_refusals(ctx, kernel):
    """RSGPU_ERR_UNSUPPORTED: nothing runs, the report keeps its poison and
    the rows their damage."""
    blk = Blocks(ctx, 16, 4, 2048, 3)
    blk.xor(1, 7, 99, 0x44)
    damaged = blk.snapshot()
    bad = sm.rs_matrix(16, 4).copy()
    bad[0, 3] = 0
    for mode in MODES:
        with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_UNSUPPORTED"):
            blk.repair(kernel, mode, coef=bad)
        torch.cuda.synchronize()
        assert (blk.rep.cpu().numpy() == 0xA5).all() and blk.equals(damaged)
    one = Blocks(ctx, 16, 1, 2048, 2)
    one.xor(0, 16, 5, 1)
    damaged = one.snapshot()
    for mode in MODES:
        with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_UNSUPPORTED"):
            one.repair(kernel, mode)
        torch.cuda.synchronize()
        assert (one.rep.cpu().numpy() == 0xA5).all() and one.equals(damaged)
    two = Blocks(ctx, 16, 2, 2048, 2)
    two.xor(0, 3, 5, 1)
    damaged = two.snapshot()
    with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_UNSUPPORTED"):
        two.repair(kernel, "columns")
    torch.cuda.synchronize()
    assert (two.rep.cpu().numpy() == 0xA5).all() and two.equals(damaged)
    # e = 2 is enough for ONE_ROW mode
    want, after = two.model("one_row", [0])
    assert want == [(1, 1, rm.REPAIRED, 3), CLEAN]
    run(two, kernel, "one_row", want, two.pristine)
    with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_ARG"):
        ctx.repair_blocks(16, 4, 2048, 2048, 3, blk.src, blk.par, blk.rep[1:])  # misaligned report
    # null rows, a null report, an unknown mode: argument errors, nothing runs
    blk.rep.fill_(0xA5)
    damaged = blk.snapshot()
    h, L = ctx._h, rsgpu.lib()
    s, p, r = blk.src.data_ptr(), blk.par.data_ptr(), blk.rep.data_ptr()
    for src, par, rep, mode in ((None, p, r, 0), (s, None, r, 0), (s, p, None, 0), (s, p, r, 2), (s, p, r, -1)):
        assert L.rsgpu_repair_blocks(h, 16, 4, 2048, 2048, 3, src, par, None, mode, rep) == -1
    torch.cuda.synchronize()
    assert (blk.rep.cpu().numpy() == 0xA5).all() and blk.equals(damaged)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_report_is_overwritten_not_accumulated(ctx, kernel, mode):
    blk = Blocks(ctx, 16, 4, L0, 3)
    blk.xor(1, 7, 99, 0x44)
    blk.xor(1, 7, 4100, 0x45)
    same(blk.repair(kernel, mode), [CLEAN, (2, 2, rm.REPAIRED, 7), CLEAN])
    # other damage, the buffer still holding the first call's reports
    blk.xor(0, 18, 99, 0x44)
    want, after = blk.model(mode, [0])
    assert want == [(1, 1, rm.REPAIRED, 18), CLEAN, CLEAN]
    same(blk.repair(kernel, mode, poison=None), want)
    assert blk.equals(blk.pristine)


def test_path_check(ctx):
    blk = Blocks(ctx, 64, 32, 4096, 2)
    for mode in MODES:
        seen = {}
        ctx.timing_enable(True)
        try:
            for kernel in KERNELS:
                same(blk.repair(kernel, mode), [CLEAN, CLEAN])
                seen[kernel] = [n for n, _, _ in ctx.timing_read()]
        finally:
            ctx.timing_enable(False)
        assert FUSED_NAME in seen["auto"] and FUSED_NAME in seen["fused"]
        assert FUSED_NAME not in seen["two_pass"] and "k_repair_compare" in seen["two_pass"]
        assert "k_repair_compare" not in seen["auto"]
        gated = [FUSED_NAME + "_gated" in seen[kn] for kn in ("auto", "fused")]
        assert gated == [mode == "one_row"] * 2
        assert all("k_repair_finalise" in names for names in seen.values())
    assert blk.equals(blk.pristine)


@pytest.mark.parametrize("which", ["data", "parity"])
def test_encoder_repair(ctx, which):
    enc = rsgpu.GpuEncoder(20, 4096, 7, blocks=2, seed=4, ctx=ctx)
    enc.encode_all()
    torch.cuda.synchronize()
    src0, par0 = enc.src.clone(), enc.par.clone()
    rep = enc.repair()
    assert rep.dtype == DT and len(rep) == 2
    same(rep, [CLEAN, CLEAN])
    row = 5 if which == "data" else 23
    rows = enc.src.view(2, 20, enc.pitch) if which == "data" else enc.par.view(2, 7, enc.pitch)
    rows[1, row % 20, 77] ^= 0x10
    rows[1, row % 20, 4095] ^= 0xFF
    assert not (torch.equal(enc.src, src0) and torch.equal(enc.par, par0))
    same(enc.repair(), [CLEAN, (2, 2, rm.REPAIRED, row)])
    assert torch.equal(enc.src, src0) and torch.equal(enc.par, par0)
    same(enc.repair(mode="columns"), [CLEAN, CLEAN])
    assert (enc.scrub()["status"] == sm.CLEAN).all()
