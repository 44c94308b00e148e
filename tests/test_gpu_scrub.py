"""Parity scrub on the GPU (include/rsgpu.h rsgpu_scrub_blocks) under every
scrub kernel choice: data from fill_synthetic, parity from encode_blocks, rows
then damaged with torch indexing, and every report compared field by field
with the numpy model of the contract (tests/scrub_model.py).

The model's syndromes of undamaged blocks are zero (checked once per code on
a block read back from the device, model_clean); the expected syndromes of a
damaged block follow from them by linearity (scrub_model.damage, itself
checked against the full model in tests/test_scrub.py), and the expected
report is the model's brute force over rows on those syndromes."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import gpu_family as gf  # noqa: E402
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402

KERNELS = ["auto", "fused", "two_pass"]
FUSED_NAME = "k_rs_bs_scrub"
# the compiled codes: (k, e) -> Horner chunk C (rs_bitsliced.hip's plans)
COMPILED = {(16, 4): 16, (16, 8): 16, (64, 32): 16, (64, 16): 16, (100, 20): 20, (5, 4): 5, (20, 7): 20}
# every code of the clean test: the compiled ones, a Cauchy matrix, wide and tall RS
CODES = [(k, e, "rs") for k, e in COMPILED] + [(24, 12, "cauchy"), (9, 40, "rs"), (213, 37, "rs")]
DT = rsgpu.SCRUB_REPORT_DTYPE


@pytest.fixture(scope="module")
def ctx():
    yield from gf.device_context(reset_scrub_kernel=True)


same = gf.same


class Blocks(gf.DeviceBlocks):
    """B synthetic blocks and their parity on the device; scrub() returns the
    reports as a structured array."""

    def __init__(self, ctx, k, e, L, B, kind="rs", pitch=None, offset=0, seed=11):
        super().__init__(ctx, k, e, L, B, pitch or (L + 255) // 256 * 256, offset, kind, seed=seed)
        self.rep = torch.empty(B * DT.itemsize, dtype=torch.uint8, device=self.dev)

    def scrub(self, kernel="auto", locate=True, poison=0xA5, coef="own"):
        self.ctx.set_scrub_kernel(kernel)
        self.rep.fill_(poison)
        try:
            self.ctx.scrub_blocks(self.k, self.e, self.L, self.pitch, self.B, self.src, self.par, self.rep,
                                  coef=self.coef if isinstance(coef, str) else coef, locate=locate)
        finally:
            self.ctx.set_scrub_kernel("auto")
        torch.cuda.synchronize()
        return self.rep.cpu().numpy().view(DT)


CLEAN = (0, sm.CLEAN, -1)


@pytest.fixture(scope="module")
def model_clean(ctx):
    """Once per compiled code: the full model on one undamaged block read back
    from the device (L = 4160) gives zero syndromes and CLEAN."""
    done = {}

    def check(k, e):
        if (k, e) not in done:
            blk = Blocks(ctx, k, e, 4160, 2)
            s, p = blk.host_block(1)
            syn = sm.syndromes(blk.c, s, p)
            assert not syn.any()
            assert sm.report(blk.c, syn) == CLEAN
            done[(k, e)] = True
        return np.zeros((e, 4160), np.uint8)

    return check


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k,e,kind", CODES, ids=str)
def test_clean_blocks(ctx, kernel, k, e, kind):
    for L in (32, 96, 2048, 2080, 4160):
        for B in (1, 3):
            rep = Blocks(ctx, k, e, L, B, kind).scrub(kernel)
            same(rep, [CLEAN] * B)


def damaged_rows(k, e):
    C, opw = COMPILED[(k, e)], rsgpu_rows_per_wave(k, e)
    rows = [0, C - 1, C, k - 1, k, k + opw - 1, k + opw, k + e - 1]
    return sorted({r for r in rows if 0 <= r < k + e})


def rsgpu_rows_per_wave(k, e):
    """(E + NW - 1) / NW of the compiled plans (rs_bitsliced_rows_per_wave)."""
    nw = 4 if (k, e) in ((64, 32), (100, 20)) else 2 if (k, e) == (64, 16) else 1
    return (e + nw - 1) // nw


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k,e", list(COMPILED), ids=str)
def test_one_damaged_row(ctx, model_clean, kernel, k, e):
    """B = 3 per case, only the middle block damaged: every (byte position,
    XOR value) pair is one such triple of a single call per damaged row."""
    L = 4160
    cases = [(pos, x) for pos in (0, 31, 32, 2047, 2048, L - 1) for x in (0x01, 0x80, 0xFF)]
    blk = Blocks(ctx, k, e, L, 3 * len(cases))
    zero = model_clean(k, e)
    for row in damaged_rows(k, e):
        want = []
        for i, (pos, x) in enumerate(cases):
            blk.xor(3 * i + 1, row, pos, x)
            want += [CLEAN, sm.report(blk.c, sm.damage(blk.c, zero, row, [pos], [x])), CLEAN]
            assert want[-2] == (1, sm.ONE_ROW, row)  # what the contract says outright
        rep = blk.scrub(kernel)
        for i, (pos, x) in enumerate(cases):
            blk.xor(3 * i + 1, row, pos, x)
        same(rep, want)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k,e", list(COMPILED), ids=str)
def test_idle_lanes_are_not_counted(ctx, kernel, k, e):
    """L = 2080: the second tile has one busy lane, the others re-read the row
    head.  Damage at byte 0 is one bad column, not 64."""
    blk = Blocks(ctx, k, e, 2080, 3)
    for row in (0, k):
        blk.xor(1, row, 0, 0x5C)
        rep = blk.scrub(kernel)
        blk.xor(1, row, 0, 0x5C)
        assert int(rep[1]["bad_columns"]) == 1
        same(rep, [CLEAN, (1, sm.ONE_ROW, row), CLEAN])


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k,e", list(COMPILED), ids=str)
def test_two_damaged_rows(ctx, model_clean, kernel, k, e):
    L = 4160
    zero = model_clean(k, e)
    blk = Blocks(ctx, k, e, L, 4)
    c = blk.c
    # block 0: two rows in different tiles; block 1: the same row in both
    # tiles; block 2: two rows in the same column (e >= 3: distance >= 4, two
    # errors cannot look like one -- derived, not measured); block 3: a source
    # and a parity row in one column
    hits = [(0, 2, 5, 0x21), (0, k - 1, 3000, 0x9D),
            (1, k + 1, 5, 0x21), (1, k + 1, 3000, 0x9D),
            (2, 1, 100, 0x17), (2, 3, 100, 0xE0),
            (3, 0, 2050, 0x01), (3, k + e - 1, 2050, 0x01)]
    syn = [zero.copy() for _ in range(4)]
    for b, row, col, x in hits:
        blk.xor(b, row, col, x)
        syn[b] = sm.damage(c, syn[b], row, [col], [x])
    want = [sm.report(c, s) for s in syn]
    assert want[0] == (2, sm.DAMAGED, -1) and want[1] == (2, sm.ONE_ROW, k + 1)
    assert want[2] == (1, sm.DAMAGED, -1) and want[3] == (1, sm.DAMAGED, -1)
    same(blk.scrub(kernel), want)


@pytest.mark.parametrize("kernel", KERNELS)
def test_flags(ctx, kernel):
    blk = Blocks(ctx, 16, 4, 2048, 3)
    blk.xor(1, 7, 99, 0x44)
    same(blk.scrub(kernel, locate=False), [CLEAN, (1, sm.DAMAGED, -1), CLEAN])
    same(blk.scrub(kernel, locate=True), [CLEAN, (1, sm.ONE_ROW, 7), CLEAN])
    # LOCATE needs a locatable matrix: nothing runs, the report keeps its poison
    bad = sm.rs_matrix(16, 4).copy()
    bad[0, 3] = 0
    with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_UNSUPPORTED"):
        blk.scrub(kernel, coef=bad)
    torch.cuda.synchronize()
    assert (blk.rep.cpu().numpy() == 0xA5).all()
    one = Blocks(ctx, 16, 1, 2048, 2)
    with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_UNSUPPORTED"):
        one.scrub(kernel)
    torch.cuda.synchronize()
    assert (one.rep.cpu().numpy() == 0xA5).all()
    one.xor(0, 16, 5, 1)
    same(one.scrub(kernel, locate=False), [(1, sm.DAMAGED, -1), CLEAN])


@pytest.mark.parametrize("kernel", KERNELS)
def test_caller_matrix_and_wide_codes(ctx, kernel):
    """The two-pass path with a Cauchy matrix and with more parity than
    source rows: a source and a parity row each."""
    for k, e, kind in ((24, 12, "cauchy"), (9, 40, "rs")):
        blk = Blocks(ctx, k, e, 2080, 3, kind)
        zero = np.zeros((e, 2080), np.uint8)
        for row in (0, k - 1, k, k + e - 1):
            blk.xor(1, row, 2079, 0xC3)
            blk.xor(1, row, 17, 0x01)
            want = sm.report(blk.c, sm.damage(blk.c, zero, row, [2079, 17], [0xC3, 0x01]))
            assert want == (2, sm.ONE_ROW, row)
            rep = blk.scrub(kernel)
            blk.xor(1, row, 2079, 0xC3)
            blk.xor(1, row, 17, 0x01)
            same(rep, [CLEAN, want, CLEAN])


@pytest.mark.parametrize("kernel", KERNELS)
def test_unaligned_rows_run_two_pass(ctx, kernel):
    blk = Blocks(ctx, 16, 4, 1000, 3, pitch=1000, offset=1)
    assert blk.src.data_ptr() % 16 == 1
    blk.xor(1, 9, 999, 0x80)
    ctx.timing_enable(True)
    try:
        rep = blk.scrub(kernel)
        names = [n for n, _, _ in ctx.timing_read()]
    finally:
        ctx.timing_enable(False)
    same(rep, [CLEAN, (1, sm.ONE_ROW, 9), CLEAN])
    assert FUSED_NAME not in names and "k_scrub_compare" in names


@pytest.mark.parametrize("kernel", KERNELS)
def test_aligned_rows_with_a_tail(ctx, kernel):
    """L = 1001 at pitch 1008, 16-byte aligned: the two-pass compare walks 992
    bytes 16 at a time and the last 9 one by one; damage on both sides of that
    seam and in the middle of a 16-byte group."""
    blk = Blocks(ctx, 16, 4, 1001, 3, pitch=1008)
    zero = np.zeros((4, 1001), np.uint8)
    cols, xors = [0, 7, 991, 992, 1000], [0x01, 0xFF, 0x80, 0x33, 0x02]
    for row in (3, 17):
        for col, x in zip(cols, xors):
            blk.xor(1, row, col, x)
        want = sm.report(blk.c, sm.damage(blk.c, zero, row, cols, xors))
        assert want == (5, sm.ONE_ROW, row)
        rep = blk.scrub(kernel)
        for col, x in zip(cols, xors):
            blk.xor(1, row, col, x)
        same(rep, [CLEAN, want, CLEAN])


@pytest.mark.parametrize("kernel", KERNELS)
def test_more_blocks_than_a_grid_holds(ctx, kernel):
    B = 65536 + 3
    blk = Blocks(ctx, 5, 4, 32, B, pitch=32)
    blk.xor(65537, 6, 31, 0xFF)
    rep = blk.scrub(kernel)
    assert int(rep["bad_columns"].sum()) == 1 and int((rep["status"] != sm.CLEAN).sum()) == 1
    assert (rep["row"][rep["status"] == sm.CLEAN] == -1).all()
    assert tuple(int(v) for v in rep[65537]) == (1, sm.ONE_ROW, 6)


def test_slices(ctx):
    """(2, 8) with 1 MiB rows through the two-pass path: 8 MiB of parity per
    block, so the 128 MiB scratch holds 16 blocks and 17 blocks run as two
    slices; one damaged row in the last block of the first slice, another in
    the only block of the second.  The model runs on the damaged columns and a
    few others (the full rows are consistent by construction: encode_blocks,
    tested on its own)."""
    k, e, L, B = 2, 8, 1 << 20, 17
    assert rsgpu.scrub_locatable(k, e)
    blk = Blocks(ctx, k, e, L, B, pitch=L)
    for b, row, col, x in [(15, 1, 0, 0x10), (15, 1, L - 1, 0xEE), (16, k + 3, 12345, 0x02), (16, k + 3, 777, 0x03)]:
        blk.xor(b, row, col, x)
    cols = torch.tensor([0, 1, 777, 12345, L - 2, L - 1], device=blk.src.device)
    hs = blk.src.view(B, k, L)[:, :, cols].cpu().numpy()
    hp = blk.par.view(B, e, L)[:, :, cols].cpu().numpy()
    for locate in (True, False):
        want = [sm.scrub(blk.c, hs[b], hp[b], locate) for b in range(B)]
        assert want[:15] == [CLEAN] * 15
        assert want[15:] == ([(2, sm.ONE_ROW, 1), (2, sm.ONE_ROW, k + 3)] if locate else [(2, sm.DAMAGED, -1)] * 2)
        ctx.timing_enable(True)
        try:
            rep = blk.scrub("two_pass", locate=locate)
            slices = [nb for n, _, nb in ctx.timing_read() if n == "k_scrub_compare"]
        finally:
            ctx.timing_enable(False)
        same(rep, want)
        assert slices == [16, 1]


def test_path_check(ctx):
    blk = Blocks(ctx, 64, 32, 4096, 2)
    seen = {}
    ctx.timing_enable(True)
    try:
        for kernel in KERNELS:
            same(blk.scrub(kernel), [CLEAN, CLEAN])
            seen[kernel] = [n for n, _, _ in ctx.timing_read()]
    finally:
        ctx.timing_enable(False)
    assert FUSED_NAME in seen["auto"] and FUSED_NAME in seen["fused"]
    assert FUSED_NAME not in seen["two_pass"] and "k_scrub_compare" in seen["two_pass"]
    assert "k_scrub_compare" not in seen["auto"]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("which", ["data", "parity"])
def test_repair_round_trip(ctx, kernel, which):
    """Scrub, decode_general with the reported row as the one erasure, write
    the row back: the original bytes, and a second scrub into the same report
    buffer (now holding ONE_ROW) says CLEAN."""
    k, e, L = 16, 4, 4160
    blk = Blocks(ctx, k, e, L, 3)
    row = 5 if which == "data" else k + 2
    orig = blk.rows(row)[1].clone()
    blk.rows(row)[1, 1000:1100] ^= 0x3C
    blk.rows(row)[1, 4159] ^= 0x01
    rep = blk.scrub(kernel)
    same(rep, [CLEAN, (101, sm.ONE_ROW, row), CLEAN])
    got = int(rep[1]["row"])
    dev = blk.src.device
    d_err = torch.tensor([got], dtype=torch.uint8, device=dev)
    out = torch.zeros(blk.pitch, dtype=torch.uint8, device=dev)
    ws = torch.empty(rsgpu.decode_general_workspace_bytes(k, k + e, 1, 1), dtype=torch.uint8, device=dev)
    status = torch.full((1,), 7, dtype=torch.int32, device=dev)
    ctx.decode_general(k, k + e, L, blk.pitch, 1, None, blk.src[1 * k * blk.pitch:],
                       blk.par[1 * e * blk.pitch:], d_err, 1, out, ws, status)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert torch.equal(out[:L], orig)
    blk.rows(row)[1] = out[:L]
    ctx.set_scrub_kernel(kernel)
    try:
        # no poison this time: the buffer still holds the first call's reports
        ctx.scrub_blocks(k, e, L, blk.pitch, 3, blk.src, blk.par, blk.rep)
    finally:
        ctx.set_scrub_kernel("auto")
    torch.cuda.synchronize()
    same(blk.rep.cpu().numpy().view(DT), [CLEAN] * 3)


def test_encoder_scrub(ctx):
    enc = rsgpu.GpuEncoder(20, 4096, 7, blocks=2, seed=4, ctx=ctx)
    enc.encode_all()
    rep = enc.scrub()
    assert rep.dtype == DT and len(rep) == 2
    same(rep, [CLEAN, CLEAN])
    enc.par.view(2, 7, enc.pitch)[1, 3, 77] ^= 0x10
    same(enc.scrub(), [CLEAN, (1, sm.ONE_ROW, 23)])
    same(enc.scrub(locate=False), [CLEAN, (1, sm.DAMAGED, -1)])
