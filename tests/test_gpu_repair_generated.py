"""The generated repair on the GPU (include/rsgpu.h rsgpu_set_repair_kernel
RSGPU_REPAIR_KERNEL_GENERATED; k_rs_jit_repair, k_rs_jitw_repair): for every
layout of the generated kernels and the lengths at which a tile, a lane or a
workgroup is partly or wholly idle, in both modes, the reports against the numpy
model of the contract (tests/repair_model.py, run on the damaged rows read back
from the device) and reports, the whole source allocation and the whole parity
allocation (gap and guard bytes included), byte for byte, against what the same
call writes under the two-pass repair; the modes' semantics; the launch
sequence; the fallbacks; and a batch of more blocks than a grid holds.  More
than 64 source rows: tests/test_gpu_family_generated_wide.py."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import gpu_family as gf  # noqa: E402
import repair_model as rm  # noqa: E402
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402

DT = rsgpu.REPAIR_REPORT_DTYPE
CLEAN = (0, 0, rm.CLEAN, -1)
B = 5
SEQUENCE = {"columns": ["k_rs_jit_repair", "k_repair_finalise"],
            "one_row": ["k_rs_jit_repair", "k_repair_finalise", "k_rs_jit_repair_gated"]}

# tests/test_gpu_scrub_generated.py's shapes: the smallest that reach every
# layout of the generated kernels (every k no multiple of its layout's chunk)
LAYOUTS = [
    (10, 4, "rs"),      # 8-row layout, one wave, partial second chunk
    (11, 12, "rs"),     # 8-row layout, two waves, the last with 4 rows
    (13, 20, "rs"),     # 2 x 10 rows
    (13, 24, "rs"),     # 2 x 12 rows
    (14, 32, "rs"),     # 2 x 16 rows
    (9, 34, "rs"),      # four waves of 10 rows: 8, 9, 8, 9 rows
    (6, 3, "cauchy"),   # a caller's matrix
    (5, 4, "rs"),       # a compiled code through the generated program (also against fused)
]
# 32: one live lane; 2112: the second tile has 2 live lanes; 4160: 3 tiles, so
# with two tiles per workgroup the last workgroup owns a tile past the row end;
# 6144: 3 full tiles
LENGTHS = [32, 2112, 4160, 6144]


@pytest.fixture(scope="module")
def ctx():
    for c in gf.device_context(reset_scrub_kernel=True):
        yield c
        c.set_repair_kernel("auto")


class Blocks(gf.DeviceBlocks):
    def __init__(self, ctx, k, e, L, nb=B, pitch=None, **kw):
        super().__init__(ctx, k, e, L, nb, L + 48 if pitch is None else pitch, **kw)
        self.rep = torch.empty(nb * DT.itemsize, dtype=torch.uint8, device=self.dev)
        torch.cuda.synchronize()

    def hit(self, hits):
        """XORs [(block, row, column, x)], columns up to the pitch: the gap too."""
        full = lambda t, rows: t[: self.B * rows * self.pitch].view(self.B, rows, self.pitch)  # noqa: E731
        for b, row, col, x in hits:
            (full(self.src, self.k)[b, row] if row < self.k else full(self.par, self.e)[b, row - self.k])[col] ^= x
        torch.cuda.synchronize()

    def restore(self, snap):
        self.src_all.copy_(snap[0])
        self.par_all.copy_(snap[1])

    def repair(self, repair_kernel, mode, scrub_kernel="auto", names=None):
        """One call into a poisoned report buffer: (reports, the report's bytes,
        the source allocation, the parity allocation) after it; names: a list
        that receives the call's record names."""
        self.ctx.set_scrub_kernel(scrub_kernel)
        self.ctx.set_repair_kernel(repair_kernel)
        self.rep.fill_(gf.POISON)
        call = lambda: self.ctx.repair_blocks(self.k, self.e, self.L, self.pitch, self.B, self.src, self.par,  # noqa: E731
                                               self.rep, coef=self.coef, mode=mode)
        try:
            if names is None:
                call()
            else:
                names += gf.recorded(self.ctx, call)
        finally:
            self.ctx.set_repair_kernel("auto")
            self.ctx.set_scrub_kernel("auto")
        torch.cuda.synchronize()
        raw = self.rep.cpu().numpy()
        return raw.view(DT).copy(), raw.tobytes(), self.src_all.clone(), self.par_all.clone()

    def model(self, mode):
        """The model on the blocks as they are now: ([verdict per block], the
        allocations as the call must leave them)."""
        want = []
        src, par = self.snapshot()
        sv, pv = self.view(src[self.offset:], self.k), self.view(par[self.offset:], self.e)
        for b in range(self.B):
            s, p = self.host_block(b)
            s2, p2, verdict = rm.repair(self.c, s, p, mode)
            want.append(verdict)
            sv[b, :, : self.L] = torch.from_numpy(s2).to(sv.device)
            pv[b, :, : self.L] = torch.from_numpy(p2).to(pv.device)
        return want, (src, par)

    def check(self, mode, others=("two_pass",)):
        """From the blocks as they are now: generated == the model (reports and
        rows), and == every scrub kernel of `others` under the repair kernel
        auto, reports and whole allocations byte for byte.  Leaves the blocks
        as the generated repair left them; returns the model's verdicts."""
        damaged = self.snapshot()
        want, after = self.model(mode)
        names = []
        rep, raw, src, par = self.repair("generated", mode, names=names)
        assert names == SEQUENCE[mode]
        gf.same(rep, want, gf.REPAIR_FIELDS)
        assert torch.equal(src, after[0]), "source allocation against the model"
        assert torch.equal(par, after[1]), "parity allocation against the model"
        for kernel in others:
            self.restore(damaged)
            _, raw2, src2, par2 = self.repair("auto", mode, scrub_kernel=kernel)
            assert raw == raw2, (kernel, mode, "reports")
            assert torch.equal(src, src2), (kernel, mode, "source allocation")
            assert torch.equal(par, par2), (kernel, mode, "parity allocation")
        return want


def damage_sets(k, e, L, pitch):
    """Two calls' worth of (block, row, column, xor), one damage kind per
    block: [none | one source row: the first lane of tile 0, the last live lane
    of the last tile, byte len - 1 | parity row 0 | the last parity row | two
    columns naming different rows] and [two rows in one column (e >= 4) | bytes
    of the gap [len, pitch) of source and parity rows | a source row in the
    last tile only | a parity row of the second quarter | a middle parity row]:
    with rows 0, e / 4, e / 2 and e - 1 a correction lands in every wave's
    rows of every layout."""
    last = L - 1
    a = [(1, k - 1, 0, 0x01), (1, k - 1, min(31, last), 0x80), (1, k - 1, L - 32, 0xFF), (1, k - 1, last, 0x3C),
         (2, k, last, 0x5A), (2, k, 0, 0xC1),
         (3, k + e - 1, 0, 0x01), (3, k + e - 1, last, 0xF0),
         (4, 0, 0, 0x21), (4, k + 1, last, 0x9D)]
    b = [(1, 1, L, 0x55), (1, 1, pitch - 1, 0xAA), (1, k + e - 1, L, 0x55), (1, k, pitch - 1, 0xAA),
         (2, 0, L - L % 2048 if L % 2048 else L - 2048, 0x11),
         (3, k + e // 4, min(33, last), 0x6E),
         (4, k + e // 2, L // 2, 0x77)]
    if e >= 4:
        b += [(0, 0, L // 3, 0x17), (0, k - 1, L // 3, 0xE0)]
    return a, b


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k,e,kind", LAYOUTS, ids=str)
def test_rows_and_reports_match_the_model_and_two_pass(ctx, k, e, kind, L):
    others = ("two_pass", "fused") if (k, e, kind) == (5, 4, "rs") else ("two_pass",)
    for mode in rm.MODES:
        blk = Blocks(ctx, k, e, L, kind=kind)
        pristine = blk.snapshot()
        assert blk.check(mode, others) == [CLEAN] * B  # every block clean
        assert torch.equal(blk.src_all, pristine[0]) and torch.equal(blk.par_all, pristine[1])
        for n, hits in enumerate(damage_sets(k, e, L, blk.pitch)):
            blk.restore(pristine)
            blk.hit(hits)
            want = blk.check(mode, others)
            one = rm.REPAIRED
            if n == 0:
                two = len({0, L - 1})
                assert want == [CLEAN, (len({0, min(31, L - 1), L - 32, L - 1}),) * 2 + (one, k - 1),
                                (two, two, one, k), (two, two, one, k + e - 1),
                                (two, two, one, -1) if mode == "columns" else (two, 0, rm.DAMAGED, -1)]
            else:
                assert want[0] == ((1, 0, rm.DAMAGED, -1) if e >= 4 else CLEAN)
                assert want[1:] == [CLEAN, (1, 1, one, 0), (1, 1, one, k + e // 4), (1, 1, one, k + e // 2)]


def test_columns_corrects_what_one_row_explains_and_leaves_the_rest(ctx):
    """One correctable column and one with two damaged rows in a block: PARTIAL
    under COLUMNS, the second column as it was; the block untouched under
    ONE_ROW."""
    for k, e in ((10, 4), (14, 32)):
        L = 4160
        blk = Blocks(ctx, k, e, L)
        pristine = blk.snapshot()
        blk.hit([(2, 3, 4100, 0x42), (2, 1, 70, 0x17), (2, k + 1, 70, 0xE0)])
        damaged = blk.snapshot()
        rep, _, src, par = blk.repair("generated", "columns")
        gf.same(rep, [CLEAN, CLEAN, (2, 1, rm.PARTIAL, 3), CLEAN, CLEAN], gf.REPAIR_FIELDS)
        assert blk.row(2, 3)[4100] == blk.view(pristine[0], k)[2, 3, 4100]  # corrected
        assert torch.equal(blk.rows(1)[:, 70], blk.view(damaged[0], k)[:, 1, 70])  # left as it was
        assert torch.equal(blk.rows(k + 1)[:, 70], blk.view(damaged[1], e)[:, 1, 70])
        want = blk.view(damaged[0].clone(), k)
        want[2, 3, 4100] ^= 0x42
        assert torch.equal(blk.view(src, k), want) and torch.equal(par, damaged[1])
        blk.restore(damaged)
        rep, _, src, par = blk.repair("generated", "one_row")
        gf.same(rep, [CLEAN, CLEAN, (2, 0, rm.DAMAGED, -1), CLEAN, CLEAN], gf.REPAIR_FIELDS)
        assert torch.equal(src, damaged[0]) and torch.equal(par, damaged[1])


def test_one_row_leaves_a_block_of_two_rows_untouched(ctx):
    """The block whose two bad columns name different rows: DAMAGED under
    ONE_ROW and not a byte of it changes, while its neighbours are repaired."""
    k, e, L = 13, 20, 4160
    blk = Blocks(ctx, k, e, L)
    pristine = blk.snapshot()
    blk.hit([(1, 0, 0, 0x21), (1, k + 1, L - 1, 0x9D), (0, 5, 2050, 0x01), (2, k + 19, 17, 0x80)])
    damaged = blk.snapshot()
    rep, _, src, par = blk.repair("generated", "one_row")
    gf.same(rep, [(1, 1, rm.REPAIRED, 5), (2, 0, rm.DAMAGED, -1), (1, 1, rm.REPAIRED, k + 19), CLEAN, CLEAN],
            gf.REPAIR_FIELDS)
    for t, snap, pris, rows in ((src, damaged[0], pristine[0], k), (par, damaged[1], pristine[1], e)):
        assert torch.equal(blk.view(t, rows)[1], blk.view(snap, rows)[1]), "the damaged block was written"
        for b in (0, 2, 3, 4):
            assert torch.equal(blk.view(t, rows)[b], blk.view(pris, rows)[b])


@pytest.mark.parametrize("mode", rm.MODES)
def test_a_second_call_reports_clean(ctx, mode):
    k, e, L = 9, 34, 2112
    blk = Blocks(ctx, k, e, L)
    pristine = blk.snapshot()
    blk.hit([(0, 8, 2111, 0xFF), (0, 8, 0, 0x01), (3, k + 9, 2080, 0x10), (4, k + 33, 31, 0x08)])
    rep = blk.repair("generated", mode)[0]
    gf.same(rep, [(2, 2, rm.REPAIRED, 8), CLEAN, CLEAN, (1, 1, rm.REPAIRED, k + 9), (1, 1, rm.REPAIRED, k + 33)],
            gf.REPAIR_FIELDS)
    rep, _, src, par = blk.repair("generated", mode)
    gf.same(rep, [CLEAN] * B, gf.REPAIR_FIELDS)
    assert torch.equal(src, pristine[0]) and torch.equal(par, pristine[1])


def scrub_scratch_bytes(ctx):
    fn = rsgpu.testhooks().rsgpu_internal_scrub_scratch_bytes
    fn.restype, fn.argtypes = C.c_longlong, [C.c_void_p]
    return fn(ctx.handle)


@pytest.mark.parametrize("mode", rm.MODES)
def test_launch_sequence_and_no_parity_scratch(mode):
    """On a context of its own: the generated repair records its launches and
    the finalise, no encode, and leaves the scrub family's buffer at its
    tables; the two-pass repair of the same blocks then records an encode and
    grows the buffer by the slice's parity."""
    for c in gf.device_context():
        k, e, L = 10, 4, 6144  # a block's parity is larger than the buffer's tables
        blk = Blocks(c, k, e, L, kind="cauchy")
        assert scrub_scratch_bytes(c) == 0
        spare = blk.alloc(e)
        enc = gf.recorded(c, lambda: c.encode_blocks(k, e, L, blk.pitch, B, blk.src, spare, coef=blk.coef))
        assert enc
        blk.hit([(1, 4, 2100, 0x66), (3, k + 2, 0, 0x09)])
        damaged = blk.snapshot()
        names = []
        rep = blk.repair("generated", mode, names=names)[0]
        assert names == SEQUENCE[mode] and not set(enc) & set(names)
        tables = scrub_scratch_bytes(c)
        assert 0 < tables < e * blk.pitch, "the buffer has room for computed parity"
        gf.same(rep, [CLEAN, (1, 1, rm.REPAIRED, 4), CLEAN, (1, 1, rm.REPAIRED, k + 2), CLEAN], gf.REPAIR_FIELDS)
        blk.restore(damaged)
        names = []
        blk.repair("auto", mode, names=names)
        assert names[: len(enc)] == enc and "k_repair_compare" in names
        assert scrub_scratch_bytes(c) >= tables + B * e * blk.pitch
        # the scrub kernel GENERATED alone does not select it, and AUTO is the default
        blk.restore(damaged)
        names = []
        blk.repair("auto", mode, scrub_kernel="generated", names=names)
        assert "k_repair_compare" in names and "k_rs_jit_repair" not in names


def test_unknown_values_are_refused(ctx):
    with pytest.raises(KeyError):
        ctx.set_repair_kernel("fused")
    L = rsgpu.lib()
    for bad in (-1, 2, 3):
        assert L.rsgpu_set_repair_kernel(ctx.handle, bad) == -1
    blk = Blocks(ctx, 10, 4, 64)
    blk.xor(1, 2, 5, 0x31)
    names = []
    blk.repair("auto", "one_row", names=names)  # the refused values changed nothing
    assert "k_rs_jit_repair" not in names


def fallback_cases(ctx):
    yield "d_src offset by 1", Blocks(ctx, 10, 4, 64, pitch=64, offset=1)
    yield "pitch % 16 != 0", Blocks(ctx, 10, 4, 64, pitch=72)
    yield "len % 32 != 0", Blocks(ctx, 10, 4, 2100, pitch=2112)
    yield "e > 64", Blocks(ctx, 4, 65, 64)
    yield "a compiled code, misaligned pitch", Blocks(ctx, 5, 4, 64, pitch=72)


@pytest.mark.parametrize("mode", rm.MODES)
def test_fallbacks_run_what_auto_runs(ctx, mode):
    for what, blk in fallback_cases(ctx):
        assert sm.locatable(blk.c), what  # (4, 65): the two-pass repair takes it
        blk.hit([(1, 2, blk.L - 1, 0x44), (3, blk.k + blk.e - 1, 0, 0x02)])
        damaged = blk.snapshot()
        want, after = blk.model(mode)
        assert [w[:3] for w in want] == [CLEAN[:3], (1, 1, rm.REPAIRED), CLEAN[:3], (1, 1, rm.REPAIRED), CLEAN[:3]]
        auto_names, names = [], []
        _, raw2, src2, par2 = blk.repair("auto", mode, names=auto_names)
        blk.restore(damaged)
        rep, raw, src, par = blk.repair("generated", mode, names=names)
        assert names == auto_names and "k_repair_compare" in names, what
        gf.same(rep, want, gf.REPAIR_FIELDS)
        assert raw == raw2 and torch.equal(src, src2) and torch.equal(par, par2), what
        assert torch.equal(src, after[0]) and torch.equal(par, after[1]), what


def test_generated_comes_before_fused(ctx):
    """(5, 4) on rows the fused repair takes: AUTO records the compiled kernel,
    GENERATED the generated one, under every scrub kernel choice."""
    blk = Blocks(ctx, 5, 4, 2112)
    names = []
    blk.repair("auto", "columns", names=names)
    assert names == ["k_rs_bs_repair", "k_repair_finalise"]
    for scrub in ("auto", "fused", "two_pass", "generated"):
        names = []
        blk.repair("generated", "columns", scrub_kernel=scrub, names=names)
        assert names == SEQUENCE["columns"], scrub


def test_nothing_to_repair_records_only_the_finalise(ctx):
    for k, e, L in ((10, 4, 0), (10, 0, 64)):
        blk = Blocks(ctx, k, e, L, pitch=64, encode=False)
        names = []
        rep = blk.repair("generated", "one_row", names=names)[0]
        assert names == ["k_repair_finalise"]
        gf.same(rep, [CLEAN] * B, gf.REPAIR_FIELDS)


def test_unsupported_cases_are_shared(ctx):
    c = sm.rs_matrix(10, 4).copy()
    c[0, 3] = 0
    assert not sm.locatable(c)
    blk = Blocks(ctx, 10, 4, 2112, c=c)
    small = Blocks(ctx, 10, 2, 64)
    ctx.set_repair_kernel("generated")
    try:
        for b, mode in ((blk, "one_row"), (small, "columns")):
            b.rep.fill_(gf.POISON)
            with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_UNSUPPORTED"):
                ctx.repair_blocks(b.k, b.e, b.L, b.pitch, B, b.src, b.par, b.rep, coef=b.coef, mode=mode)
            torch.cuda.synchronize()
            assert (b.rep.cpu().numpy() == gf.POISON).all()
    finally:
        ctx.set_repair_kernel("auto")


def test_more_blocks_than_a_grid_holds(ctx):
    """65537 blocks of the (3, 3) Cauchy code at len 32: two slices, a damaged
    column in block 2 and one in block 65536, the second slice's only block."""
    nb = 65537
    for mode in rm.MODES:
        blk = Blocks(ctx, 3, 3, 32, nb=nb, pitch=32, kind="cauchy")
        pristine = blk.snapshot()
        blk.xor(2, 1, 31, 0xFF)
        blk.xor(65536, 3, 0, 0x01)
        names = []
        rep, _, src, par = blk.repair("generated", mode, names=names)
        assert names == SEQUENCE[mode] * 2
        assert tuple(int(v) for v in rep[2]) == (1, 1, rm.REPAIRED, 1)
        assert tuple(int(v) for v in rep[65536]) == (1, 1, rm.REPAIRED, 3)
        rest = np.delete(rep, [2, 65536])
        assert (rest["status"] == rm.CLEAN).all() and (rest["bad_columns"] == 0).all()
        assert (rest["repaired_columns"] == 0).all() and (rest["row"] == -1).all()
        assert torch.equal(src, pristine[0]) and torch.equal(par, pristine[1])
