"""The generated scrub on the GPU (include/rsgpu.h RSGPU_SCRUB_GENERATED;
k_rs_jit_scrub, k_rs_jitw_scrub): for every layout of the generated kernels and
the lengths at which a tile, a lane or a workgroup is partly or wholly idle,
the reports under `generated` against the numpy model of the contract
(tests/scrub_model.py, run on the rows read back from the device) and, byte for
byte, against `two_pass`; with and without locate, into a poisoned report
buffer; the launch sequence; the fallbacks; and that the rows are only read.  More
than 64 source rows: tests/test_gpu_family_generated_wide.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import gpu_family as gf  # noqa: E402
import repair_model as rm  # noqa: E402
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402

DT = rsgpu.SCRUB_REPORT_DTYPE
GENERATED = ["k_rs_jit_scrub", "k_scrub_finalise"]
CLEAN = (0, sm.CLEAN, -1)
B = 5

# (k, e, matrix): every k is no multiple of its layout's chunk (8, 5 or 6 sources)
LAYOUTS = [
    (10, 4, "rs"),      # 8-row layout, one wave, partial second chunk
    (11, 12, "rs"),     # 8-row layout, two waves, the last with 4 rows
    (13, 20, "rs"),     # 2 x 10 rows
    (13, 24, "rs"),     # 2 x 12 rows
    (14, 32, "rs"),     # 2 x 16 rows
    (9, 34, "rs"),      # four waves of 10 rows: 8, 9, 8, 9 rows (wide_row0)
    (6, 3, "cauchy"),   # a caller's matrix
    (5, 4, "rs"),       # a compiled code through the generated program (also against fused)
]
# 32: one live lane; 2112: the second tile has 2 live lanes; 4160: 3 tiles, so
# with two tiles per workgroup the last workgroup owns a tile that does not
# exist; 6144: 3 full tiles
LENGTHS = [32, 2112, 4160, 6144]


@pytest.fixture(scope="module")
def ctx():
    yield from gf.device_context(reset_scrub_kernel=True)


class Blocks(gf.DeviceBlocks):
    def __init__(self, ctx, k, e, L, nb=B, pitch=None, **kw):
        super().__init__(ctx, k, e, L, nb, L + 48 if pitch is None else pitch, **kw)
        self.rep = torch.empty(nb * DT.itemsize, dtype=torch.uint8, device=self.dev)
        torch.cuda.synchronize()

    def scrub(self, kernel, locate=True, coef="own", names=None):
        """The reports of one call under `kernel` into a poisoned buffer;
        names: a list that receives the call's record names."""
        self.ctx.set_scrub_kernel(kernel)
        self.rep.fill_(gf.POISON)
        call = lambda: self.ctx.scrub_blocks(self.k, self.e, self.L, self.pitch, self.B, self.src, self.par,  # noqa: E731
                                              self.rep, coef=self.coef if isinstance(coef, str) else coef, locate=locate)
        try:
            if names is None:
                call()
            else:
                names += gf.recorded(self.ctx, call)
        finally:
            self.ctx.set_scrub_kernel("auto")
        torch.cuda.synchronize()
        return self.rep.cpu().numpy().view(DT).copy()

    def model(self, locate=True, c=None):
        hs, hp = self.host(self.src, self.k), self.host(self.par, self.e)
        return [sm.scrub(self.c if c is None else c, hs[b], hp[b], locate) for b in range(self.B)]

    def enc_names(self):
        """What a plain encode of the same rows records (into a spare buffer)."""
        spare = self.alloc(self.e)[self.offset:]
        return gf.recorded(self.ctx, lambda: self.ctx.encode_blocks(self.k, self.e, self.L, self.pitch, self.B,
                                                                    self.src, spare, coef=self.coef))

    def check(self, others=("two_pass",)):
        """generated == the model, and == every kernel of `others` byte for
        byte, with and without locate; the rows are not written."""
        before = self.snapshot()
        for locate in (True, False):
            names = []
            rep = self.scrub("generated", locate, names=names)
            assert names == GENERATED
            gf.same(rep, self.model(locate))
            for kernel in others:
                assert rep.tobytes() == self.scrub(kernel, locate).tobytes(), (kernel, locate)
        assert torch.equal(self.src_all, before[0]), "source allocation written"
        assert torch.equal(self.par_all, before[1]), "parity allocation written"


def damage_sets(k, e, L, pitch):
    """Two calls' worth of (block, row, column, xor), one damage kind per
    block: [none | one source row, first lane of tile 0 and last live lane of
    the last tile | parity row 0 | the last parity row | two columns naming
    different rows] and [two rows in one column (e >= 4) | a byte of the gap
    [len, pitch) of a source and of a parity row | a source row in the last
    tile only | none | a middle parity row]."""
    last = L - 1
    a = [(1, k - 1, 0, 0x01), (1, k - 1, min(31, last), 0x80), (1, k - 1, L - 32, 0xFF), (1, k - 1, last, 0x3C),
         (2, k, last, 0x5A),
         (3, k + e - 1, 0, 0x01), (3, k + e - 1, last, 0xF0),
         (4, 0, 0, 0x21), (4, k + 1, last, 0x9D)]
    b = [(1, 1, L, 0x55), (1, 1, pitch - 1, 0xAA), (1, k + e - 1, L, 0x55), (1, k, pitch - 1, 0xAA),
         (2, 0, L - L % 2048 if L % 2048 else L - 2048, 0x11),
         (4, k + e // 2, L // 2, 0x77)]
    if e >= 4:
        b += [(0, 0, L // 3, 0x17), (0, k - 1, L // 3, 0xE0)]
    return a, b


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k,e,kind", LAYOUTS, ids=str)
def test_reports_match_the_model_and_two_pass(ctx, k, e, kind, L):
    blk = Blocks(ctx, k, e, L, kind=kind)
    others = ("two_pass", "fused") if (k, e, kind) == (5, 4, "rs") else ("two_pass",)
    blk.check(others)  # every block clean
    assert blk.model() == [CLEAN] * B
    full = lambda t, rows: t[: B * rows * blk.pitch].view(B, rows, blk.pitch)  # noqa: E731
    for n, hits in enumerate(damage_sets(k, e, L, blk.pitch)):
        for b, row, col, x in hits:  # columns up to the pitch: the gap is damaged too
            (full(blk.src, k)[b, row] if row < k else full(blk.par, e)[b, row - k])[col] ^= x
        torch.cuda.synchronize()
        want = blk.model()
        if n == 0:
            assert want == [CLEAN, (len({0, min(31, L - 1), L - 32, L - 1}), sm.ONE_ROW, k - 1), (1, sm.ONE_ROW, k),
                            (len({0, L - 1}), sm.ONE_ROW, k + e - 1), (len({0, L - 1}), sm.DAMAGED, -1)]
        else:
            assert want[0] == ((1, sm.DAMAGED, -1) if e >= 4 else CLEAN)
            assert want[1:] == [CLEAN, (1, sm.ONE_ROW, 0), CLEAN, (1, sm.ONE_ROW, k + e // 2)]
        blk.check(others)
        for b, row, col, x in hits:
            (full(blk.src, k)[b, row] if row < k else full(blk.par, e)[b, row - k])[col] ^= x


def fallback_cases(ctx):
    yield "d_src offset by 1", Blocks(ctx, 10, 4, 64, pitch=64, offset=1)
    yield "pitch % 16 != 0", Blocks(ctx, 10, 4, 64, pitch=72)
    yield "len % 32 != 0", Blocks(ctx, 10, 4, 2100, pitch=2112)
    yield "e > 64", Blocks(ctx, 4, 66, 64)


def test_fallbacks_run_two_pass(ctx):
    for what, blk in fallback_cases(ctx):
        blk.xor(1, 2, blk.L - 1, 0x44)
        blk.xor(3, blk.k + blk.e - 1, 0, 0x02)
        enc = blk.enc_names()
        assert enc, what
        for locate in (True, False):
            names = []
            rep = blk.scrub("generated", locate, names=names)
            assert names == enc + ["k_scrub_compare", "k_scrub_finalise"], what
            want = blk.model(locate)
            assert [w[0] for w in want] == [0, 1, 0, 1, 0]
            gf.same(rep, want)


def test_nothing_to_scrub_records_only_the_finalise(ctx):
    for k, e, L in ((10, 4, 0), (10, 0, 64)):
        blk = Blocks(ctx, k, e, L, pitch=64, encode=False)
        names = []
        rep = blk.scrub("generated", locate=e >= 2, names=names)  # locate needs a locatable matrix, e >= 2
        assert names == ["k_scrub_finalise"]
        gf.same(rep, [CLEAN] * B)


def test_matrix_that_is_not_locatable(ctx):
    c = sm.rs_matrix(10, 4).copy()
    c[0, 3] = 0
    assert not sm.locatable(c)
    blk = Blocks(ctx, 10, 4, 2112, c=c)
    blk.xor(2, 3, 2100, 0x10)
    blk.xor(2, 12, 7, 0x01)
    names = []
    rep = blk.scrub("generated", locate=False, names=names)
    assert names == GENERATED
    gf.same(rep, [CLEAN, CLEAN, (2, sm.DAMAGED, -1), CLEAN, CLEAN])
    assert rep.tobytes() == blk.scrub("two_pass", locate=False).tobytes()
    blk.ctx.set_scrub_kernel("generated")
    blk.rep.fill_(gf.POISON)
    try:
        with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_UNSUPPORTED"):
            ctx.scrub_blocks(10, 4, blk.L, blk.pitch, B, blk.src, blk.par, blk.rep, coef=c, locate=True)
    finally:
        blk.ctx.set_scrub_kernel("auto")
    torch.cuda.synchronize()
    assert (blk.rep.cpu().numpy() == gf.POISON).all()


def test_each_call_follows_its_own_matrix(ctx):
    """Three matrices of (10, 4) by turns -- gf_gen_rs_matrix, Cauchy, and the
    RS rows with every column scaled (same ratios, another matrix) -- with a
    generated encode of one of them in between: the programs are cached per
    matrix, and the locate tables follow the call."""
    k, e, L = 10, 4, 2112
    scaled = sm.gf_mul(sm.rs_matrix(k, e), np.arange(3, 3 + k, dtype=np.uint8)[None, :])
    sets = [Blocks(ctx, k, e, L, kind="rs"), Blocks(ctx, k, e, L, kind="cauchy"), Blocks(ctx, k, e, L, c=scaled)]
    assert all(sm.locatable(s.c) for s in sets)
    for i, s in enumerate(sets):
        s.xor(1, 2 + i, 5, 0x31)
        s.xor(3, k + i, L - 1, 0x07)
    spare = sets[1].alloc(e)
    for turn in (0, 1, 2, 0, 1, 0, 2):
        s = sets[turn]
        rep = s.scrub("generated")
        gf.same(rep, [CLEAN, (1, sm.ONE_ROW, 2 + turn), CLEAN, (1, sm.ONE_ROW, k + turn), CLEAN])
        # the same rows under the next matrix: every column is bad, as the model says
        other = sets[(turn + 1) % 3]
        rep = s.scrub("generated", coef=other.c)
        want = s.model(c=other.c)
        assert all(w[0] > L // 2 and w[1] == sm.DAMAGED for w in want)
        gf.same(rep, want)
        if turn == 1:
            ctx.set_encode_kernel("generated")
            try:
                ctx.encode_blocks(k, e, L, s.pitch, B, s.src, spare, coef=s.coef)
            finally:
                ctx.set_encode_kernel("auto")
            torch.cuda.synchronize()
            full = spare[: B * e * s.pitch].view(B, e, s.pitch)[:, :, :L]
            clean = s.view(s.par, e)[:, :, :L].clone()
            clean[3, turn, L - 1] ^= 0x07  # the parity before the damage
            # block 1's source row is damaged, so its fresh parity differs; the others agree
            assert all(torch.equal(full[b], clean[b]) for b in (0, 2, 3, 4))


def test_more_blocks_than_a_grid_holds(ctx):
    nb = 65536 + 3
    blk = Blocks(ctx, 2, 2, 32, nb=nb, pitch=32)
    blk.xor(3, 1, 31, 0xFF)
    blk.xor(65537, 2, 0, 0x01)
    names = []
    rep = blk.scrub("generated", names=names)
    assert names == ["k_rs_jit_scrub", "k_rs_jit_scrub", "k_scrub_finalise"]
    assert int(rep["bad_columns"].sum()) == 2 and int((rep["status"] != sm.CLEAN).sum()) == 2
    assert (rep["row"][rep["status"] == sm.CLEAN] == -1).all()
    assert tuple(int(v) for v in rep[3]) == (1, sm.ONE_ROW, 1)
    assert tuple(int(v) for v in rep[65537]) == (1, sm.ONE_ROW, 2)
    assert rep.tobytes() == blk.scrub("two_pass").tobytes()


@pytest.mark.parametrize("mode", rm.MODES)
def test_repair_runs_its_two_pass_form(ctx, mode):
    k, e, L = 10, 4, 2112
    RDT = rsgpu.REPAIR_REPORT_DTYPE
    out = {}
    for kernel in ("two_pass", "generated"):
        blk = Blocks(ctx, k, e, L, kind="cauchy")
        blk.xor(1, 4, 2100, 0x66)
        blk.xor(3, k + 2, 0, 0x09)
        rep = torch.full((B * RDT.itemsize,), gf.POISON, dtype=torch.uint8, device=blk.dev)
        ctx.set_scrub_kernel(kernel)
        try:
            names = gf.recorded(ctx, lambda: ctx.repair_blocks(k, e, L, blk.pitch, B, blk.src, blk.par, rep,
                                                               coef=blk.coef, mode=mode))
        finally:
            ctx.set_scrub_kernel("auto")
        torch.cuda.synchronize()
        out[kernel] = (names, rep.cpu().numpy().tobytes(), blk.src_all.cpu(), blk.par_all.cpu(), blk)
    names, rep, src, par, blk = out["generated"]
    assert names == out["two_pass"][0] and "k_repair_compare" in names and "k_rs_jit_scrub" not in names
    assert rep == out["two_pass"][1]
    assert torch.equal(src, out["two_pass"][2]) and torch.equal(par, out["two_pass"][3])
    gf.same(np.frombuffer(rep, RDT), [(0, 0, rm.CLEAN, -1), (1, 1, rm.REPAIRED, 4), (0, 0, rm.CLEAN, -1),
                                      (1, 1, rm.REPAIRED, k + 2), (0, 0, rm.CLEAN, -1)], gf.REPAIR_FIELDS)
    assert blk.model() == [CLEAN] * B  # repaired in place
