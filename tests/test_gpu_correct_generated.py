"""rsgpu_correct_blocks under rsgpu_set_correct_kernel FUSED with the scrub
kernel GENERATED (k_rs_jit_correct / k_rs_jitw_correct, include/rsgpu.h): the
blocks and the comparison of tests/test_gpu_correct.py (Blocks, run: the
reports field by field and the whole source and parity allocations, padding
and sentinels included, against the numpy model of the contract,
tests/correct_model.py), the damage planned by position in the generated tile
(tests/correct_generated_cases.py).  Every call must also have run the kernel
the case expects, which the timing records say: the generated form records
k_rs_jit_correct and k_correct_finalise, no compare, no compiled kernel and
none of the names a plain encode of the same arguments records.

A tile is 2048 bytes, a lane's share 32: len 32 is one lane, 2112 a full tile
and two lanes, L0 = 6304 three full tiles and five lanes (a workgroup of three
tiles and one whose last two tiles lie past the row end); with plus48 the
bytes in [len, pitch) hold sentinels.

More than 64 source rows on the two- and four-wave layouts (here only on the
one-wave one): tests/test_gpu_family_generated_wide.py."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import correct_cases as cc  # noqa: E402
import correct_fused_cases as fc  # noqa: E402
import correct_generated_cases as gc  # noqa: E402
import correct_model as cm  # noqa: E402
import gpu_family as gf  # noqa: E402
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402
from test_gpu_correct import CLEAN, DT, FIELDS, Blocks, run  # noqa: E402
from test_gpu_correct_fused import columns_repair, encode_names  # noqa: E402

L0 = gc.L0
SHAPES = [(32, "eq"), (2112, "eq"), (L0, "eq"), (L0, "plus48")]
GENERATED, COMPILED, COMPARE = "k_rs_jit_correct", "k_rs_bs_correct", "k_correct_compare"


def set_tiles(ctx, n):
    f = rsgpu.testhooks().rsgpu_internal_set_jitw_tiles
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int]
    assert f(ctx.handle, n) == 0


@pytest.fixture(scope="module")
def ctx():
    for c in gf.device_context(reset_scrub_kernel=True):
        c.set_correct_kernel("fused")
        c.set_scrub_kernel("generated")
        yield c
        c.set_correct_kernel("auto")
        c.set_scrub_kernel("auto")
        set_tiles(c, 0)


def checked(blk, t, want, after, ran=GENERATED, poison=gf.POISON):
    """run(), and the kernels the call ran: the generated or the compiled one
    and no encode, or the two passes."""
    enc = encode_names(blk)
    names = set(gf.recorded(blk.ctx, lambda: run(blk, t, want, after, poison)))
    assert "k_correct_finalise" in names, names
    assert {n for n in (GENERATED, COMPILED, COMPARE) if n in names} == {ran}, names
    if ran == COMPARE:
        assert enc <= names, (names, enc)
    else:
        assert not (names & enc), (names, enc)


def planned(ctx, k, e, kind, L, mode, plan, B=cc.BLOCKS):
    blk = Blocks(ctx, k, e, kind, L, mode, B=B)
    for b in range(blk.B - 1):
        for _, col, hits in plan(k, e, L, b):
            blk.hit(b, hits, col)
    return blk


def own_matrix(ctx, c, L, mode):
    """Two blocks under a caller's matrix c."""
    e, k = c.shape
    pitch, offset = gf.pitch_of(L, mode)
    blk = Blocks.__new__(Blocks)
    gf.DeviceBlocks.__init__(blk, ctx, k, e, L, 2, pitch, offset, "cauchy", c=c)
    blk.rep = torch.empty(2 * DT.itemsize, dtype=torch.uint8, device=blk.dev)
    torch.cuda.synchronize()
    return blk


@pytest.mark.parametrize("L,mode", SHAPES, ids=str)
@pytest.mark.parametrize("k,e,kind", gc.T2_SHAPES, ids=str)
def test_every_layout(ctx, k, e, kind, L, mode):
    """Blocks 0 .. 2 damaged as planned, the last one clean: t = 2, a second
    call on the result, then t = 1 on the damaged state, which is also
    rsgpu_repair_blocks' COLUMNS; the two-wave wide layouts also with two and
    three tiles per workgroup."""
    blk = planned(ctx, k, e, kind, L, mode, gc.plan)
    damaged = blk.snapshot()
    want, after = blk.model(2)
    assert want[-1] == CLEAN and all(w[1] >= 1 for w in want[:-1]), want
    if L == L0:
        assert all(w[2] >= 9 and w[1] > w[2] and w[3] == cm.PARTIAL for w in want[:-1]), want
    checked(blk, 2, want, after)
    want2, after2 = blk.model(2)
    assert all(w[1] == 0 and w[3] in (cm.CLEAN, cm.DAMAGED) for w in want2) and blk.equals(after2)
    checked(blk, 2, want2, after2, poison=None)
    if 16 < e <= 32 and L == L0:
        for tiles in (2, 3):
            blk.restore(damaged)
            set_tiles(ctx, tiles)
            try:
                checked(blk, 2, want, after)
            finally:
                set_tiles(ctx, 0)
    blk.restore(damaged)
    want1, after1 = blk.model(1)
    assert all(w[2] == 0 for w in want1)
    checked(blk, 1, want1, after1)
    blk.restore(damaged)
    columns_repair(ctx, blk, want1, after1)


@pytest.mark.parametrize("L,mode", SHAPES[1:], ids=str)
@pytest.mark.parametrize("k,e,kind", gc.T1_SHAPES, ids=str)
def test_one_row_codes(ctx, k, e, kind, L, mode):
    """e < 5: t = 1 runs the generated form; two-row columns stay."""
    blk = planned(ctx, k, e, kind, L, mode, gc.t1_plan)
    damaged = blk.snapshot()
    want1, after1 = blk.model(1)
    assert all(w[1] >= 1 and w[2] == 0 and w[0] > w[1] for w in want1[:-1]) and want1[-1] == CLEAN
    checked(blk, 1, want1, after1)
    blk.restore(damaged)
    columns_repair(ctx, blk, want1, after1)


@pytest.mark.parametrize("k,e,kind", gc.BAND_SHAPES, ids=str)
def test_pairs_across_bands(ctx, k, e, kind):
    """k > 64, block 1 of 3 damaged in pairs of rows inside a 64-row band,
    across bands and on both sides of every band's edge, a column each: all of
    them two-row corrections; t = 1 leaves every byte; a second call finds the
    block clean."""
    blk = Blocks(ctx, k, e, kind, 4128, "plus48", B=3)
    todo = cc.band_pairs(k, e)
    for col, hits in todo:
        blk.hit(1, hits, col)
    damaged = blk.snapshot()
    n = len(todo)
    want, after = blk.model(2, [1])
    assert want == [CLEAN, (n, n, n, cm.REPAIRED, -1), CLEAN]
    assert torch.equal(after[0], blk.pristine[0]) and torch.equal(after[1], blk.pristine[1])
    checked(blk, 1, [CLEAN, (n, 0, 0, cm.DAMAGED, -1), CLEAN], damaged)
    checked(blk, 2, want, blk.pristine)
    checked(blk, 2, [CLEAN] * 3, blk.pristine, poison=None)


def test_three_rows_of_three_bands_are_left_alone(ctx):
    """(245, 5) Cauchy: a column damaged in data rows of three different
    bands stays byte for byte, the column beside it in row 244 alone is
    corrected."""
    blk = Blocks(ctx, 245, 5, "cauchy", 4128, "plus48", B=3)
    (col3, hits3), (col1, hits1) = cc.three_bands(245)
    blk.hit(1, hits3, col3)
    want_after = blk.snapshot()
    blk.hit(1, hits1, col1)
    want, after = blk.model(2, [1])
    assert want == [CLEAN, (2, 1, 0, cm.PARTIAL, 244), CLEAN]
    assert torch.equal(after[0], want_after[0]) and torch.equal(after[1], want_after[1])
    checked(blk, 2, want, after)
    checked(blk, 2, [CLEAN, (1, 0, 0, cm.DAMAGED, -1), CLEAN], after, poison=None)


def test_two_matching_pairs_leave_the_column_alone(ctx):
    """A caller's matrix with four dependent columns of [C | I]: the columns
    two pairs explain stay byte for byte, the one beside them is corrected."""
    blk = own_matrix(ctx, cc.dependent_matrix(), 4128, "plus48")
    for col, hits in cc.AMBIGUOUS + cc.UNIQUE:
        blk.hit(1, hits, col)
    want, after = blk.model(2)
    assert want == [CLEAN, (6, 1, 1, cm.PARTIAL, -1)]
    checked(blk, 2, want, after)
    checked(blk, 2, [CLEAN, (5, 0, 0, cm.DAMAGED, -1)], after, poison=None)


def test_two_matching_pairs_in_different_bands(ctx):
    """(129, 7) with dependent columns of [C | I] in one 64-row band, in two
    neighbouring ones and in the last, one-row band."""
    blk = own_matrix(ctx, cc.dependent_wide_matrix(), 4128, "plus48")
    for col, hits in cc.AMBIGUOUS_WIDE + cc.UNIQUE_WIDE:
        blk.hit(1, hits, col)
    n = len(cc.AMBIGUOUS_WIDE)
    want, after = blk.model(2)
    assert want == [CLEAN, (n + 2, 2, 2, cm.PARTIAL, -1)]
    checked(blk, 2, want, after)
    checked(blk, 2, [CLEAN, (n, 0, 0, cm.DAMAGED, -1)], after, poison=None)


def test_a_pair_at_every_position(ctx):
    """(11, 12) Cauchy, L = 2080: one damaged pair per block at each of the 32
    byte offsets of the first and of the last lane of the full tile and of the
    last tile's only lane."""
    k, e, L = 11, 12, 2080
    cols = [32 * lane + o for lane in (0, 63, 64) for o in range(32)]
    blk = Blocks(ctx, k, e, "cauchy", L, "eq", B=len(cols) + 1)
    rng = np.random.default_rng(8)
    for b, col in enumerate(cols):
        blk.hit(b, fc.hits_of(fc.PAIR_KINDS[b % len(fc.PAIR_KINDS)], k, e, rng), col)
    want, after = blk.model(2)
    assert want == [(1, 1, 1, cm.REPAIRED, -1)] * len(cols) + [CLEAN]
    assert torch.equal(after[0], blk.pristine[0]) and torch.equal(after[1], blk.pristine[1])
    checked(blk, 2, want, blk.pristine)


@pytest.mark.parametrize("k,e", [(12, 6), (14, 32)], ids=str)
def test_scattered_damage_that_locate_calls_damaged(ctx, k, e):
    """Block 1 damaged in 12 distinct rows, two per column: the locate gives
    it up, this call brings every column back, a second call is CLEAN."""
    L = 4128
    blk = Blocks(ctx, k, e, "cauchy", L, "plus48", B=3)
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
    checked(blk, 2, want, blk.pristine)
    checked(blk, 2, [CLEAN] * 3, blk.pristine, poison=None)


@pytest.mark.parametrize("k,e,kind", gc.T2_SHAPES, ids=str)
def test_generated_and_two_pass_agree(ctx, k, e, kind):
    """One damaged batch per layout: byte-identical reports and allocations."""
    blk = planned(ctx, k, e, kind, L0, "plus48", gc.plan)
    damaged = blk.snapshot()
    gen = []
    names = set(gf.recorded(ctx, lambda: gen.append(blk.correct(2))))
    assert GENERATED in names and COMPARE not in names
    got = blk.snapshot()
    blk.restore(damaged)
    ctx.set_correct_kernel("two_pass")
    try:
        two = []
        names = set(gf.recorded(ctx, lambda: two.append(blk.correct(2))))
    finally:
        ctx.set_correct_kernel("fused")
    assert COMPARE in names and GENERATED not in names
    assert two[0].tobytes() == gen[0].tobytes() and gen[0]["two_row_columns"][:-1].min() >= 9
    assert blk.equals(got)


def test_precedence_and_fallbacks(ctx):
    """(16, 8) gf_gen_rs_matrix: the compiled form has precedence; with the
    caller's coef equal to that matrix the generated form runs.  len % 32 != 0,
    rows one byte off alignment and the scrub kernel "auto": TWO_PASS runs, and
    is correct."""
    cases = [(16, 8, "rs", 4160, "plus48", False, None, COMPILED), (16, 8, "rs", 4160, "plus48", True, None, GENERATED),
             (12, 6, "cauchy", 4144, "eq", False, None, COMPARE), (12, 6, "cauchy", 4160, "mis1", False, None, COMPARE),
             (12, 6, "cauchy", 4160, "plus48", False, "auto", COMPARE)]
    for k, e, kind, L, mode, own_coef, scrub, ran in cases:
        blk = Blocks(ctx, k, e, kind, L, mode)
        if own_coef:
            blk.coef = blk.c
        for b in range(blk.B - 1):
            for _, col, hits in cc.plan(k, e, L, b):
                blk.hit(b, hits, col)
        want, after = blk.model(2)
        assert all(w[2] >= 9 for w in want[:-1])
        if scrub:
            ctx.set_scrub_kernel(scrub)
        try:
            checked(blk, 2, want, after, ran=ran)
        finally:
            ctx.set_scrub_kernel("generated")


def test_refusals_and_nothing_to_check(ctx):
    """As tests/test_gpu_correct_fused.py pins them: t outside {1, 2}
    RSGPU_ERR_ARG, t = 2 with e = 4 and an unlocatable matrix
    RSGPU_ERR_UNSUPPORTED, poison kept, nothing written; e == 0 / len == 0
    CLEAN with the finalise alone recorded."""
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
    four = Blocks(ctx, 12, 4, "cauchy", 2048, "eq", B=2)
    four.hit(1, [(3, 0x44)], 99)
    damaged = four.snapshot()
    with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_UNSUPPORTED"):
        four.correct(2)
    torch.cuda.synchronize()
    assert (four.rep.cpu().numpy() == gf.POISON).all() and four.equals(damaged)
    checked(four, 1, [CLEAN, (1, 1, 0, cm.REPAIRED, 3)], four.pristine)
    for k, e, L in ((12, 6, 0), (12, 0, 64)):
        none = Blocks.__new__(Blocks)
        gf.DeviceBlocks.__init__(none, ctx, k, e, L, 3, max(L, 16), 0, "cauchy", encode=False)
        none.rep = torch.empty(3 * DT.itemsize, dtype=torch.uint8, device=none.dev)
        torch.cuda.synchronize()
        before = none.snapshot()
        for t in (1, 2):
            names = gf.recorded(ctx, lambda: gf.same(none.correct(t), [CLEAN] * 3, FIELDS))
            assert names == ["k_correct_finalise"], names
            assert none.equals(before)


def test_more_blocks_than_a_grid_holds(ctx):
    """65539 blocks of (6, 5) Cauchy, L = 32: two slices, two launches of the
    generated kernel, damage on both sides of the slice edge."""
    B = 65536 + 3
    blk = Blocks(ctx, 6, 5, "cauchy", 32, "eq", B=B)
    blk.hit(65534, [(2, 0x31), (7, 0x07)], 31)
    blk.hit(65535, [(4, 0x80)], 0)
    blk.hit(65537, [(0, 0x01), (5, 0xFE)], 16)
    blk.hit(B - 1, [(6, 0x11), (10, 0x22)], 1)
    hit = [65534, 65535, 65537, B - 1]
    want, after = blk.model(2, hit)
    assert [want[b] for b in hit] == [(1, 1, 1, cm.REPAIRED, -1), (1, 1, 0, cm.REPAIRED, 4),
                                      (1, 1, 1, cm.REPAIRED, -1), (1, 1, 1, cm.REPAIRED, -1)]
    rep = []
    names = gf.recorded(ctx, lambda: rep.append(blk.correct(2)), blocks=True)
    assert names == [(GENERATED, 65535), (GENERATED, 4), ("k_correct_finalise", B)], names
    assert (rep[0]["status"] == cm.CLEAN).sum() == B - 4
    gf.same(rep[0][65530:], want[65530:], FIELDS)
    assert blk.equals(after) and blk.equals(blk.pristine)
