"""rsgpu_correct_blocks under rsgpu_set_correct_kernel FUSED (k_rs_bs_correct,
include/rsgpu.h): the blocks and the comparison of tests/test_gpu_correct.py
(Blocks, run: the reports field by field and the whole source and parity
allocations, padding and sentinels included, against the numpy model of the
contract, tests/correct_model.py), the context set to "fused", the damage
planned by position in the fused tile (tests/correct_fused_cases.py) and for
the two-pass walk (tests/correct_cases.py).  Every call must also have run
the kernel the case expects, which the timing records say.

The fused kernel's tile is 2048 bytes, a lane's share 32: len 32 is one lane,
2080 a full tile and a one-lane tile, 4160 two full tiles and two lanes; at
4160 the pitch is len + 48, so that [len, pitch) holds sentinels."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import correct_cases as cc  # noqa: E402
import correct_fused_cases as fc  # noqa: E402
import correct_model as cm  # noqa: E402
import gpu_family as gf  # noqa: E402
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402
from test_gpu_correct import CLEAN, DT, FIELDS, Blocks, run  # noqa: E402

SHAPES = [(32, "eq"), (2080, "eq"), (4160, "plus48")]


@pytest.fixture(scope="module")
def ctx():
    for c in gf.device_context(reset_scrub_kernel=True):
        c.set_correct_kernel("fused")
        yield c
        c.set_correct_kernel("auto")


_encode_names = {}


def encode_names(blk):
    """The records a plain encode_blocks of the blocks' arguments leaves."""
    key = (blk.k, blk.e, blk.L, blk.pitch, blk.B, blk.offset, None if blk.coef is None else blk.coef.tobytes())
    if key not in _encode_names:
        out = torch.empty_like(blk.par_all)
        _encode_names[key] = set(gf.recorded(blk.ctx, lambda: blk.ctx.encode_blocks(
            blk.k, blk.e, blk.L, blk.pitch, blk.B, blk.src, out[blk.offset:], coef=blk.coef)))
        torch.cuda.synchronize()
        assert _encode_names[key]
    return _encode_names[key]


def checked(blk, t, want, after, fused=True, poison=gf.POISON):
    """run(), and the kernels the call ran: the fused one and no encode, or
    the two passes."""
    enc = encode_names(blk)
    names = set(gf.recorded(blk.ctx, lambda: run(blk, t, want, after, poison)))
    assert "k_correct_finalise" in names, names
    if fused:
        assert "k_rs_bs_correct" in names and "k_correct_compare" not in names and not (names & enc), (names, enc)
    else:
        assert "k_correct_compare" in names and "k_rs_bs_correct" not in names and enc <= names, (names, enc)


def planned(ctx, k, e, L, mode, plan):
    blk = Blocks(ctx, k, e, "rs", L, mode)
    for b in range(blk.B - 1):
        for _, col, hits in plan(k, e, L, b):
            blk.hit(b, hits, col)
    return blk


def columns_repair(ctx, blk, want1, after1):
    """rsgpu_repair_blocks COLUMNS on the blocks as they are: t = 1's reports and rows."""
    rep = torch.empty(blk.B * rsgpu.REPAIR_REPORT_DTYPE.itemsize, dtype=torch.uint8, device=blk.dev)
    ctx.repair_blocks(blk.k, blk.e, blk.L, blk.pitch, blk.B, blk.src, blk.par, rep, coef=blk.coef, mode="columns")
    torch.cuda.synchronize()
    gf.same(rep.cpu().numpy().view(rsgpu.REPAIR_REPORT_DTYPE), [(w[0], w[1], w[3], w[4]) for w in want1],
            gf.REPAIR_FIELDS)
    assert blk.equals(after1)


# the tile plan at every shape; correct_cases.plan, whose columns go up to 3007, at the longest
PLANNED = [(k, e, L, mode, plan) for k, e in fc.T2_CODES for L, mode in SHAPES
           for plan in (fc.plan, cc.plan) if plan is fc.plan or L == 4160]


@pytest.mark.parametrize("k,e,L,mode,plan", PLANNED, ids=lambda v: v.__module__ if callable(v) else str(v))
def test_planned_damage(ctx, k, e, L, mode, plan):
    """Blocks 0 .. 2 damaged as planned, the last one clean: t = 2, a second
    call on the result, then t = 1 on the damaged state, which is also
    rsgpu_repair_blocks' COLUMNS."""
    blk = planned(ctx, k, e, L, mode, plan)
    damaged = blk.snapshot()
    want, after = blk.model(2)
    assert want[-1] == CLEAN and all(w[1] >= 1 for w in want[:-1]), want
    if L == 4160:
        assert all(w[2] >= 9 and w[1] > w[2] and w[3] == cm.PARTIAL for w in want[:-1]), want
    checked(blk, 2, want, after)
    want2, after2 = blk.model(2)
    assert all(w[1] == 0 and w[3] in (cm.CLEAN, cm.DAMAGED) for w in want2) and blk.equals(after2)
    checked(blk, 2, want2, after2, poison=None)
    blk.restore(damaged)
    want1, after1 = blk.model(1)
    assert all(w[2] == 0 for w in want1)
    checked(blk, 1, want1, after1)
    blk.restore(damaged)
    columns_repair(ctx, blk, want1, after1)


@pytest.mark.parametrize("L,mode", SHAPES, ids=str)
@pytest.mark.parametrize("k,e", fc.T1_CODES, ids=str)
def test_one_row_codes(ctx, k, e, L, mode):
    """e = 4: t = 1 runs fused; two-row columns stay."""
    blk = planned(ctx, k, e, L, mode, fc.t1_plan)
    damaged = blk.snapshot()
    want1, after1 = blk.model(1)
    assert all(w[1] >= 1 and w[2] == 0 for w in want1[:-1]) and want1[-1] == CLEAN
    checked(blk, 1, want1, after1)
    blk.restore(damaged)
    columns_repair(ctx, blk, want1, after1)


@pytest.mark.parametrize("k,e", [(64, 32), (100, 20), (16, 8)], ids=str)
def test_scattered_damage_that_locate_calls_damaged(ctx, k, e):
    """Block 1 damaged in 12 distinct rows, two per column: the locate gives
    it up, the fused correct brings every column back, a second call is
    CLEAN."""
    L = 4160
    blk = Blocks(ctx, k, e, "rs", L, "plus48", B=3)
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


def test_a_pair_at_every_position(ctx):
    """(16, 8), L = 2080: one damaged pair per block at each of the 32 byte
    offsets of the first and of the last lane of the full tile and of the
    last tile's only lane."""
    k, e, L = 16, 8, 2080
    cols = [32 * lane + o for lane in (0, 63, 64) for o in range(32)]
    blk = Blocks(ctx, k, e, "rs", L, "eq", B=len(cols) + 1)
    rng = np.random.default_rng(8)
    kinds = fc.PAIR_KINDS
    for b, col in enumerate(cols):
        blk.hit(b, fc.hits_of(kinds[b % len(kinds)], k, e, rng), col)
    want, after = blk.model(2)
    assert want == [(1, 1, 1, cm.REPAIRED, -1)] * len(cols) + [CLEAN]
    assert torch.equal(after[0], blk.pristine[0]) and torch.equal(after[1], blk.pristine[1])
    checked(blk, 2, want, blk.pristine)


@pytest.mark.parametrize("k,e", fc.T2_CODES, ids=str)
def test_fused_and_two_pass_agree(ctx, k, e):
    """One damaged batch per code: byte-identical reports and allocations."""
    blk = planned(ctx, k, e, 4160, "plus48", fc.plan)
    damaged = blk.snapshot()
    blk.rep.fill_(gf.POISON)
    fused = blk.correct(2)
    got = blk.snapshot()
    blk.restore(damaged)
    ctx.set_correct_kernel("two_pass")
    try:
        blk.rep.fill_(gf.POISON)
        two = []
        names = set(gf.recorded(ctx, lambda: two.append(blk.correct(2))))
    finally:
        ctx.set_correct_kernel("fused")
    assert "k_correct_compare" in names and "k_rs_bs_correct" not in names
    assert two[0].tobytes() == fused.tobytes() and fused["two_row_columns"][:-1].min() >= 9
    assert blk.equals(got)


def test_fallbacks_run_two_pass(ctx):
    """A caller's coef equal to the RS matrix, a Cauchy (12, 6), len % 32 != 0,
    rows one byte off alignment: TWO_PASS runs, and is correct.  (No compiled
    plan is left out of FUSED.)"""
    cases = [(16, 8, "rs", 4160, "plus48", True), (12, 6, "cauchy", 4160, "plus48", False),
             (16, 8, "rs", 4144, "eq", False), (16, 8, "rs", 4160, "mis1", False)]
    for k, e, kind, L, mode, own_coef in cases:
        blk = Blocks(ctx, k, e, kind, L, mode)
        if own_coef:
            blk.coef = blk.c
        for b in range(blk.B - 1):
            for _, col, hits in cc.plan(k, e, L, b):
                blk.hit(b, hits, col)
        want, after = blk.model(2)
        assert all(w[2] >= 9 for w in want[:-1])
        checked(blk, 2, want, after, fused=False)


def test_refusals_and_nothing_to_check(ctx):
    """As tests/test_gpu_correct.py pins them under the default: t outside
    {1, 2} RSGPU_ERR_ARG, t = 2 with e = 4 and an unlocatable matrix
    RSGPU_ERR_UNSUPPORTED, poison kept, nothing written; e == 0 / len == 0
    CLEAN."""
    blk = Blocks(ctx, 16, 8, "rs", 2048, "eq", B=2)
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
        ctx.correct_blocks(16, 8, 2048, blk.pitch, 2, blk.src, blk.par, blk.rep, coef=bad, t=2)
    with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_ARG"):
        ctx.correct_blocks(16, 8, 2048, blk.pitch, 2, blk.src, blk.par, blk.rep[1:], coef=None, t=2)
    h, lib = ctx._h, rsgpu.lib()
    s, p, r = blk.src.data_ptr(), blk.par.data_ptr(), blk.rep.data_ptr()
    for src, par, rep in ((None, p, r), (s, None, r), (s, p, None)):
        assert lib.rsgpu_correct_blocks(h, 16, 8, 2048, blk.pitch, 2, src, par, None, 2, rep) == -1
    torch.cuda.synchronize()
    assert (blk.rep.cpu().numpy() == gf.POISON).all() and blk.equals(damaged)
    four = Blocks(ctx, 16, 4, "rs", 2048, "eq", B=2)
    four.hit(1, [(3, 0x44)], 99)
    damaged = four.snapshot()
    with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_UNSUPPORTED"):
        four.correct(2)
    torch.cuda.synchronize()
    assert (four.rep.cpu().numpy() == gf.POISON).all() and four.equals(damaged)
    checked(four, 1, [CLEAN, (1, 1, 0, cm.REPAIRED, 3)], four.pristine)
    for k, e, L in ((16, 8, 0), (16, 0, 64)):
        none = Blocks.__new__(Blocks)
        gf.DeviceBlocks.__init__(none, ctx, k, e, L, 3, max(L, 16), 0, "rs", encode=False)
        none.rep = torch.empty(3 * DT.itemsize, dtype=torch.uint8, device=none.dev)
        torch.cuda.synchronize()
        before = none.snapshot()
        for t in (1, 2):
            names = gf.recorded(ctx, lambda: gf.same(none.correct(t), [CLEAN] * 3, FIELDS))
            assert names == ["k_correct_finalise"], names
            assert none.equals(before)


def test_more_blocks_than_a_grid_holds(ctx):
    """65539 blocks of (5, 4), L = 32, t = 1: two slices, two launches of the
    fused kernel, damage on both sides of the slice edge."""
    B = 65536 + 3
    blk = Blocks(ctx, 5, 4, "rs", 32, "eq", B=B)
    blk.hit(65534, [(2, 0x31)], 31)
    blk.hit(65535, [(4, 0x80)], 0)
    blk.hit(65537, [(8, 0x01)], 16)
    blk.hit(B - 1, [(0, 0x11), (6, 0x22)], 1)
    hit = [65534, 65535, 65537, B - 1]
    want, after = blk.model(1, hit)
    assert [want[b] for b in hit] == [(1, 1, 0, cm.REPAIRED, 2), (1, 1, 0, cm.REPAIRED, 4), (1, 1, 0, cm.REPAIRED, 8),
                                      (1, 0, 0, cm.DAMAGED, -1)]
    rep = []
    names = gf.recorded(ctx, lambda: rep.append(blk.correct(1)), blocks=True)
    assert names == [("k_rs_bs_correct", 65535), ("k_rs_bs_correct", 4), ("k_correct_finalise", B)], names
    assert (rep[0]["status"] == cm.CLEAN).sum() == B - 4
    gf.same(rep[0][65530:], want[65530:], FIELDS)
    assert blk.equals(after)
