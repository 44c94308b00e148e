"""Degraded scrub on the GPU (include/rsgpu.h rsgpu_scrub_degraded_blocks):
data from fill_synthetic, parity from encode_blocks, rows then damaged with
torch indexing and lost rows overwritten.  Whole report arrays are compared
with the numpy model of the contract (tests/degraded_model.py), run on the
syndromes of the blocks as read back from the device (stored parity ^ the CPU
oracle's encode of the stored sources: nothing of the device's arithmetic is
trusted).  Every allocation is filled with 0x6B first, so the padding is not
zero, and compared whole with a clone taken before the call: the call only
reads."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import degraded_model as dm  # noqa: E402
import gpu_family as gf  # noqa: E402
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402
from oracle_lib import Oracle  # noqa: E402

N = dm.NONE
DT = rsgpu.SCRUB_REPORT_DTYPE
POISON = gf.POISON
Stripe, CASES, same, mixed_lists, damage = gf.DegradedStripe, gf.CASES, gf.same, gf.mixed_lists, gf.damage


@pytest.fixture(scope="module")
def ctx():
    yield from gf.device_context()


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.mark.parametrize("k,e,kind,L,B,u,mode", CASES, ids=str)
def test_against_the_model(ctx, orc, k, e, kind, L, B, u, mode):
    """Mixed lists and mixed damage against the model, with the lost rows
    zeroed and then filled with noise: the same reports both times."""
    st = Stripe(ctx, k, e, L, B, u, kind, mode)
    st.lost = mixed_lists(k, e, u, B)
    damage(st)
    st.fill_lost(None)
    want = st.model(orc)
    got = st.scrub()
    same(got, want)
    if B > 1:
        statuses = {w[1] for w in want}
        assert {dm.CLEAN, dm.ONE_ROW, dm.DAMAGED} <= statuses
        assert (dm.UNCHECKED in statuses) == (u >= e)
    same(st.scrub(locate=False), st.model(orc, locate=False))
    st.fill_lost(77)
    again = st.scrub()
    assert again.tobytes() == got.tobytes(), "the lost rows' contents changed a report"


@pytest.mark.parametrize("k,e,kind,L,B,u,mode", gf.WIDE_CASES, ids=str)
def test_wide_against_the_model(ctx, orc, k, e, kind, L, B, u, mode):
    """More than 64 source rows, or parity rows: the same comparison with
    lists around the edges of the 64-row bands in blocks 2..5, one of them
    damaged in the last data row (at (9, 70) the last parity row), which the
    model must name, and one in two rows."""
    st = Stripe(ctx, k, e, L, B, u, kind, mode)
    st.lost = gf.wide_lists(k, e, u, B)
    one, two = gf.wide_damage(st)
    st.fill_lost(None)
    want = st.model(orc)
    assert {dm.CLEAN, dm.ONE_ROW, dm.DAMAGED} <= {w[1] for w in want}
    assert want[one] == (1, dm.ONE_ROW, gf.wide_row(k, e)) and want[two] == (2, dm.DAMAGED, -1)
    assert any(w[1] == dm.ONE_ROW and w[2] >= (k + 64 if k <= 64 else 64) for w in want)
    got = st.scrub()
    same(got, want)
    same(st.scrub(locate=False), st.model(orc, locate=False))
    st.fill_lost(77)
    again = st.scrub()
    assert again.tobytes() == got.tobytes(), "the lost rows' contents changed a report"


@pytest.mark.parametrize("k,e,kind,L,B", [(16, 4, "rs", 4176, 67), (16, 4, "rs", 4160, 67),  # 4160: the fused scrub
                                          (10, 4, "cauchy", 2080, 67),
                                          (64, 32, "rs", 4099, 67), (20, 7, "rs", 31, 67)], ids=str)
def test_all_none_is_the_scrub(ctx, k, e, kind, L, B):
    """All-NONE lists: the report equals scrub_blocks' with LOCATE byte for
    byte, under every scrub kernel choice."""
    st = Stripe(ctx, k, e, L, B, 2, kind, "tail")
    damage(st)
    got = st.scrub()
    assert {int(s) for s in got["status"]} == {dm.CLEAN, dm.ONE_ROW, dm.DAMAGED}
    ref = torch.empty_like(st.rep)
    for kernel in ("two_pass", "auto"):
        ctx.set_scrub_kernel(kernel)
        try:
            ref.fill_(0x3C)
            ctx.scrub_blocks(k, e, L, st.pitch, B, st.src, st.par, ref, coef=st.coef, locate=True)
            torch.cuda.synchronize()
        finally:
            ctx.set_scrub_kernel("auto")
        assert ref.cpu().numpy().tobytes() == got.tobytes(), kernel
    nolocate = st.scrub(locate=False)
    ctx.scrub_blocks(k, e, L, st.pitch, B, st.src, st.par, ref, coef=st.coef, locate=False)
    torch.cuda.synchronize()
    assert ref.cpu().numpy().tobytes() == nolocate.tobytes()


def test_lists_and_matrices(ctx, orc):
    """Every malformation, n == e, a matrix whose first parity row is zero on
    D (the greedy pivots skip it) and a rank-deficient one, in one batch of a
    caller's matrix; the damaged BAD_LIST block is not looked at."""
    k, e, L, u = 8, 4, 100, 5
    c = sm.cauchy_matrix(k, e).copy()
    c[:, 5] = sm.gf_mul(c[:, 2], 0x35)  # columns 2 and 5 proportional
    c[0, 1] = c[0, 4] = 0               # parity row 0 blind to rows 1 and 4
    lists = [[3, 3, N, N, N], [4, 2, N, N, N], [12, N, N, N, N], [N, 2, N, N, N], [0, N, 1, N, N],
             [0, 1, 2, 3, 4], [0, 1, 2, 200, N],
             [0, 1, 2, 3, N], [8, 9, 10, 11, N], [0, 3, 9, 11, N],
             [1, 4, N, N, N], [1, 4, N, N, N], [1, 4, 8, N, N], [1, 4, N, N, N],
             [2, 5, N, N, N], [2, 5, 9, N, N], [2, N, N, N, N], [5, 11, N, N, N],
             [N, N, N, N, N], [11, N, N, N, N], [0, N, N, N, N]]
    B = len(lists)
    st = Stripe(ctx, k, e, L, B, u, "cauchy", "eq", c=c)
    st.lost = np.array(lists, np.uint8)
    st.xor(0, 6, 5, 0x11)    # BAD_LIST: stays BAD_LIST, bad_columns 0
    st.xor(7, 6, 5, 0x11)    # UNCHECKED: nobody can see it
    st.xor(11, 6, 50, 0x40)  # rows 1, 4 lost: pivots are parity rows 1, 2
    st.xor(12, k + 1, 99, 0x01)
    st.xor(13, k + 0, 0, 0x80)
    st.xor(14, 6, 5, 0x11)   # BAD_MATRIX
    st.xor(16, 7, 7, 0x07)
    st.xor(18, 0, 0, 0x01)
    torch.cuda.synchronize()
    st.fill_lost(None)
    want = st.model(orc)
    assert [w[1] for w in want[:7]] == [dm.BAD_LIST] * 7
    assert [w[1] for w in want[7:10]] == [dm.UNCHECKED] * 3
    assert want[10] == (0, dm.CLEAN, -1) and want[11][0] == 1 and want[13][0] == 1
    assert [w[1] for w in want[14:16]] == [dm.BAD_MATRIX] * 2 and want[16][1] != dm.BAD_MATRIX
    got = st.scrub()
    same(got, want)
    same(st.scrub(locate=False), st.model(orc, locate=False))
    st.fill_lost(31)
    assert st.scrub().tobytes() == got.tobytes(), "the lost rows' contents changed a report"


def test_nothing_to_check(ctx):
    """e == 0 and len == 0: CLEAN for a well-formed list, BAD_LIST otherwise."""
    for k, e, L in ((6, 0, 64), (5, 4, 0)):
        st = Stripe(ctx, k, e, L, 4, 4, "rs", "plus48")
        st.lost = np.array([[N, N, N, N], [0, 1, N, N] if e else [N, N, N, N], [1, 0, N, N], [0, 1, 2, 3]], np.uint8)
        want = [(0, dm.CLEAN, -1), (0, dm.CLEAN, -1), (0, dm.BAD_LIST, -1),
                (0, dm.CLEAN, -1) if e else (0, dm.BAD_LIST, -1)]
        same(st.scrub(), want)


def test_error_returns_leave_the_report_alone(ctx):
    st = Stripe(ctx, 5, 4, 64, 3, 2, "rs", "eq")
    d_lost = torch.from_numpy(st.lost).to(st.dev)
    rep = torch.empty(3 * DT.itemsize + 8, dtype=torch.uint8, device=st.dev)
    L = rsgpu.lib()
    h = ctx.handle

    def call(src=st.src, par=st.par, u=2, lost=d_lost, flags=1, report=rep, pitch=64, blocks=3):
        rep.fill_(POISON)
        rc = L.rsgpu_scrub_degraded_blocks(h, 5, 4, 64, pitch, blocks, rsgpu._ptr(src), rsgpu._ptr(par), None, u,
                                           rsgpu._ptr(lost), flags, rsgpu._ptr(report))
        torch.cuda.synchronize()
        assert (rep.cpu().numpy() == POISON).all() or rc == 0
        return rc

    assert call() == 0
    assert call(src=None) == -1 and call(par=None) == -1 and call(lost=None) == -1 and call(report=None) == -1
    assert call(report=rep[4:]) == -1  # misaligned
    assert call(u=0) == -1 and call(u=9) == -1
    assert call(flags=2) == -1 and call(flags=3) == -1
    assert call(pitch=63) == -1 and call(blocks=0) == -1


def test_slices(ctx):
    """(2, 8) with 1 MiB rows: 8 MiB of parity per block, so the 128 MiB
    scratch holds 16 blocks and 17 blocks run as two slices; the damage sits
    in the last block of the first slice and in the only block of the second.
    The model runs on the damaged columns and a few others (the full rows are
    consistent by construction: encode_blocks, tested on its own)."""
    k, e, L, B, u = 2, 8, 1 << 20, 17, 3
    st = Stripe(ctx, k, e, L, B, u, "rs", "eq")
    st.lost[15] = [0, k + 2, N]
    st.lost[16] = [k + 0, k + 7, N]
    st.lost[3] = [1, 0, N]
    st.lost[4] = [1, N, N]
    st.xor(15, 1, 0, 0x10)
    st.xor(15, 1, L - 1, 0xEE)
    st.xor(16, k + 3, 12345, 0x02)
    st.xor(16, 0, 777, 0x03)
    torch.cuda.synchronize()
    st.fill_lost(5)
    cols = torch.tensor([0, 1, 777, 12345, L - 2, L - 1], device=st.dev)
    hs = st.view(st.src, k)[:, :, cols].cpu().numpy()
    hp = st.view(st.par, e)[:, :, cols].cpu().numpy()
    want = [dm.report(st.c, hs[b], hp[b], st.lost[b]) for b in range(B)]
    assert want[15] == (2, dm.ONE_ROW, 1) and want[16] == (2, dm.DAMAGED, -1) and want[3][1] == dm.BAD_LIST
    got = st.scrub()
    same(got, want)
    st.fill_lost(None)
    assert st.scrub().tobytes() == got.tobytes(), "the lost rows' contents changed a report"


def test_more_blocks_than_a_grid_holds(ctx):
    """65535 + 3 blocks run as two slices of the grid; lists and damage on
    both sides of the boundary.  The model runs on those blocks; every other
    block is consistent with an all-NONE list."""
    k, e, L, u = 5, 4, 16, 2
    B = 65535 + 3
    st = Stripe(ctx, k, e, L, B, u, "rs", "eq")
    edge = [0, 65533, 65534, 65535, 65536, B - 1]
    st.lost[65533] = [0, N]
    st.lost[65534] = [2, k + 1]
    st.lost[65535] = [k + 0, N]
    st.lost[65536] = [1, 0]
    st.lost[B - 1] = [3, N]
    st.xor(65534, 4, 15, 0x09)
    st.xor(65535, 1, 0, 0x90)
    st.xor(B - 1, k + 3, 7, 0x01)
    torch.cuda.synchronize()
    st.fill_lost(3)
    want = {}
    for b in edge:
        hs = st.view(st.src, k)[b, :, :L].contiguous().cpu().numpy()
        hp = st.view(st.par, e)[b, :, :L].contiguous().cpu().numpy()
        want[b] = dm.report(st.c, hs, hp, st.lost[b])
    assert want[65534][1] == dm.ONE_ROW and want[65535] == (1, dm.ONE_ROW, 1) and want[65536][1] == dm.BAD_LIST
    got = st.scrub()
    for b in edge:
        assert (int(got[b]["bad_columns"]), int(got[b]["status"]), int(got[b]["row"])) == want[b], b
    rest = np.ones(B, bool)
    rest[edge] = False
    assert (got["bad_columns"][rest] == 0).all() and (got["status"][rest] == dm.CLEAN).all()
    assert (got["row"][rest] == -1).all()


def test_encoder_scrub_degraded(ctx):
    enc = rsgpu.GpuEncoder(16, 4096, 4, blocks=3, seed=2, ctx=ctx)
    enc.encode_all()
    lost = np.array([[N, N], [3, 17], [5, N]], np.uint8)
    enc.src.view(3, 16, enc.pitch)[1, 3].zero_()
    enc.src.view(3, 16, enc.pitch)[2, 9, 100] ^= 0x20
    rep = enc.scrub_degraded(lost)
    same(rep, [(0, dm.CLEAN, -1), (0, dm.CLEAN, -1), (1, dm.ONE_ROW, 9)])
    with pytest.raises(ValueError):
        enc.scrub_degraded(lost[:2])
