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
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402
from oracle_lib import Oracle  # noqa: E402

N = dm.NONE
DT = rsgpu.SCRUB_REPORT_DTYPE
POISON = 0xA5


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU test needs a HIP device"
    c = rsgpu.Context(0)
    c.set_torch_stream()
    yield c
    torch.cuda.synchronize()
    c.close()


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def matrix(k, e, kind):
    return sm.rs_matrix(k, e) if kind == "rs" else sm.cauchy_matrix(k, e)


def pitch_of(L, mode):
    """eq: pitch == len; plus48: len + 48; mis1: rows one byte past the
    allocation's alignment; tail: a 16-byte aligned pitch around a len that
    is no multiple of 16 (vector body, byte tail)."""
    if mode == "plus48":
        return L + 48, 0
    if mode == "mis1":
        return L, 1
    if mode == "tail":
        return (L + 255) // 256 * 256, 0
    return L, 0


class Stripe:
    """B consistent synthetic blocks on the device, a list of lost rows per block."""

    def __init__(self, ctx, k, e, L, B, u, kind="rs", mode="eq", seed=11, c=None):
        self.ctx, self.k, self.e, self.L, self.B, self.u = ctx, k, e, L, B, u
        self.pitch, offset = pitch_of(L, mode)
        self.c = matrix(k, e, kind) if c is None else np.ascontiguousarray(c, np.uint8)
        self.coef = None if kind == "rs" and c is None else self.c
        self.dev = dev = torch.device("cuda", 0)

        def alloc(rows):  # at least a byte, so that the pointer is not null
            t = torch.empty(max(1, B * rows * self.pitch) + offset, dtype=torch.uint8, device=dev)
            t.fill_(0x6B)
            return t

        self.src_all, self.par_all = alloc(k), alloc(e)
        self.src, self.par = self.src_all[offset:], self.par_all[offset:]
        ctx.fill_synthetic(self.src, B * k, L, self.pitch, seed, 0)
        ctx.encode_blocks(k, e, L, self.pitch, B, self.src, self.par, coef=self.coef)
        self.lost = np.full((B, u), N, np.uint8)
        self.rep = torch.empty(B * DT.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

    def view(self, t, rows):
        return t[: self.B * rows * self.pitch].view(self.B, rows, self.pitch)

    def row(self, blk, row):
        if row < self.k:
            return self.view(self.src, self.k)[blk, row, : self.L]
        return self.view(self.par, self.e)[blk, row - self.k, : self.L]

    def xor(self, blk, row, col, x):
        self.row(blk, row)[col] ^= x

    def fill_lost(self, seed):
        """Every listed row of every well-formed list: zero (seed None) or noise."""
        g = torch.Generator(device="cpu").manual_seed(seed or 0)
        for b in range(self.B):
            for r in dm.list_rows(self.lost[b], self.k, self.e) or []:
                if seed is None:
                    self.row(b, r).zero_()
                else:
                    self.row(b, r).copy_(torch.randint(0, 256, (self.L,), dtype=torch.uint8, generator=g))

    def scrub(self, locate=True):
        d_lost = torch.from_numpy(self.lost).to(self.dev)
        self.rep.fill_(POISON)
        before = self.src_all.clone(), self.par_all.clone()
        self.ctx.scrub_degraded_blocks(self.k, self.e, self.L, self.pitch, self.B, self.src, self.par, self.u,
                                       d_lost, self.rep, coef=self.coef, locate=locate)
        torch.cuda.synchronize()
        assert torch.equal(self.src_all, before[0]), "source allocation written"
        assert torch.equal(self.par_all, before[1]), "parity allocation written"
        assert (d_lost.cpu().numpy() == self.lost).all(), "lists written"
        return self.rep.cpu().numpy().view(DT).copy()

    def model(self, orc, locate=True):
        """The model's reports on the blocks as they are on the device now."""
        hs = self.view(self.src, self.k)[:, :, : self.L].contiguous().cpu().numpy()
        hp = self.view(self.par, self.e)[:, :, : self.L].contiguous().cpu().numpy()
        g = orc.init_tables(self.k, self.e, self.c) if self.e else None
        out = []
        for b in range(self.B):
            syn = hp[b].copy()
            if self.e and self.L:
                calc = [np.zeros(self.L, np.uint8) for _ in range(self.e)]
                orc.encode_data(self.L, self.k, self.e, g, [np.ascontiguousarray(r) for r in hs[b]], calc)
                syn ^= np.stack(calc)
            out.append(dm.report_syn(self.c, syn, self.lost[b], locate))
        return out


def same(rep, want):
    got = [(int(r["bad_columns"]), int(r["status"]), int(r["row"])) for r in rep]
    assert got == [tuple(w) for w in want], [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != tuple(w)]


def mixed_lists(k, e, u, B, seed=5):
    """Per block n = b mod (min(u, e) + 1) lost rows, n == e included where u
    allows; data only, parity only and both by turns; block 0 holds the first
    rows, block 1 the last ones."""
    rng = np.random.default_rng(seed)
    nmax = min(u, e)
    lost = np.full((B, u), N, np.uint8)
    for b in range(B):
        n = b % (nmax + 1) if B > 1 else min(nmax, max(1, e - 2))
        kind = (b // (nmax + 1)) % 3
        if kind == 0:  # data only
            rows = rng.choice(k, min(n, k), replace=False)
        elif kind == 1:  # parity only
            rows = k + rng.choice(e, n, replace=False)
        else:
            rows = rng.choice(k + e, n, replace=False)
        lost[b] = dm.pad(np.sort(rows), u)
    if B > 2:
        n = min(nmax, max(1, e - 2))
        lost[0] = dm.pad(np.arange(n), u)
        lost[1] = dm.pad(np.arange(k + e - n, k + e), u)
    return lost


def damage(st, seed=9):
    """Block b gets damage kind (b // (min(u, e) + 1)) mod 7, so that every
    kind meets every n: none; one byte of a survivor; one survivor in several
    columns, the first and the last included; two survivors in different
    columns; two survivors in one column; a byte of the first surviving parity
    row (a pivot row when data rows are lost); a byte of the last surviving
    parity row (a rest row)."""
    rng = np.random.default_rng(seed)
    k, e, L = st.k, st.e, st.L
    nmax = min(st.u, e)
    for b in range(st.B):
        lost = dm.list_rows(st.lost[b], k, e) or []
        surv = [r for r in range(k + e) if r not in lost]
        spar = [r for r in surv if r >= k]
        kind = (b // (nmax + 1)) % 7 if st.B > 1 else 2
        x = lambda: int(rng.integers(1, 256))  # noqa: E731
        pick = lambda n: [int(r) for r in rng.choice(surv, n, replace=False)]  # noqa: E731
        if kind == 1:
            st.xor(b, pick(1)[0], int(rng.integers(0, L)), x())
        elif kind == 2:
            r = pick(1)[0]
            for col in sorted({0, L - 1, L // 2, (L // 3) | 1 if L > 1 else 0, min(17, L - 1)}):
                st.xor(b, r, col, x())
        elif kind == 3:
            r1, r2 = pick(2)
            st.xor(b, r1, 0, x())
            st.xor(b, r2, L - 1 if L > 1 else 0, x())
        elif kind == 4:
            r1, r2 = pick(2)
            col = int(rng.integers(0, L))
            st.xor(b, r1, col, x())
            st.xor(b, r2, col, x())
        elif kind == 5 and spar:
            st.xor(b, spar[0], int(rng.integers(0, L)), x())
        elif kind == 6 and spar:
            st.xor(b, spar[-1], int(rng.integers(0, L)), x())
    torch.cuda.synchronize()


# codes (5, 4) (16, 4) (20, 7) (64, 32) RS and Cauchy (10, 4); len in {1, 31,
# 32, 2080, 4176} and 4099 (a 16-byte body with a 3-byte tail); the three
# pitches; blocks in {1, 67}; u in {1, 2, 4, 8}
CASES = [
    (5, 4, "rs", 4176, 67, 4, "plus48"),
    (5, 4, "rs", 1, 67, 1, "eq"),
    (5, 4, "rs", 31, 67, 2, "eq"),
    (5, 4, "rs", 4099, 67, 2, "tail"),
    (16, 4, "rs", 32, 67, 8, "eq"),
    (16, 4, "rs", 2080, 1, 2, "plus48"),
    (16, 4, "rs", 2080, 67, 4, "mis1"),
    (20, 7, "rs", 4176, 67, 8, "eq"),
    (20, 7, "rs", 31, 1, 4, "plus48"),
    (64, 32, "rs", 2080, 67, 8, "eq"),
    (64, 32, "rs", 4176, 1, 1, "plus48"),
    (64, 32, "rs", 32, 67, 2, "mis1"),
    (10, 4, "cauchy", 2080, 67, 4, "plus48"),
    (10, 4, "cauchy", 4176, 1, 8, "eq"),
    (10, 4, "cauchy", 1, 1, 1, "mis1"),
]


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
