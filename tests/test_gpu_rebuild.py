"""Rebuild in place on the GPU (include/rsgpu.h rsgpu_rebuild_blocks): the
stripes, lists and damage kinds of the degraded scrub (tests/gpu_family.py), the lost rows
overwritten with noise before every call.  What the call must leave behind is
put together on the device from a clone of the state before the call and the
rows the numpy model of the contract (tests/rebuild_model.py) rebuilds from
the blocks as read back, and compared with the WHOLE allocations: padding,
survivors and the blocks that must stay untouched are in the same comparison.
Every allocation is filled with 0x6B first."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import degraded_model as dm  # noqa: E402
import gpu_family as gf  # noqa: E402
import rebuild_model as rm  # noqa: E402
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402
from oracle_lib import Oracle  # noqa: E402

N = dm.NONE
DT = rsgpu.SCRUB_REPORT_DTYPE
POISON = gf.POISON


@pytest.fixture(scope="module")
def ctx():
    yield from gf.device_context()


@pytest.fixture(scope="module")
def orc():
    return Oracle()


class Stripe(gf.DegradedStripe):
    """The degraded scrub's stripe with a clone of the original encode."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.orig = self.snapshot()

    def noise(self, seed):
        self.fill_lost(seed)
        torch.cuda.synchronize()

    def hosts(self):
        return self.host(self.src, self.k), self.host(self.par, self.e)

    def rebuild(self, check):
        d_lost = torch.from_numpy(self.lost).to(self.dev)
        self.rep.fill_(POISON)
        self.ctx.rebuild_blocks(self.k, self.e, self.L, self.pitch, self.B, self.src, self.par, self.u, d_lost,
                                self.rep, coef=self.coef, check=check)
        torch.cuda.synchronize()
        assert (d_lost.cpu().numpy() == self.lost).all(), "lists written"
        return self.rep.cpu().numpy().view(DT).copy()

    def original(self):
        """The original encode as (B, k, pitch) and (B, e, pitch) views."""
        return self.view(self.orig[0][self.offset:], self.k), self.view(self.orig[1][self.offset:], self.e)

    def is_original(self, b):
        os_, op = self.original()
        return (torch.equal(self.view(self.src, self.k)[b], os_[b])
                and torch.equal(self.view(self.par, self.e)[b], op[b]))

    def expect(self, pre, host, check, reports=None):
        """What the call leaves of the pre-call state `pre` (clones of the
        allocations; `host` the same blocks on the host): the model's reports
        and the two allocations."""
        hs, hp = host
        es, ep = pre[0].clone(), pre[1].clone()
        vs = self.view(es[self.offset:], self.k)
        vp = self.view(ep[self.offset:], self.e)
        want = []
        for b in range(self.B):
            sb, pb = hs[b], hp[b]
            rep, s2, p2 = rm.call(self.c, sb, pb, self.lost[b], check, None if reports is None else reports[b])
            want.append(rep)
            if s2 is sb:
                continue  # nothing of the block is written
            rows = dm.list_rows(self.lost[b], self.k, self.e) + ([rep[2]] if rep[1] == dm.ONE_ROW else [])
            for r in rows:
                row = torch.from_numpy(np.ascontiguousarray(s2[r] if r < self.k else p2[r - self.k]))
                (vs[b, r] if r < self.k else vp[b, r - self.k])[: self.L] = row.to(self.dev)
        return want, es, ep

    def same_bytes(self, es, ep):
        assert torch.equal(self.src_all, es), "source allocation"
        assert torch.equal(self.par_all, ep), "parity allocation"


same = gf.same


def lists_of(k, e, u, B):
    """mixed_lists; above 64 source or parity rows with the lists around the
    edges of the 64-row bands in blocks 2..5 (gf.wide_lists)."""
    return gf.wide_lists(k, e, u, B) if max(k, e) > 64 else gf.mixed_lists(k, e, u, B)


@pytest.mark.parametrize("k,e,kind,L,B,u,mode", gf.CASES + gf.WIDE_CASES, ids=str)
def test_unchecked_against_the_model(ctx, k, e, kind, L, B, u, mode):
    """Mixed lists, n from 0 to min(u, e), consistent survivors: every block
    is CLEAN, the allocations are what the model says, which is the original
    encode; other noise in the lost rows, the same bytes and reports."""
    st = Stripe(ctx, k, e, L, B, u, kind, mode)
    st.lost = lists_of(k, e, u, B)
    if B > 1:
        ns = {len(dm.list_rows(lst, k, e)) for lst in st.lost}
        assert ns == set(range(min(u, e) + 1))
    st.noise(1)
    pre, host = st.snapshot(), st.hosts()
    got = st.rebuild(check=False)
    want, es, ep = st.expect(pre, host, check=False)
    same(got, want)
    assert all(w == (0, dm.CLEAN, -1) for w in want)
    st.same_bytes(es, ep)
    st.same_bytes(*st.orig)
    st.noise(2)
    again = st.rebuild(check=False)
    assert again.tobytes() == got.tobytes()
    st.same_bytes(*st.orig)


def test_unchecked_with_two_damaged_survivors(ctx):
    """Inconsistent survivors: the result is the one the greedy pivots define,
    byte for byte, in the vector body and in the byte tail."""
    k, e, L, B, u = 16, 4, 2083, 67, 4
    st = Stripe(ctx, k, e, L, B, u, "rs", "tail")
    st.lost = gf.mixed_lists(k, e, u, B)
    rng = np.random.default_rng(6)
    for b in range(B):
        surv = [r for r in range(k + e) if r not in dm.list_rows(st.lost[b], k, e)]
        for r, col in zip(rng.choice(surv, 2, replace=False), (int(rng.integers(0, L - 3)), L - 1 - b % 3)):
            st.xor(b, int(r), col, int(rng.integers(1, 256)))
    st.noise(3)
    pre, host = st.snapshot(), st.hosts()
    got = st.rebuild(check=False)
    want, es, ep = st.expect(pre, host, check=False)
    same(got, want)
    st.same_bytes(es, ep)
    assert not torch.equal(st.src_all, st.orig[0])  # the damage went into rebuilt rows
    st.noise(4)
    assert st.rebuild(check=False).tobytes() == got.tobytes()
    st.same_bytes(es, ep)


def checked(st, orc):
    """One checked call on the stripe as it is, against the models; returns
    the reports."""
    pre, host = st.snapshot(), st.hosts()
    reports = st.model(orc)  # the degraded model on the blocks as they are
    want, es, ep = st.expect(pre, host, check=True, reports=reports)
    got = st.rebuild(check=True)
    same(got, want)
    st.same_bytes(es, ep)
    hs, hp = host
    ohs, ohp = (v[:, :, : st.L].cpu().numpy() for v in st.original())
    for b, w in enumerate(want):
        lost = dm.list_rows(st.lost[b], st.k, st.e)
        if w[1] == dm.CLEAN and lost is not None:
            assert st.is_original(b), b
        elif w[1] == dm.ONE_ROW:
            keep = np.ones(st.k + st.e, bool)
            keep[lost + [w[2]]] = False
            if (np.vstack([hs[b], hp[b]])[keep] == np.vstack([ohs[b], ohp[b]])[keep]).all():
                assert st.is_original(b), b  # the damage lay in the located row alone
    return want, (es, ep)


CHECKED = [(k, e, kind, L, B, min(u, 7), mode) for k, e, kind, L, B, u, mode in gf.CASES + gf.WIDE_CASES]


@pytest.mark.parametrize("k,e,kind,L,B,u,mode", CHECKED, ids=str)
def test_checked_against_the_models(ctx, orc, k, e, kind, L, B, u, mode):
    """Mixed lists and the degraded scrub's damage kinds: the reports are the
    degraded model's (BAD_MATRIX judged on the list as it is rebuilt), CLEAN
    blocks and ONE_ROW blocks come back as the original encode, DAMAGED ones
    keep their bytes, UNCHECKED ones are the model's."""
    wide = max(k, e) > 64
    st = Stripe(ctx, k, e, L, B, u, kind, mode)
    st.lost = lists_of(k, e, u, B)
    one, two = gf.wide_damage(st) if wide else (gf.damage(st), None)
    st.noise(5)
    before = st.snapshot()
    want, after = checked(st, orc)
    if B > 1:
        statuses = {w[1] for w in want}
        assert {dm.CLEAN, dm.ONE_ROW, dm.DAMAGED} <= statuses
        assert (dm.UNCHECKED in statuses) == (u >= e)
    if wide:  # a located row in the second 64-row band or above: it is rebuilt
        assert want[one] == (1, dm.ONE_ROW, gf.wide_row(k, e)) and want[two] == (2, dm.DAMAGED, -1)
        assert any(w[1] == dm.ONE_ROW and w[2] >= (k + 64 if k <= 64 else 64) for w in want)
        assert st.is_original(one)
    # the same input with other noise: the same bytes and reports; a block
    # that is not written keeps the noise in its lost rows, whichever it was
    st.src_all.copy_(before[0])
    st.par_all.copy_(before[1])
    st.noise(6)
    got = st.rebuild(check=True)
    same(got, want)
    vs, vp = st.view(after[0][st.offset:], k), st.view(after[1][st.offset:], e)
    for b, w in enumerate(want):
        if w[1] in (dm.DAMAGED, dm.BAD_MATRIX):
            for r in dm.list_rows(st.lost[b], k, e):
                (vs[b, r] if r < k else vp[b, r - k])[:L] = st.row(b, r)
    st.same_bytes(*after)


LISTS = [[3, 3, N, N, N], [4, 2, N, N, N], [12, N, N, N, N], [N, 2, N, N, N], [0, N, 1, N, N],
         [0, 1, 2, 3, 4], [0, 1, 2, 200, N],
         [0, 1, 2, 3, N], [8, 9, 10, 11, N], [0, 3, 9, 11, N],
         [1, 4, N, N, N], [1, 4, N, N, N], [1, 4, 8, N, N], [1, 4, N, N, N],
         [2, 5, N, N, N], [2, 5, 9, N, N], [2, N, N, N, N], [5, 11, N, N, N],
         [N, N, N, N, N], [11, N, N, N, N], [0, N, N, N, N],
         [2, 5, 8, 9, N], [2, 5, 6, 7, N], [1, 4, 8, 9, N]]


@pytest.mark.parametrize("check", [False, True])
def test_lists_and_matrices(ctx, orc, check):
    """Every malformation, n > e, n == e, a first parity row that is zero on D
    (the pivots skip it) and a rank-deficient matrix, also with n == e, in one
    batch of a caller's matrix."""
    k, e, L, u = 8, 4, 100, 5
    c = sm.cauchy_matrix(k, e).copy()
    c[:, 5] = sm.gf_mul(c[:, 2], 0x35)  # columns 2 and 5 proportional
    c[0, 1] = c[0, 4] = 0               # parity row 0 blind to rows 1 and 4
    st = Stripe(ctx, k, e, L, len(LISTS), u, "cauchy", "eq", c=c)
    st.lost = np.array(LISTS, np.uint8)
    if check:
        st.xor(0, 6, 5, 0x11)    # BAD_LIST: not looked at
        st.xor(7, 6, 5, 0x11)    # UNCHECKED: rebuilt on trust, the damage goes in
        st.xor(11, 6, 50, 0x40)  # rows 1, 4 lost: pivots are parity rows 1, 2
        st.xor(12, k + 1, 99, 0x01)
        st.xor(13, k + 0, 0, 0x80)
        st.xor(14, 6, 5, 0x11)   # BAD_MATRIX
        st.xor(16, 7, 7, 0x07)
        st.xor(18, 0, 0, 0x01)
    st.noise(8)
    if check:
        want, _ = checked(st, orc)
    else:
        pre, host = st.snapshot(), st.hosts()
        got = st.rebuild(check=False)
        want, es, ep = st.expect(pre, host, check=False)
        same(got, want)
        st.same_bytes(es, ep)
        assert [w[1] for w in want[7:14]] == [dm.CLEAN] * 7
    assert [w[1] for w in want[:7]] == [dm.BAD_LIST] * 7
    assert [w[1] for w in want[14:16]] == [dm.BAD_MATRIX] * 2
    assert [w[1] for w in want[21:23]] == [dm.BAD_MATRIX] * 2
    if check:
        assert [w[1] for w in want[7:10]] == [dm.UNCHECKED] * 3 and want[23][1] == dm.UNCHECKED
        assert want[16] == (1, dm.ONE_ROW, 7) and want[10] == (0, dm.CLEAN, -1)
        assert not st.is_original(7) and st.is_original(16) and st.is_original(23)


def test_nothing_to_rebuild(ctx):
    """e == 0 and len == 0: CLEAN for a well-formed list, BAD_LIST otherwise,
    nothing written."""
    for k, e, L in ((6, 0, 64), (5, 4, 0)):
        for check in (False, True):
            st = Stripe(ctx, k, e, L, 4, 4, "rs", "plus48")
            st.lost = np.array([[N, N, N, N], [0, 1, N, N] if e else [N, N, N, N], [1, 0, N, N], [0, 1, 2, 3]],
                               np.uint8)
            want = [(0, dm.CLEAN, -1), (0, dm.CLEAN, -1), (0, dm.BAD_LIST, -1),
                    (0, dm.CLEAN, -1) if e else (0, dm.BAD_LIST, -1)]
            same(st.rebuild(check), want)
            st.same_bytes(*st.orig)


def test_column_stride_loop(ctx):
    """(5, 4), 32816-byte rows, 1024 blocks: 2051 columns on 8 workgroups of
    256 lanes per block, so lanes take a second column.  Against the device
    clone of the encode only."""
    k, e, L, B, u = 5, 4, 32816, 1024, 2
    st = Stripe(ctx, k, e, L, B, u, "rs", "eq")
    rows = np.arange(B)
    st.lost = np.stack([rows % 4, 4 + (rows // 4) % 5], axis=1).astype(np.uint8)
    view_s, view_p = st.view(st.src, k), st.view(st.par, e)
    for r in range(k + e):  # noise into the lost rows, a row index at a time
        for col in range(2):
            blocks = torch.from_numpy(np.flatnonzero(st.lost[:, col] == r)).to(st.dev)
            if r < k:
                view_s[blocks, r, :L] = 0xE7
            else:
                view_p[blocks, r - k, :L] = 0xE7
    torch.cuda.synchronize()
    assert not torch.equal(st.src_all, st.orig[0]) and not torch.equal(st.par_all, st.orig[1])
    got = st.rebuild(check=False)
    assert (got["status"] == dm.CLEAN).all() and (got["bad_columns"] == 0).all() and (got["row"] == -1).all()
    st.same_bytes(*st.orig)


def test_more_blocks_than_a_grid_holds(ctx):
    """65535 + 4 blocks of (5, 4) at len 16 run as two slices; every block
    has a lost row, a survivor is damaged on both sides of the boundary."""
    k, e, L, u = 5, 4, 16, 2
    B = 65535 + 4
    st = Stripe(ctx, k, e, L, B, u, "rs", "eq")
    st.lost[:, 0] = np.arange(B) % (k + e)
    flat_s, flat_p = st.view(st.src, k), st.view(st.par, e)
    for r in range(k + e):
        blocks = torch.from_numpy(np.flatnonzero(st.lost[:, 0] == r)).to(st.dev)
        if r < k:
            flat_s[blocks, r, :L] = 0x3D
        else:
            flat_p[blocks, r - k, :L] = 0x3D
    edge = {0: 3, 65534: 1, 65535: k + 2, 65536: 0, B - 1: 2}
    for b, r in edge.items():
        assert st.lost[b, 0] != r
        st.xor(b, r, b % L, 0x81)
    torch.cuda.synchronize()
    got = st.rebuild(check=True)
    for b, r in edge.items():
        assert (int(got[b]["bad_columns"]), int(got[b]["status"]), int(got[b]["row"])) == (1, dm.ONE_ROW, r), b
    rest = np.ones(B, bool)
    rest[list(edge)] = False
    assert (got["status"][rest] == dm.CLEAN).all() and (got["bad_columns"][rest] == 0).all()
    assert (got["row"][rest] == -1).all()
    st.same_bytes(*st.orig)


def test_on_the_stream(ctx):
    """encode -> damage -> checked rebuild -> scrub with no host
    synchronisation in between: every block CLEAN.  On the same input the
    trusting rebuild seals the damage in: with two spare rows the scrub finds
    both disagreeing (DAMAGED) and does not name the flipped row; with one
    spare row it blames that healthy parity row (the hazard of
    tests/test_degraded.py), where the checked rebuild writes nothing."""
    k, e, L, B, u = 5, 4, 4099, 12, 3
    dev = torch.device("cuda", 0)
    pitch = 4352
    src = torch.empty(B * k * pitch, dtype=torch.uint8, device=dev).fill_(0x6B)
    par = torch.empty(B * e * pitch, dtype=torch.uint8, device=dev).fill_(0x6B)
    rep_rebuild = torch.empty(B * DT.itemsize, dtype=torch.uint8, device=dev)
    rep_scrub = torch.empty_like(rep_rebuild)
    two = np.full((B, u), N, np.uint8)  # two spare rows
    two[0::2, :2] = [0, 4]
    two[1::2, :2] = [1, k + 1]
    one = np.full((B, u), N, np.uint8)  # one spare row
    one[:] = [0, 1, 4]
    noise = torch.randint(0, 256, (L,), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)
    torch.cuda.synchronize()

    def run(check, lost):
        d_lost = torch.from_numpy(lost).to(dev)
        ctx.fill_synthetic(src, B * k, L, pitch, 17, 0)
        ctx.encode_blocks(k, e, L, pitch, B, src, par)
        good = src.clone(), par.clone()
        src.view(B, k, pitch)[:, 3, 10] ^= 0x5A
        for b in range(B):
            for r in dm.list_rows(lost[b], k, e):
                (src.view(B, k, pitch)[b, r] if r < k else par.view(B, e, pitch)[b, r - k])[:L] = noise
        ctx.rebuild_blocks(k, e, L, pitch, B, src, par, u, d_lost, rep_rebuild, check=check)
        ctx.scrub_blocks(k, e, L, pitch, B, src, par, rep_scrub, locate=True)
        torch.cuda.synchronize()
        whole = torch.equal(src, good[0]) and torch.equal(par, good[1])
        return rep_rebuild.cpu().numpy().view(DT).copy(), rep_scrub.cpu().numpy().view(DT).copy(), whole

    first, after, whole = run(True, two)
    assert (first["status"] == dm.ONE_ROW).all() and (first["row"] == 3).all()
    assert (after["status"] == dm.CLEAN).all() and (after["bad_columns"] == 0).all() and whole
    first, after, whole = run(False, two)
    assert (first["status"] == dm.CLEAN).all() and not whole
    assert (after["status"] == dm.DAMAGED).all() and (after["bad_columns"] == 1).all()
    first, after, whole = run(False, one)
    assert (after["status"] == dm.ONE_ROW).all() and (after["row"] == k + 3).all() and not whole
    first, after, whole = run(True, one)
    assert (first["status"] == dm.DAMAGED).all() and (first["bad_columns"] == 1).all()


def test_error_returns_leave_the_report_alone(ctx):
    st = Stripe(ctx, 5, 4, 64, 3, 2, "rs", "eq")
    rep = torch.empty(3 * DT.itemsize + 8, dtype=torch.uint8, device=st.dev)
    lists = {u: torch.full((3 * u,), N, dtype=torch.uint8, device=st.dev) for u in (1, 2, 7, 8, 9)}
    L = rsgpu.lib()
    h = ctx.handle

    def call(src=st.src, par=st.par, u=2, lost=None, flags=1, report=rep, pitch=64, blocks=3):
        rep.fill_(POISON)
        rc = L.rsgpu_rebuild_blocks(h, 5, 4, 64, pitch, blocks, rsgpu._ptr(src), rsgpu._ptr(par), None, u,
                                    rsgpu._ptr(lists[max(u, 1)] if lost is None else lost), flags,
                                    rsgpu._ptr(report))
        torch.cuda.synchronize()
        assert (rep.cpu().numpy() == POISON).all() or rc == 0
        return rc

    assert call() == 0 and call(flags=0) == 0 and call(u=7) == 0 and call(u=8, flags=0) == 0
    assert call(u=0) == -1 and call(u=0, flags=0) == -1 and call(u=9) == -1 and call(u=9, flags=0) == -1
    assert call(u=8) == -1  # with the check a located row may join: u <= 7
    assert call(flags=2) == -1 and call(flags=3) == -1
    assert call(src=None) == -1 and call(par=None) == -1 and call(lost=0) == -1 and call(report=None) == -1
    assert call(report=rep[4:]) == -1  # misaligned
    assert call(pitch=63) == -1 and call(blocks=0) == -1
    st.same_bytes(*st.orig)


def test_encoder_rebuild(ctx):
    enc = rsgpu.GpuEncoder(16, 4096, 4, blocks=3, seed=2, ctx=ctx)
    enc.encode_all()
    torch.cuda.synchronize()
    good = enc.src.clone(), enc.par.clone()
    lost = np.array([[N, N], [3, 17], [5, N]], np.uint8)
    enc.src.view(3, 16, enc.pitch)[1, 3].zero_()
    enc.par.view(3, 4, enc.pitch)[1, 1].zero_()
    enc.src.view(3, 16, enc.pitch)[2, 5].zero_()
    enc.src.view(3, 16, enc.pitch)[2, 9, 100] ^= 0x20
    damaged = enc.src.clone(), enc.par.clone()
    rep = enc.rebuild(lost)
    same(rep, [(0, dm.CLEAN, -1), (0, dm.CLEAN, -1), (1, dm.ONE_ROW, 9)])
    assert torch.equal(enc.src, good[0]) and torch.equal(enc.par, good[1])
    enc.src.copy_(damaged[0])
    enc.par.copy_(damaged[1])
    rep = enc.rebuild(lost, check=False)
    same(rep, [(0, dm.CLEAN, -1)] * 3)
    assert torch.equal(enc.src[: 2 * 16 * enc.pitch], good[0][: 2 * 16 * enc.pitch])
    assert not torch.equal(enc.src, good[0])
    with pytest.raises(ValueError):
        enc.rebuild(lost[:2])
