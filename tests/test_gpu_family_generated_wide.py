"""The five generated forms of the scrub family at wide k and wide e together
(k_rs_jit_* / k_rs_jitw_* scrub, repair, locate, degraded and correct behind
rsgpu_set_scrub_kernel GENERATED; include/rsgpu.h): more than 64 source rows on
every layout of the generated kernels, up to k + e = 250 and to both sides of
the four-wave 16-row layout's LDS budget (tests/family_wide_cases.py, whose
damage tests/test_family_wide_cases.py checks on the models alone), and a
seeded draw over shapes, matrices, lengths, pitches, tiles per workgroup and
calls.

The blocks and checks are those of the five suites of the generated forms
(tests/test_gpu_scrub_generated.py, _repair_, _locate_, _degraded_ and
_correct_generated.py), with the models run on syndromes that the CPU oracle
computes from the rows read back.  Every call: the reports (and lists) are the
model's; the rows are the model's, the snapshot from before a call that only
reads; the whole allocations, the 0x6B bytes in [len, pitch) included, are
the expected bytes; the timing records name the generated kernel and no
encode (the two passes where the correction's tables do not fit); and the
same call under the two-pass setting gives the same report bytes and rows."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import correct_model as cm  # noqa: E402
import degraded_model as dm  # noqa: E402
import family_wide_cases as fw  # noqa: E402
import gpu_family as gf  # noqa: E402
import locate_model as lm  # noqa: E402
import repair_model as rm  # noqa: E402
import scrub_model as sm  # noqa: E402
import test_gpu_correct as tc  # noqa: E402
import test_gpu_correct_generated as tcg  # noqa: E402
import test_gpu_degraded_generated as tdg  # noqa: E402
import test_gpu_locate_generated as tlg  # noqa: E402
import test_gpu_repair_generated as trg  # noqa: E402
import test_gpu_scrub_generated as tsg  # noqa: E402
from oracle_lib import Oracle  # noqa: E402
from test_gpu_rebuild import Stripe as RebuildStripe  # noqa: E402

N = dm.NONE
MODE = "plus48"  # 48 bytes of 0x6B behind every row


@pytest.fixture(scope="module")
def ctx():
    for c in gf.device_context(reset_scrub_kernel=True):
        yield c
        for setter in (c.set_locate_kernel, c.set_degraded_kernel, c.set_correct_kernel, c.set_repair_kernel):
            setter("auto")
        tlg.set_tiles(c, 0)


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def arm(ctx, form="fused"):
    """The settings under which locate, degraded scrub, checked rebuild and
    correction run their generated form, or their two passes."""
    ctx.set_locate_kernel(form)
    ctx.set_degraded_kernel(form)
    ctx.set_correct_kernel(form)
    ctx.set_scrub_kernel("generated")


def syndromes(blk, orc):
    """(B, e, L): the stored parity of the rows as they are on the device
    XOR the parity the oracle computes from the stored sources."""
    hs, syn = blk.host(blk.src, blk.k), blk.host(blk.par, blk.e).copy()
    g = orc.init_tables(blk.k, blk.e, blk.c)
    for b in range(blk.B):
        calc = [np.zeros(blk.L, np.uint8) for _ in range(blk.e)]
        orc.encode_data(blk.L, blk.k, blk.e, g, [np.ascontiguousarray(r) for r in hs[b]], calc)
        syn[b] ^= np.stack(calc)
    return syn


def plant(blk, plan):
    """[[(row, column, x)]] per block into the rows on the device."""
    for b, hits in enumerate(plan):
        by_row = {}
        for r, col, x in hits:
            by_row.setdefault(r, []).append((col, x))
        for r, cx in by_row.items():
            cols = torch.tensor([c for c, _ in cx], dtype=torch.int64, device=blk.dev)
            assert len(set(cols.tolist())) == len(cx)
            blk.rows(r)[b, cols] ^= torch.tensor([x for _, x in cx], dtype=torch.uint8, device=blk.dev)
    torch.cuda.synchronize()


def patched(blk, fixes):
    """Clones of the allocations with [[(row, column, x)]] per block XORed in."""
    src, par = blk.snapshot()
    sv, pv = blk.view(src[blk.offset:], blk.k), blk.view(par[blk.offset:], blk.e)
    for b, fix in enumerate(fixes):
        for r, col, x in fix:
            (sv[b, r] if r < blk.k else pv[b, r - blk.k])[col] ^= x
    return src, par


def no_encode(names):
    assert not any(n.startswith(tdg.ENCODES) for n in names), names


class Scrub(tsg.Blocks):
    """test_gpu_scrub_generated's blocks; the model on the oracle's syndromes."""
    syn = None

    def model(self, locate=True, c=None):
        return [sm.report(self.c, s, locate) for s in self.syn]


class Repair(trg.Blocks):
    """test_gpu_repair_generated's blocks; the model on the bad columns."""
    orc = None

    def model(self, mode):
        syn = syndromes(self, self.orc)
        hs, hp = self.host(self.src, self.k), self.host(self.par, self.e)
        out = [fw.repair_verdict(self.c, hs[b], hp[b], syn[b], mode) for b in range(self.B)]
        return [w for w, _ in out], patched(self, [fix for _, fix in out])


class Locate(tlg.GenBlocks):
    def check(self, u, syn=None):
        want = super().check(u, syn)
        names = gf.recorded(self.ctx, lambda: self.locate(u))
        assert tlg.GENERATED in names and "k_locate_finish" in names, names
        no_encode(names)
        return want


class Stripe(tdg.Stripe, RebuildStripe):
    """test_gpu_degraded_generated's stripe and check with test_gpu_rebuild's
    clone of the original encode, rebuild and expectation."""

    def checked_rebuild(self, orc):
        """rebuild_blocks with the check on the stripe as it is: reports and
        allocations are the models', the generated kernel checked, a block the
        verdict allows is the original encode again and any other is as it
        was; the two-pass setting then gives the same bytes from the same
        state."""
        pre, host = self.snapshot(), self.hosts()
        syn = syndromes(self, orc)
        reports = [dm.report_syn(self.c, syn[b], self.lost[b]) for b in range(self.B)]
        want, es, ep = self.expect(pre, host, check=True, reports=reports)
        got, names = tdg.records(self.ctx, lambda: self.rebuild(check=True))
        gf.same(got, want)
        self.same_bytes(es, ep)
        assert tdg.GENERATED in names and not any(n.startswith(tdg.COMPARE) for n in names), names
        sv, pv = self.view(pre[0][self.offset:], self.k), self.view(pre[1][self.offset:], self.e)
        for b, w in enumerate(want):
            if w[1] in (dm.DAMAGED, dm.BAD_MATRIX, dm.BAD_LIST):
                assert torch.equal(self.view(self.src, self.k)[b], sv[b]), b
                assert torch.equal(self.view(self.par, self.e)[b], pv[b]), b
        after = self.snapshot()
        self.src_all.copy_(pre[0])
        self.par_all.copy_(pre[1])
        arm(self.ctx, "two_pass")
        try:
            again, names = tdg.records(self.ctx, lambda: self.rebuild(check=True))
        finally:
            arm(self.ctx)
        assert any(n.startswith(tdg.COMPARE) for n in names) and tdg.GENERATED not in names, names
        assert again.tobytes() == got.tobytes()
        self.same_bytes(*after)
        return want


class Correct(tc.Blocks):
    """test_gpu_correct's blocks under a caller's matrix; the model on the bad
    columns of the oracle's syndromes."""

    def __init__(self, ctx, orc, k, e, c, L, mode, B):
        pitch, offset = gf.pitch_of(L, mode)
        gf.DeviceBlocks.__init__(self, ctx, k, e, L, B, pitch, offset, "cauchy", c=c)
        self.orc = orc
        self.rep = torch.empty(B * tc.DT.itemsize, dtype=torch.uint8, device=self.dev)
        torch.cuda.synchronize()
        self.pristine = self.snapshot()

    def model(self, t, blocks=None):
        syn = syndromes(self, self.orc)
        hs, hp = self.host(self.src, self.k), self.host(self.par, self.e)
        out = [fw.correct_verdict(self.c, hs[b], hp[b], syn[b], t) for b in range(self.B)]
        return [w for w, _ in out], patched(self, [fix for _, fix in out])

    def both(self, t, want, after, ran, poison=gf.POISON):
        """The call from the blocks as they are, under "fused" and then from
        the same state under "two_pass": the model's reports and allocations
        and the expected kernels both times, the same report bytes."""
        before = self.snapshot()
        tcg.checked(self, t, want, after, ran=ran, poison=poison)
        rep = self.rep.cpu().numpy().tobytes()
        self.restore(before)
        arm(self.ctx, "two_pass")
        try:
            tcg.checked(self, t, want, after, ran=tcg.COMPARE, poison=poison)
        finally:
            arm(self.ctx)
        assert self.rep.cpu().numpy().tobytes() == rep


def ids(v):
    return "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


SHAPE_L = [(k, e, kind, L) for k, e, kind in fw.SHAPES for L in fw.LENGTHS]
TILES = [(k, e, kind, L, 0) for k, e, kind, L in SHAPE_L] + [(k, e, kind, fw.L0, n) for k, e, kind in fw.TILED for n in (2, 3)]


@pytest.fixture
def tiles(ctx):
    """Sets the tiles per workgroup of the two-wave wide layouts (0: the
    library's choice) for the test's duration."""
    yield lambda n: tlg.set_tiles(ctx, n)
    tlg.set_tiles(ctx, 0)


@pytest.mark.parametrize("k,e,kind,L,tpw", TILES, ids=str)
def test_scrub(ctx, orc, tiles, k, e, kind, L, tpw):
    """band_plan's two rounds, with and without locate: a row of every band
    edge alone in a block is named, blocks of several rows are DAMAGED."""
    tiles(tpw)
    blk = Scrub(ctx, k, e, L, nb=fw.B, c=fw.matrix(k, e, kind))
    pristine = blk.snapshot()
    for rnd in range(fw.ROUNDS):
        rows = fw.band_rows(k, e, rnd)
        plant(blk, fw.band_plan(k, e, L, rnd))
        blk.syn = syndromes(blk, orc)
        want = blk.model()
        assert [w[1:] for w in want] == [(sm.ONE_ROW, r[0]) for r in rows[:fw.SINGLES]] + \
            [(sm.DAMAGED, -1)] * 2 + [(sm.CLEAN, -1)]
        blk.check()
        blk.src_all.copy_(pristine[0])
        blk.par_all.copy_(pristine[1])


@pytest.mark.parametrize("mode", rm.MODES)
@pytest.mark.parametrize("k,e,kind,L", SHAPE_L, ids=str)
def test_repair(ctx, orc, k, e, kind, L, mode):
    """band_plan's two rounds: ONE_ROW repairs the blocks of one row and leaves
    the others byte for byte, COLUMNS brings every block back to the encode."""
    blk = Repair(ctx, k, e, L, nb=fw.B, c=fw.matrix(k, e, kind))
    blk.orc = orc
    pristine = blk.snapshot()
    for rnd in range(fw.ROUNDS):
        rows = fw.band_rows(k, e, rnd)
        plant(blk, fw.band_plan(k, e, L, rnd))
        damaged = blk.snapshot()
        want = blk.check(mode)
        assert [w[2:] for w in want[:fw.SINGLES]] == [(rm.REPAIRED, r[0]) for r in rows[:fw.SINGLES]]
        assert want[-1] == trg.CLEAN
        if mode == "columns":
            assert [w[2:] for w in want[fw.SINGLES:-1]] == [(rm.REPAIRED, -1)] * 2
            assert torch.equal(blk.src_all, pristine[0]) and torch.equal(blk.par_all, pristine[1])
        else:
            assert [w[1:] for w in want[fw.SINGLES:-1]] == [(0, rm.DAMAGED, -1)] * 2
            for t, snap, n in ((blk.src, damaged[0], k), (blk.par, damaged[1], e)):
                for b in (fw.MULTI, fw.OVER):
                    assert torch.equal(blk.view(t, n)[b], blk.view(snap[blk.offset:], n)[b]), "a DAMAGED block was written"
        blk.restore(pristine)


@pytest.mark.parametrize("k,e,kind,L,tpw", TILES, ids=str)
def test_locate(ctx, orc, tiles, k, e, kind, L, tpw):
    """band_plan's two rounds at u = 1, 3 and 8: the lists are the planted
    rows wherever the model lists them (tests/test_family_wide_cases.py: every
    block within min(u, e - 1) rows on a Cauchy matrix)."""
    tiles(tpw)
    arm(ctx)
    st = Locate(ctx, k, e, L, fw.B, gf.pitch_of(L, MODE)[0], c=fw.matrix(k, e, kind))
    pristine = st.snapshot()
    for rnd in range(fw.ROUNDS):
        rows = fw.band_rows(k, e, rnd)
        plant(st, fw.band_plan(k, e, L, rnd))
        syn = list(syndromes(st, orc))
        for u in fw.US:
            want, lists = st.check(u, syn)
            assert want[-1] == (0, lm.CLEAN, -1) and want[fw.OVER][1] == lm.DAMAGED
            if kind == "cauchy":
                for b in range(fw.OVER):
                    if len(rows[b]) <= min(u, e - 1):
                        assert lists[b] == rows[b] + [N] * (u - len(rows[b])), (u, b)
        st.src_all.copy_(pristine[0])
        st.par_all.copy_(pristine[1])


@pytest.mark.parametrize("k,e,kind,L", SHAPE_L, ids=str)
def test_degraded_scrub(ctx, orc, k, e, kind, L):
    """gpu_family.wide_lists and wide_damage: lists around every band edge, a
    block damaged in the last data row, which is named, and one in two rows;
    locate on and off; other bytes in the lost rows, the same reports."""
    arm(ctx)
    st = Stripe(ctx, k, e, L, fw.B, fw.degraded_u(e), "cauchy", MODE, c=fw.matrix(k, e, kind))
    st.lost = gf.wide_lists(k, e, st.u, fw.B)
    one, two = gf.wide_damage(st)
    st.fill_lost(None)
    syn = syndromes(st, orc)
    got, want = st.check(True, syn)
    assert want[one] == (1, dm.ONE_ROW, gf.wide_row(k, e)) and want[two] == (2, dm.DAMAGED, -1)
    st.check(False, syn)
    st.fill_lost(77)
    again, _ = st.check(True, syndromes(st, orc))
    assert again.tobytes() == got.tobytes(), "the lost rows' contents changed a report"


@pytest.mark.parametrize("k,e,kind,L", SHAPE_L, ids=str)
def test_checked_rebuild(ctx, orc, k, e, kind, L):
    """The same lists at u = 7 and the same damage, noise in the lost rows:
    the located row is rebuilt with the listed ones, the block damaged in two
    rows keeps every byte, every other block is the original encode."""
    arm(ctx)
    st = Stripe(ctx, k, e, L, fw.B, fw.degraded_u(e, True), "cauchy", MODE, c=fw.matrix(k, e, kind))
    st.lost = gf.wide_lists(k, e, st.u, fw.B)
    one, two = gf.wide_damage(st)
    st.noise(5)
    want = st.checked_rebuild(orc)
    assert want[one] == (1, dm.ONE_ROW, gf.wide_row(k, e)) and want[two] == (2, dm.DAMAGED, -1)
    assert all(st.is_original(b) == (b != two) for b in range(fw.B)), [st.is_original(b) for b in range(fw.B)]


@pytest.mark.parametrize("k,e,kind,L", SHAPE_L, ids=str)
def test_correct(ctx, orc, k, e, kind, L):
    """correct_plan: t = 2, a second t = 2 call on the result, then t = 1 on
    the damage again.  Where the pair tables do not fit the chunk buffers
    (family_wide_cases.fits), t = 2 runs the two passes and t = 1 the
    generated kernel."""
    arm(ctx)
    blk = Correct(ctx, orc, k, e, fw.matrix(k, e, kind), L, MODE, fw.CORRECT_B)
    plan, pairs = fw.correct_plan(k, e, L)
    plant(blk, plan)
    damaged = blk.snapshot()
    ran = tcg.GENERATED if fw.fits(k, e) else tcg.COMPARE
    want, after = blk.model(2)
    assert want[-1] == tc.CLEAN and want[fw.ONES][1:] == (want[fw.ONES][0], 0, cm.REPAIRED, -1)
    if kind == "cauchy" and L == fw.L0:
        assert want[fw.BANDS] == (len(pairs),) * 3 + (cm.REPAIRED, -1) and want[fw.THREES] == (2, 0, 0, cm.DAMAGED, -1)
        assert all(want[b][2] >= 9 and want[b][3] == cm.PARTIAL for b in fw.PLANNED)
    blk.both(2, want, after, ran)
    want2, after2 = blk.model(2)
    assert all(w[1] == 0 and w[3] in (cm.CLEAN, cm.DAMAGED) for w in want2) and blk.equals(after2)
    blk.both(2, want2, after2, ran, poison=None)
    blk.restore(damaged)
    want1, after1 = blk.model(1)
    assert all(w[2] == 0 for w in want1) and want1[fw.ONES] == want[fw.ONES]
    blk.both(1, want1, after1, tcg.GENERATED)


CASES = fw.draw_cases()


@pytest.mark.parametrize("case", CASES, ids=fw.case_id)
def test_drawn_case(ctx, orc, tiles, case):
    """family_wide_cases.draw: one call on DRAW_B blocks of a drawn shape,
    matrix, length, pitch and tiles per workgroup, damaged in 1 to 3 rows per
    block, with the checks of the planned cases."""
    k, e, L = case.k, case.e, case.L
    c = fw.matrix(k, e, case.kind, case.seed)
    hits = fw.draw_hits(case)
    pitch = gf.pitch_of(L, case.mode)[0]
    tiles(case.tiles)
    arm(ctx)
    if case.call == "scrub":
        blk = Scrub(ctx, k, e, L, nb=fw.DRAW_B, pitch=pitch, c=c)
        plant(blk, hits)
        blk.syn = syndromes(blk, orc)
        blk.check()
    elif case.call == "repair":
        blk = Repair(ctx, k, e, L, nb=fw.DRAW_B, pitch=pitch, c=c)
        blk.orc = orc
        plant(blk, hits)
        blk.check(case.arg)
    elif case.call == "locate":
        st = Locate(ctx, k, e, L, fw.DRAW_B, pitch, c=c)
        plant(st, hits)
        st.check(case.arg, list(syndromes(st, orc)))
    elif case.call == "degraded":
        st = Stripe(ctx, k, e, L, fw.DRAW_B, case.arg, "cauchy", case.mode, c=c)
        st.lost = fw.draw_lists(case)
        plant(st, hits)
        st.noise(case.seed)
        syn = syndromes(st, orc)
        st.check(True, syn)
        st.check(False, syn)
        st.checked_rebuild(orc)
    else:
        blk = Correct(ctx, orc, k, e, c, L, case.mode, fw.DRAW_B)
        plant(blk, hits)
        want, after = blk.model(case.arg)
        blk.both(case.arg, want, after, tcg.GENERATED if fw.fits(k, e, case.arg) else tcg.COMPARE)
