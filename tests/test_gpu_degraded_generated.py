"""rsgpu_scrub_degraded_blocks under rsgpu_set_degraded_kernel FUSED with the
scrub kernel GENERATED (k_rs_jit_degraded, k_rs_jitw_degraded; include/rsgpu.h):
the stripes, lists and damage of tests/test_gpu_degraded.py (tests/gpu_family.py)
and the checks of tests/test_gpu_degraded_fused.py, on matrices that have no
compiled kernel.  Every report field comes from the numpy model
(tests/degraded_model.py) run on the syndromes of the blocks as read back;
every call must leave sources, parity and lists as they were
(DegradedStripe.scrub), must have run the kernels the case expects and no
encode (the timing records say which), and a second call under "two_pass" must
give the same report bytes.

A tile is 2048 bytes, a lane's share 32: L0 = 3 * 2048 + 5 * 32 gives three
full tiles and one whose last 59 lanes are idle; with two or three tiles per
workgroup the last workgroup also owns tiles past the row end.

More than 64 source rows: tests/test_gpu_family_generated_wide.py."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import degraded_model as dm  # noqa: E402
import gpu_family as gf  # noqa: E402
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402
from test_degraded_generated_api import (BAD_MATRIX_LISTS, FINISHED_LISTS, MATRICES, bad_matrix, pivot_lists,  # noqa: E402
                                         pivot_hits, statuses_of)
from test_gpu_locate import hooks as locate_hooks  # noqa: E402
from test_gpu_rebuild import Stripe as RebuildStripe  # noqa: E402

N = dm.NONE
TILE = 2048
L0 = 3 * TILE + 5 * 32
B0 = 67
GENERATED = "k_rs_jit_degraded"
COMPILED = "k_rs_bs_degraded"
COMPARE = "k_degraded_compare"
ENCODES = ("k_rs_jit(", "k_rs_tc(", "k_rs_bs", "k_dot")
LENGTHS = [32, 2112, 4160, 6144]  # tests/test_gpu_scrub_generated.py
same, mixed_lists, damage = gf.same, gf.mixed_lists, gf.damage


def hooks():
    H = locate_hooks()
    H.rsgpu_internal_set_degraded_group.argtypes = [C.c_void_p, C.c_longlong]
    H.rsgpu_internal_set_jitw_tiles.argtypes = [C.c_void_p, C.c_int]
    H.rsgpu_internal_scrub_scratch_bytes.argtypes = [C.c_void_p]
    H.rsgpu_internal_scrub_scratch_bytes.restype = C.c_longlong
    return H


def set_tiles(ctx, n):
    assert hooks().rsgpu_internal_set_jitw_tiles(ctx.handle, n) == 0


@pytest.fixture(scope="module")
def ctx():
    for c in gf.device_context(reset_scrub_kernel=True):
        c.set_degraded_kernel("fused")
        c.set_scrub_kernel("generated")
        yield c
        c.set_degraded_kernel("auto")
        c.set_scrub_kernel("auto")
        hooks().rsgpu_internal_set_degraded_group(c.handle, 0)
        set_tiles(c, 0)


def records(ctx, call):
    """call()'s result and the names of the timing records it left."""
    out = []
    names = gf.recorded(ctx, lambda: out.append(call()))
    return out[0], set(names)


def ran(names, which):
    """The records of a call that ran the generated kernel, the compiled one,
    or the two passes."""
    assert {"k_degraded_prepare", "k_degraded_finalise"} <= names, names
    compare = any(n.startswith(COMPARE) for n in names)
    assert (GENERATED in names, COMPILED in names, compare) == \
        (which == "generated", which == "compiled", which == "two_pass"), (which, names)
    if which == "generated":  # no encode of any kind
        assert not any(n.startswith(ENCODES) for n in names), names


class Stripe(gf.DegradedStripe):
    ran = "generated"  # the kernel that is expected to serve these blocks

    def syndromes(self):
        """Per block the syndromes (e, L) of the rows as they are on the device."""
        hs, syn = self.host(self.src, self.k), self.host(self.par, self.e).copy()
        for j in range(self.k):  # sm.syndromes, every block at once
            syn ^= sm.gf_mul(self.c[:, j][None, :, None], hs[:, j][:, None, :])
        return syn

    def check(self, locate=True, syn=None):
        """The call against the model, the kernels that ran, and the same bytes
        under "two_pass"; returns the reports and the model's tuples."""
        syn = self.syndromes() if syn is None else syn
        want = [dm.report_syn(self.c, syn[b], self.lost[b], locate) for b in range(self.B)]
        got, names = records(self.ctx, lambda: self.scrub(locate))
        same(got, want)
        ran(names, self.ran)
        self.ctx.set_degraded_kernel("two_pass")
        try:
            again, names = records(self.ctx, lambda: self.scrub(locate))
        finally:
            self.ctx.set_degraded_kernel("fused")
        ran(names, "two_pass")
        assert again.tobytes() == got.tobytes(), "two_pass reports differ"
        return got, want


@pytest.mark.parametrize("kind", ["cauchy", "rs"])
@pytest.mark.parametrize("k,e", MATRICES, ids=str)
def test_every_layout(ctx, k, e, kind):
    """mixed_lists and damage on every layout of the generated kernels, as a
    Cauchy matrix and as gf_gen_rs_matrix passed by the caller; locate on and
    off; then the lost rows do not matter: zeroed and filled with noise, the
    same reports.  The statuses are those the model names on the CPU
    (tests/test_degraded_generated_api.py)."""
    u = min(8, e)
    st = Stripe(ctx, k, e, L0, B0, u, "cauchy", "plus48", c=gf.matrix(k, e, kind))
    st.lost = mixed_lists(k, e, u, B0)
    damage(st)
    st.fill_lost(None)
    syn = st.syndromes()
    got, want = st.check(True, syn)
    assert {w[1] for w in want} == statuses_of(k, e, kind, u), {w[1] for w in want}
    st.check(False, syn)
    st.fill_lost(77)
    again, _ = st.check()
    assert again.tobytes() == got.tobytes(), "the lost rows' contents changed a report"


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k,e", [(10, 4), (13, 20)], ids=str)
def test_lengths(ctx, k, e, L):
    """One live lane; a tile with two live lanes; three tiles, so that with
    two tiles per workgroup the last workgroup owns a tile that does not
    exist; three full tiles.  The first and the last byte carry damage: of one
    survivor, and of two."""
    u, B = 4, 10
    st = Stripe(ctx, k, e, L, B, u, "cauchy", "plus48")
    st.lost = mixed_lists(k, e, u, B)
    for b in range(B):
        surv = [r for r in range(k + e) if r not in (dm.list_rows(st.lost[b], k, e) or [])]
        if b % 3 == 1:
            st.xor(b, surv[b % len(surv)], 0, 0x31 + b)
            st.xor(b, surv[b % len(surv)], L - 1, 0x52 + b)
        elif b % 3 == 2:
            st.xor(b, surv[0], 0, 0x13 + b)
            st.xor(b, surv[-1], L - 1, 0x71 + b)
    torch.cuda.synchronize()
    st.fill_lost(L)
    got, want = st.check()
    assert {dm.CLEAN, dm.ONE_ROW, dm.DAMAGED} <= {w[1] for w in want}
    st.check(False)


@pytest.mark.parametrize("tpw", [1, 2, 3])
@pytest.mark.parametrize("k,e", [(13, 20), (14, 32)], ids=str)
def test_tiles_per_workgroup(ctx, k, e, tpw):
    """One, two and three tiles per workgroup on L0's four tiles: with two and
    three the last workgroup owns tiles past the row end."""
    u, B = 8, B0  # 67 blocks: every kind of damage() occurs
    st = Stripe(ctx, k, e, L0, B, u, "cauchy", "eq")
    st.lost = mixed_lists(k, e, u, B)
    damage(st)
    st.fill_lost(tpw)
    set_tiles(ctx, tpw)
    try:
        _, want = st.check()
    finally:
        set_tiles(ctx, 0)
    assert {dm.CLEAN, dm.ONE_ROW, dm.DAMAGED} <= {w[1] for w in want}


@pytest.mark.parametrize("k,e", [(13, 20), (9, 44)], ids=str)
def test_pivots_across_waves(ctx, k, e):
    """Eight lost data rows; parity rows 0..3 and four data rows; parity rows
    1..7 and one data row: the pivot rows are not the first parity rows and
    lie in one wave or in two.  Per list one block with a byte of a pivot row
    damaged, one with a byte of the last parity row (a rest row, of the last
    wave), one with a byte of a surviving data row."""
    u = 8
    lists = pivot_lists(k)
    st = Stripe(ctx, k, e, L0, 3 * len(lists), u, "cauchy", "eq")
    for b, row, col, x in pivot_hits(k, e, lists):
        st.lost[b] = dm.pad(np.array(lists[b // 3]), u)
        st.xor(b, row, col, x)
    torch.cuda.synchronize()
    st.fill_lost(5)
    got, want = st.check()
    assert [w[:2] for w in want] == [(1, dm.ONE_ROW)] * st.B
    assert [w[2] for w in want] == [row for _, row, _, _ in pivot_hits(k, e, lists)]
    st.check(False)


def test_every_byte_of_a_lane_and_the_edges(ctx):
    """One block per position of a single damaged byte: the 32 offsets of a
    lane, the first and the last lane of the full tile, the last tile's only
    lane; one data row lost.  The model's row, and one bad column, come back."""
    k, e, L, u = 10, 4, 2080, 2
    cols = [7 * 32 + o for o in range(32)] + [3, 31, 2047 - 31, 2047, 2048, 2048 + 13, 2079]
    st = Stripe(ctx, k, e, L, len(cols), u, "cauchy", "eq")
    for b, col in enumerate(cols):
        st.lost[b] = [b % k, N]
        st.xor(b, (b + 5) % (k + e) if (b + 5) % (k + e) != b % k else k + 1, col, 1 + b)
    torch.cuda.synchronize()
    st.fill_lost(9)
    got, want = st.check()
    assert all(w[0] == 1 and w[1] == dm.ONE_ROW for w in want), want


def test_blocks_the_prepare_finishes(ctx):
    """BAD_LIST, UNCHECKED ((5, 4) with four listed rows) and all-NONE blocks
    between running ones, all damaged: the prepare's reports stay, the
    neighbours' are right.  Then BAD_MATRIX: a matrix with two equal columns,
    both listed as lost."""
    k, e, L, u = 5, 4, 4160, 4
    for c, lists in ((gf.matrix(k, e, "cauchy"), FINISHED_LISTS), (bad_matrix(k, e), BAD_MATRIX_LISTS)):
        st = Stripe(ctx, k, e, L, len(lists), u, "cauchy", "plus48", c=c)
        st.lost = np.array(lists, np.uint8)
        for b in range(st.B):
            rows = dm.list_rows(st.lost[b], k, e) or []
            row = next(r for r in range(k + e) if r not in rows)
            st.xor(b, row, (517 * b) % L, 0x11 + b)
        torch.cuda.synchronize()
        st.fill_lost(4)
        got, want = st.check()
        if lists is FINISHED_LISTS:
            assert [w[1] for w in want][1::2] == [dm.BAD_LIST, dm.UNCHECKED, dm.BAD_LIST, dm.UNCHECKED]
            assert all(w[0] == 1 for w in want[0::2]) and want[4][1] == dm.ONE_ROW
        else:
            # block 0: rows 1 (damaged) and 2 have the same column, two rows explain it
            assert [w[1] for w in want] == [dm.DAMAGED, dm.BAD_MATRIX, dm.ONE_ROW, dm.BAD_MATRIX, dm.ONE_ROW]
        st.check(False)


@pytest.mark.parametrize("k,e", [(10, 4), (14, 32)], ids=str)
def test_all_none_is_the_generated_scrub(ctx, k, e):
    """All-NONE lists: the reports equal scrub_blocks' with LOCATE under
    GENERATED byte for byte."""
    st = Stripe(ctx, k, e, L0, B0, 2, "cauchy", "eq")
    damage(st)
    got, names = records(ctx, st.scrub)
    ran(names, "generated")
    assert {int(s) for s in got["status"]} == {dm.CLEAN, dm.ONE_ROW, dm.DAMAGED}
    ref = torch.empty_like(st.rep)
    ref.fill_(0x3C)
    _, names = records(ctx, lambda: ctx.scrub_blocks(k, e, st.L, st.pitch, st.B, st.src, st.par, ref, coef=st.coef,
                                                     locate=True))
    torch.cuda.synchronize()
    assert "k_rs_jit_scrub" in names
    assert ref.cpu().numpy().tobytes() == got.tobytes()


SELECTION = [(16, 4, "rs", L0, "eq", "compiled"), (10, 4, "cauchy", L0, "mis1", "two_pass"),
             (10, 4, "cauchy", 4176, "eq", "two_pass"), (9, 70, "rs", 2080, "eq", "two_pass")]


@pytest.mark.parametrize("k,e,kind,L,mode,which", SELECTION, ids=str)
def test_selection_by_rows(ctx, k, e, kind, L, mode, which):
    """A compiled code without `coef` runs k_rs_bs_degraded, which has
    precedence; rows off the 16-byte alignment, a len that is no multiple of
    32 and e = 70 run TWO_PASS, with the model's reports."""
    u, B = min(8, e), 23
    st = Stripe(ctx, k, e, L, B, u, kind, mode)
    st.ran = which
    st.lost = mixed_lists(k, e, u, B)
    damage(st)
    st.fill_lost(3)
    st.check()


def test_selection_by_settings(ctx):
    """(10, 4) Cauchy: "fused" needs the scrub kernel "generated", and
    "generated" needs "fused": every other pair runs TWO_PASS; the same report
    bytes every time."""
    k, e, u = 10, 4, 4
    st = Stripe(ctx, k, e, L0, B0, u, "cauchy", "eq")
    st.lost = mixed_lists(k, e, u, B0)
    damage(st)
    st.fill_lost(2)
    first, _ = st.check()
    try:
        for degraded, scrub in (("fused", "auto"), ("fused", "two_pass"), ("fused", "fused"), ("two_pass", "generated"),
                                ("auto", "generated")):
            ctx.set_degraded_kernel(degraded)
            ctx.set_scrub_kernel(scrub)
            got, names = records(ctx, st.scrub)
            ran(names, "two_pass")
            assert got.tobytes() == first.tobytes(), (degraded, scrub)
    finally:
        ctx.set_degraded_kernel("fused")
        ctx.set_scrub_kernel("generated")
    assert rsgpu.lib().rsgpu_set_degraded_kernel(ctx.handle, 3) == -1
    _, names = records(ctx, st.scrub)
    ran(names, "generated")  # a refused value changes nothing


@pytest.mark.parametrize("k,e,u", [(10, 4, 3), (14, 32, 7)], ids=str)
def test_checked_rebuild(ctx, k, e, u):
    """rebuild_blocks with the check: reports and every byte of the
    allocations are rebuild_model's; the check ran k_rs_jit_degraded."""
    st = RebuildStripe(ctx, k, e, 2080, B0, u, "cauchy", "eq")
    st.lost = mixed_lists(k, e, u, B0)
    damage(st)
    st.noise(1)
    pre, host = st.snapshot(), st.hosts()
    got, names = records(ctx, lambda: st.rebuild(check=True))
    want, es, ep = st.expect(pre, host, check=True)
    same(got, want)
    assert {dm.CLEAN, dm.ONE_ROW, dm.DAMAGED} <= {w[1] for w in want}
    st.same_bytes(es, ep)
    assert GENERATED in names and not any(n.startswith(COMPARE) for n in names), names


def test_two_matrices_by_turns(ctx):
    """(10, 4) Cauchy and (10, 4) gf_gen_rs_matrix passed by the caller, three
    turns each on one context: the program cache and the per-block tables."""
    k, e, u, B = 10, 4, 4, 23
    sts = []
    for i, kind in enumerate(("cauchy", "rs")):
        st = Stripe(ctx, k, e, L0, B, u, "cauchy", "eq", seed=20 + i, c=gf.matrix(k, e, kind))
        st.lost = mixed_lists(k, e, u, B, seed=7 + i)
        damage(st, seed=3 + i)
        st.fill_lost(40 + i)
        sts.append((st, st.syndromes()))
    seen = [[], []]
    for turn in range(3):
        for i, (st, syn) in enumerate(sts):
            seen[i].append(st.check(True, syn)[0].tobytes())
    assert len(set(seen[0])) == 1 and len(set(seen[1])) == 1 and seen[0][0] != seen[1][0]


def test_groups():
    """A context of its own, so that no earlier two-pass call has grown the
    scrub family's scratch: 67 blocks in groups of 30 are three prepares,
    launches and finalises, the scratch is as large afterwards as before
    (nothing), and the report bytes are those of one group."""
    k, e, u = 10, 4, 4
    H = hooks()
    for c in gf.device_context(reset_scrub_kernel=True):
        c.set_degraded_kernel("fused")
        c.set_scrub_kernel("generated")
        st = Stripe(c, k, e, L0, B0, u, "cauchy", "plus48")
        st.lost = mixed_lists(k, e, u, B0)
        damage(st)
        st.fill_lost(6)
        before = H.rsgpu_internal_scrub_scratch_bytes(c.handle)
        assert H.rsgpu_internal_set_degraded_group(c.handle, 30) == 0
        out = []
        names = gf.recorded(c, lambda: out.append(st.scrub()), blocks=True)
        assert H.rsgpu_internal_scrub_scratch_bytes(c.handle) == before
        assert [n for n, _ in names] == ["k_degraded_prepare", GENERATED, "k_degraded_finalise"] * 3, names
        assert [nb for n, nb in names if n == GENERATED] == [30, 30, 7], names
        assert H.rsgpu_internal_set_degraded_group(c.handle, -1) == -1
        assert H.rsgpu_internal_set_degraded_group(c.handle, 0) == 0
        one, _ = st.check()
        assert out[0].tobytes() == one.tobytes()
