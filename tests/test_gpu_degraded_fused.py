"""rsgpu_scrub_degraded_blocks under rsgpu_set_degraded_kernel FUSED
(k_rs_bs_degraded, include/rsgpu.h): the stripes, lists and damage of
tests/test_gpu_degraded.py (tests/gpu_family.py), the context set to "fused".
Every report field comes from the numpy model (tests/degraded_model.py) run on
the syndromes of the blocks as read back (stored parity ^ the CPU oracle's
encode); every call must leave sources, parity and lists as they were
(DegradedStripe.scrub) and must have run the kernel the case expects, which
the timing records say.

The fused kernel's tile is 2048 bytes, a lane's share 32: len 32 is one lane,
2080 a full tile and a one-lane tile, 4160 two full tiles and two lanes."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import degraded_model as dm  # noqa: E402
import gpu_family as gf  # noqa: E402
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402
from oracle_lib import Oracle  # noqa: E402
from test_gpu_rebuild import Stripe as RebuildStripe  # noqa: E402

N = dm.NONE
CODES = [(16, 4), (16, 8), (64, 32), (64, 16), (100, 20), (5, 4), (20, 7)]
same, mixed_lists, damage = gf.same, gf.mixed_lists, gf.damage


@pytest.fixture(scope="module")
def ctx():
    for c in gf.device_context():
        c.set_degraded_kernel("fused")
        yield c
        c.set_degraded_kernel("auto")


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def records(ctx, call):
    """call()'s result and the names of the timing records it left."""
    out = []
    names = gf.recorded(ctx, lambda: out.append(call()))
    return out[0], set(names)


def ran(names, fused):
    """The records of a call that ran the fused kernel, or the two passes."""
    compare = any(n.startswith("k_degraded_compare") for n in names)
    assert ("k_rs_bs_degraded" in names, compare) == (fused, not fused), names
    assert {"k_degraded_prepare", "k_degraded_finalise"} <= names, names


class Stripe(gf.DegradedStripe):
    fused = True  # the fused kernel is expected to serve these blocks

    def check(self, orc, locate=True):
        """The call against the model and the kernel that ran; the reports."""
        want = self.model(orc, locate)
        got, names = records(self.ctx, lambda: self.scrub(locate))
        same(got, want)
        ran(names, self.fused)
        return got, want


EVERY = [(k, e, 4160, 67, min(8, e), mode) for k, e in CODES for mode in ("eq", "plus48")] + [
    (16, 4, 4160, 67, 1, "eq"), (16, 4, 32, 67, 4, "eq"), (64, 32, 2080, 1, 8, "plus48"), (20, 7, 2080, 67, 7, "eq")]


@pytest.mark.parametrize("k,e,L,B,u,mode", EVERY, ids=str)
def test_every_compiled_code(ctx, orc, k, e, L, B, u, mode):
    """mixed_lists and damage, locate on and off; then the lost rows do not
    matter: zeroed and filled with noise, the same reports."""
    st = Stripe(ctx, k, e, L, B, u, "rs", mode)
    st.lost = mixed_lists(k, e, u, B)
    damage(st)
    st.fill_lost(None)
    got, want = st.check(orc)
    if B > 1 and u > 1:
        statuses = {w[1] for w in want}
        assert {dm.CLEAN, dm.ONE_ROW, dm.DAMAGED} <= statuses
        assert (dm.UNCHECKED in statuses) == (u >= e)
    st.check(orc, locate=False)
    st.fill_lost(77)
    again, _ = st.check(orc)
    assert again.tobytes() == got.tobytes(), "the lost rows' contents changed a report"


@pytest.mark.parametrize("k,e", [(16, 4), (64, 32), (100, 20)], ids=str)
def test_all_none_is_the_scrub(ctx, k, e):
    """All-NONE lists: the reports equal scrub_blocks' with LOCATE byte for byte."""
    st = Stripe(ctx, k, e, 4160, 67, 2, "rs", "eq")
    damage(st)
    got, names = records(ctx, st.scrub)
    ran(names, True)
    assert {int(s) for s in got["status"]} == {dm.CLEAN, dm.ONE_ROW, dm.DAMAGED}
    ref = torch.empty_like(st.rep)
    ref.fill_(0x3C)
    ctx.scrub_blocks(k, e, st.L, st.pitch, st.B, st.src, st.par, ref, coef=None, locate=True)
    torch.cuda.synchronize()
    assert ref.cpu().numpy().tobytes() == got.tobytes()


@pytest.mark.parametrize("k,e", [(100, 20), (16, 8)], ids=str)
def test_pivots_across_waves(ctx, orc, k, e):
    """Eight lost data rows; parity rows 0..3 and four data rows; parity rows
    1..7 and one data row: the pivot rows are not the first parity rows and
    at (100, 20), five rows per wave, lie in two waves.  Per list one block
    with a byte of a pivot row damaged, one with a byte of the last parity row
    (a rest row, of the last wave), one with a byte of a surviving data row."""
    u, L = 8, 4160
    lists = [list(range(2, 10)), [3, 4, 5, 6] + [k + p for p in range(4)], [7] + [k + p for p in range(1, 8)]]
    if e == 8:  # six rows: two spare rows must be left for a row to be named
        lists = [list(range(2, 8)), [3, 4] + [k + p for p in range(4)], [7] + [k + p for p in range(1, 6)]]
    st = Stripe(ctx, k, e, L, 3 * len(lists), u, "rs", "eq")
    for i, rows in enumerate(lists):
        surv_par = [r for r in range(k, k + e) if r not in rows]
        nd = sum(r < k for r in rows)
        for j, row in enumerate((surv_par[nd - 1], k + e - 1, 0)):
            b = 3 * i + j
            st.lost[b] = dm.pad(np.array(rows), u)
            st.xor(b, row, 2048 + 37 * b, 0x40 + b)
    torch.cuda.synchronize()
    st.fill_lost(5)
    got, want = st.check(orc)
    assert all(w[0] == 1 for w in want) and {w[1] for w in want} <= {dm.ONE_ROW, dm.DAMAGED}
    assert sum(w[1] == dm.ONE_ROW for w in want) >= 6
    st.check(orc, locate=False)


def test_every_byte_of_a_lane_and_the_edges(ctx, orc):
    """One block per position of a single damaged byte: the 32 offsets of a
    lane, the first and the last lane of the full tile, the last tile's only
    lane; one data row lost.  The model's row, and one bad column, come back."""
    k, e, L, u = 16, 4, 2080, 2
    cols = [7 * 32 + o for o in range(32)] + [3, 31, 2047 - 31, 2047, 2048, 2048 + 13, 2079]
    st = Stripe(ctx, k, e, L, len(cols), u, "rs", "eq")
    for b, col in enumerate(cols):
        st.lost[b] = [b % k, N]
        st.xor(b, (b + 5) % (k + e) if (b + 5) % (k + e) != b % k else k + 1, col, 1 + b)
    torch.cuda.synchronize()
    st.fill_lost(9)
    got, want = st.check(orc)
    assert all(w[0] == 1 and w[1] == dm.ONE_ROW for w in want), want


def test_blocks_the_prepare_finishes(ctx, orc):
    """BAD_LIST, UNCHECKED ((5, 4) with four listed rows) and all-NONE blocks
    between running ones, all damaged: the prepare's reports stay, the
    neighbours' are right."""
    k, e, L, u = 5, 4, 4160, 4
    lists = [[1, N, N, N], [3, 1, N, N], [0, k + 1, N, N], [0, 1, 2, k + 3], [N, N, N, N], [2, N, 4, N],
             [k + 0, k + 2, N, N], [1, 2, 3, 4], [4, N, N, N]]
    st = Stripe(ctx, k, e, L, len(lists), u, "rs", "plus48")
    st.lost = np.array(lists, np.uint8)
    for b in range(st.B):
        rows = dm.list_rows(st.lost[b], k, e) or []
        row = next(r for r in range(k + e) if r not in rows)
        st.xor(b, row, (517 * b) % L, 0x11 + b)
    torch.cuda.synchronize()
    st.fill_lost(4)
    got, want = st.check(orc)
    assert [w[1] for w in want][1::2] == [dm.BAD_LIST, dm.UNCHECKED, dm.BAD_LIST, dm.UNCHECKED]
    assert all(w[0] == 1 for w in want[0::2]) and want[4][1] == dm.ONE_ROW
    st.check(orc, locate=False)


@pytest.mark.parametrize("k,e,kind,L,mode,own", [(16, 4, "rs", 4160, "eq", True), (16, 4, "rs", 4160, "mis1", False),
                                                 (16, 4, "rs", 4176, "eq", False),
                                                 (10, 4, "cauchy", 4160, "eq", False)], ids=str)
def test_fallbacks(ctx, orc, k, e, kind, L, mode, own):
    """A coef matrix (the built-in one, passed by the caller), rows off the
    16-byte alignment, len % 32 != 0 and a code with no compiled kernel run
    TWO_PASS under "fused", with the model's reports."""
    st = Stripe(ctx, k, e, L, 67, 4, kind, mode, c=sm.rs_matrix(k, e) if own else None)
    st.fused = False
    st.lost = mixed_lists(k, e, 4, 67)
    damage(st)
    st.fill_lost(3)
    st.check(orc)


def test_the_setter(ctx, orc):
    """two_pass and auto launch k_degraded_compare, fused k_rs_bs_degraded;
    back and forth on one context, the same bytes every time."""
    st = Stripe(ctx, 20, 7, 2080, 67, 4, "rs", "eq")
    st.lost = mixed_lists(20, 7, 4, 67)
    damage(st)
    st.fill_lost(2)
    seen = []
    try:
        for kernel in ("two_pass", "fused", "auto", "fused"):
            ctx.set_degraded_kernel(kernel)
            st.fused = kernel == "fused"
            seen.append(st.check(orc)[0].tobytes())
    finally:
        ctx.set_degraded_kernel("fused")
    assert len(set(seen)) == 1
    lib = rsgpu.lib()
    assert lib.rsgpu_set_degraded_kernel(ctx.handle, 3) == -1 and lib.rsgpu_set_degraded_kernel(ctx.handle, -1) == -1
    _, names = records(ctx, st.scrub)
    ran(names, True)  # a refused value changes nothing
    ctx.set_scrub_kernel("two_pass")  # no influence on this call
    try:
        _, names = records(ctx, st.scrub)
    finally:
        ctx.set_scrub_kernel("auto")
    ran(names, True)


@pytest.mark.parametrize("k,e,u", [(64, 32, 7), (20, 7, 4)], ids=str)
def test_checked_rebuild(ctx, k, e, u):
    """rebuild_blocks with the check under "fused": reports and every byte of
    the allocations are rebuild_model's; the check ran k_rs_bs_degraded."""
    st = RebuildStripe(ctx, k, e, 2080, 67, u, "rs", "eq")
    st.lost = mixed_lists(k, e, u, 67)
    damage(st)
    st.noise(1)
    pre, host = st.snapshot(), st.hosts()
    got, names = records(ctx, lambda: st.rebuild(check=True))
    want, es, ep = st.expect(pre, host, check=True)
    same(got, want)
    assert {dm.CLEAN, dm.ONE_ROW, dm.DAMAGED} <= {w[1] for w in want}
    st.same_bytes(es, ep)
    assert "k_rs_bs_degraded" in names and not any(n.startswith("k_degraded_compare") for n in names), names
