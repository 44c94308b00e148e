"""Partial-stripe update on the GPU (include/rsgpu.h rsgpu_update_blocks):
data and update rows from fill_synthetic, parity from encode_blocks or random.

Every allocation (source, parity, update rows) is filled with 0x6B first, so
the padding is not zero, and cloned whole before the call.  What the call must
leave is the clone patched by the rows of the numpy model of the contract
(tests/update_model.py), compared with torch.equal over the whole allocations:
a byte written in another row, another block, the padding, the update rows or
a block whose list is malformed fails the comparison."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import gpu_family as gf  # noqa: E402
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402
import update_model as um  # noqa: E402

N = um.NONE
CODES = [(5, 4, "rs"), (64, 32, "rs"), (100, 20, "rs"), (9, 40, "rs"), (213, 37, "rs"), (4, 1, "rs"),
         (6, 0, "rs"), (24, 12, "cauchy")]
# a vector body of 256 16-byte columns plus a 3-byte tail
L0 = 4099
STATUS_POISON = 0x5A5A5A5A
SDT = rsgpu.SCRUB_REPORT_DTYPE


@pytest.fixture(scope="module")
def ctx():
    yield from gf.device_context()


class Stripe(gf.DeviceBlocks):
    """B synthetic blocks, their parity and B x u update rows on the device."""

    def __init__(self, ctx, k, e, L, B, u, kind="rs", pitch=None, offset=0, parity="consistent", seed=11):
        super().__init__(ctx, k, e, L, B, pitch or max(256, (L + 255) // 256 * 256), offset, kind, seed=seed,
                         encode=parity == "consistent")
        self.u = u
        self.upd_all = self.alloc(u)
        self.upd = self.upd_all[offset:]
        ctx.fill_synthetic(self.upd, B * u, L, self.pitch, seed + 1000, 0)
        if parity != "consistent" and e > 0 and L > 0:
            g = torch.Generator(device="cpu").manual_seed(seed)
            rnd = torch.randint(0, 256, (B, e, L), dtype=torch.uint8, generator=g)
            self.view(self.par, e)[:, :, :L] = rnd.to(self.dev)
        self.status = torch.empty(B, dtype=torch.int32, device=self.dev)
        self.cols = np.full((B, u), N, np.uint8)
        torch.cuda.synchronize()

    def snapshot(self):
        return super().snapshot() + (self.upd_all.clone(),)

    def expect(self, delta=False):
        """The model on every block as it is now: (statuses, the source and
        parity allocations as the call must leave them)."""
        src, par, _ = self.snapshot()
        sv, pv = self.view(src[self.offset:], self.k), self.view(par[self.offset:], self.e)
        hs, hp, hu = self.host(self.src, self.k), self.host(self.par, self.e), self.host(self.upd, self.u)
        status = []
        for b in range(self.B):
            s2, p2, st = um.update(self.c, hs[b], hp[b], self.cols[b], hu[b], delta=delta)
            status.append(st)
            if st == um.OK and um.list_rows(self.cols[b], self.k):
                sv[b, :, : self.L] = torch.from_numpy(s2).to(self.dev)
                pv[b, :, : self.L] = torch.from_numpy(p2).to(self.dev)
        return status, (src, par)

    def upload_lists(self):
        self.status.fill_(STATUS_POISON)
        self.d_cols = torch.from_numpy(self.cols).to(self.dev)

    def update(self, delta=False, src=True, sync=True, upload=True):
        if upload:
            self.upload_lists()
        self.ctx.update_blocks(self.k, self.e, self.L, self.pitch, self.B, self.u, self.d_cols, self.upd,
                               self.src if src else None, self.par, self.status, coef=self.coef, delta=delta)
        if sync:
            torch.cuda.synchronize()
            return self.status.cpu().numpy().tolist()

    def check(self, delta=False, src=True):
        """One call against the model, whole allocations compared."""
        before = self.snapshot()
        cols_before = self.cols.copy()
        want, after = self.expect(delta)
        got = self.update(delta, src)
        assert got == want
        assert torch.equal(self.src_all, after[0]), "source allocation"
        assert torch.equal(self.par_all, after[1]), "parity allocation"
        assert torch.equal(self.upd_all, before[2]), "update rows"
        assert (self.d_cols.cpu().numpy() == cols_before).all(), "lists"
        return want, before, after

    def scrub(self):
        rep = torch.empty(self.B * SDT.itemsize, dtype=torch.uint8, device=self.dev)
        self.ctx.scrub_blocks(self.k, self.e, self.L, self.pitch, self.B, self.src, self.par, rep, coef=self.coef)
        torch.cuda.synchronize()
        return rep.cpu().numpy().view(SDT)


def mixed_lists(k, u, B, seed=5):
    """Block 0: the first u rows (j = 0 first); 1: the last u (j = k - 1 last);
    2: all NONE; 3: about half a list, NONE-padded; 4 on: u random rows."""
    rng = np.random.default_rng(seed)
    cols = np.full((B, u), N, np.uint8)
    cols[0] = np.arange(u)
    cols[1] = np.arange(k - u, k)
    if B > 3:
        half = max(1, u // 2)
        cols[3] = um.pad(np.sort(rng.choice(k, half, replace=False)), u)
    for b in range(4, B):
        cols[b] = np.sort(rng.choice(k, u, replace=False))
    return cols


def update_counts(k):
    """1, 2, 3, 9 (beyond one in-register group of 8) and k, where the code has the rows."""
    return sorted({u for u in (1, 2, 3, 9, k) if u <= k})


CODE_U = [(k, e, kind, u) for k, e, kind in CODES for u in update_counts(k)]


@pytest.mark.parametrize("parity", ["consistent", "random"])
@pytest.mark.parametrize("k,e,kind,u", CODE_U, ids=str)
def test_codes_and_update_counts(ctx, k, e, kind, u, parity):
    """Every code at every update count: full lists, NONE-padded lists, an
    all-NONE block, j = 0 and j = k - 1, over consistent parity (the result
    then equals the re-encode) and random parity (the XOR contract itself)."""
    st = Stripe(ctx, k, e, L0, 5, u, kind, parity=parity)
    st.cols = mixed_lists(k, u, 5)
    want, before, after = st.check()
    assert want == [0] * 5
    assert not torch.equal(after[0], before[0])
    # block 2 (all NONE) is untouched
    b2 = slice(2 * k * st.pitch, 3 * k * st.pitch)
    assert torch.equal(st.src_all[b2], before[0][b2])
    if parity == "consistent" and e > 0:
        # the model's parity is the re-encode of the new rows: the device's own, too
        par = st.par_all.clone()
        ctx.encode_blocks(k, e, L0, st.pitch, 5, st.src, st.par, coef=st.coef)
        torch.cuda.synchronize()
        assert torch.equal(st.par_all, par)


@pytest.mark.parametrize("delta", [False, True], ids=["new", "delta"])
@pytest.mark.parametrize("layout", ["pitch256", "odd"])
@pytest.mark.parametrize("L", [0, 1, 31, 4099, 4160])
@pytest.mark.parametrize("k,e", [(5, 4), (64, 32)], ids=str)
def test_lengths_and_pitches(ctx, k, e, L, layout, delta):
    """pitch256: 16-byte aligned rows (vector body, byte tail).  odd: an odd
    pitch and rows that start 1 byte past the allocation's alignment (byte
    path).  The kernel's name in the timing log says which path ran."""
    if layout == "pitch256":
        st = Stripe(ctx, k, e, L, 4, 3, parity="random")
    else:
        st = Stripe(ctx, k, e, L, 4, 3, pitch=(L + 3) | 1, offset=1, parity="random")
        assert st.src.data_ptr() % 16 == 1 and st.pitch % 2 == 1
    st.cols = mixed_lists(k, 3, 4)
    ctx.timing_enable(True)
    try:
        want, before, after = st.check(delta=delta)
        names = [n for n, _, _ in ctx.timing_read()]
    finally:
        ctx.timing_enable(False)
    assert want == [0] * 4
    if layout == "pitch256" and L >= 16:
        assert names == ["k_update_blocks"] + (["k_update_blocks(tail)"] if L % 16 else [])
    else:
        assert names == ["k_update_blocks(bytes)"]
    if L == 0:
        assert torch.equal(st.src_all, before[0]) and torch.equal(st.par_all, before[1])
    if delta:
        assert torch.equal(st.src_all, before[0])


@pytest.mark.parametrize("src", ["poisoned", "null"])
def test_delta_mode_leaves_the_sources_alone(ctx, src):
    """RSGPU_UPDATE_DELTA: d_src is neither read (its poison does not reach
    the parity) nor written; it may be NULL."""
    k, e, u = 64, 32, 9
    st = Stripe(ctx, k, e, L0, 4, u, parity="random")
    st.cols = mixed_lists(k, u, 4)
    want, after = st.expect(delta=True)  # from the sources before the poison
    st.src_all.fill_(0xEE)
    poisoned = st.src_all.clone()
    upd = st.upd_all.clone()
    assert st.update(delta=True, src=(src == "poisoned")) == want == [0] * 4
    assert torch.equal(st.src_all, poisoned)
    assert torch.equal(st.par_all, after[1])
    assert torch.equal(st.upd_all, upd)


@pytest.mark.parametrize("delta", [False, True], ids=["new", "delta"])
@pytest.mark.parametrize("k,e", [(5, 4), (64, 32)], ids=str)
def test_malformed_lists_among_good_ones(ctx, k, e, delta):
    st = Stripe(ctx, k, e, L0, 7, 3, parity="random")
    st.cols = np.array([[0, 2, 4],       # good
                        [3, 1, N],       # descending
                        [1, N, N],       # good
                        [2, 2, N],       # duplicate
                        [0, k, N],       # index k
                        [0, N, 3],       # a row after NONE
                        [k - 1, N, N]],  # good
                       np.uint8)
    want, before, after = st.check(delta=delta)
    assert want == [0, -2, 0, -2, -2, -2, 0]
    for b in (1, 3, 4, 5):  # byte-identical
        sb, pb = slice(b * k * st.pitch, (b + 1) * k * st.pitch), slice(b * e * st.pitch, (b + 1) * e * st.pitch)
        assert torch.equal(st.src_all[sb], before[0][sb]) and torch.equal(st.par_all[pb], before[1][pb])
    assert not torch.equal(st.par_all, before[1])


def test_one_block_one_row_equals_the_pointer_form(ctx):
    """rsgpu_ec_encode_data_update on the same bytes (its data row is the delta)."""
    k, e, j = 20, 7, 13
    st = Stripe(ctx, k, e, L0, 1, 1, parity="random")
    st.cols[0, 0] = j
    par0 = st.par_all.clone()
    a = gf.matrix(k, e, "rs")
    g = rsgpu.ec_init_tables(k, e, a)
    delta = st.upd[:L0] ^ st.view(st.src, k)[0, j, :L0]
    other = par0.clone()
    rows = [other[p * st.pitch:] for p in range(e)]
    ctx.ec_encode_data_update(L0, k, e, j, g, delta, rows)
    want, before, after = st.check()
    assert want == [0]
    assert torch.equal(st.par_all, other) and not torch.equal(other, par0)


def test_stream_order_encode_update_scrub(ctx):
    """encode, update, scrub enqueued with no host synchronisation between."""
    k, e, u, B = 64, 32, 9, 5
    st = Stripe(ctx, k, e, 4160, B, u, parity="random")
    st.cols = mixed_lists(k, u, B)
    old = st.src_all.clone()
    rep = torch.empty(B * SDT.itemsize, dtype=torch.uint8, device=st.dev)
    st.upload_lists()
    torch.cuda.synchronize()
    ctx.encode_blocks(k, e, st.L, st.pitch, B, st.src, st.par)
    st.update(sync=False, upload=False)
    ctx.scrub_blocks(k, e, st.L, st.pitch, B, st.src, st.par, rep)
    torch.cuda.synchronize()
    r = rep.cpu().numpy().view(SDT)
    assert (r["status"] == sm.CLEAN).all() and (r["bad_columns"] == 0).all()
    assert st.status.cpu().numpy().tolist() == [0] * B
    assert not torch.equal(st.src_all, old)


@pytest.mark.parametrize("delta", [False, True], ids=["new", "delta"])
def test_encoder_update(ctx, delta):
    enc = rsgpu.GpuEncoder(20, 4096, 7, blocks=3, seed=4, ctx=ctx)
    enc.encode_all()
    cols = np.array([[2, 19], [N, N], [0, N]], np.uint8)
    rows = torch.empty(3 * 2 * enc.pitch, dtype=torch.uint8, device=enc.src.device)
    ctx.fill_synthetic(rows, 3 * 2, 4096, enc.pitch, 99, 0)
    torch.cuda.synchronize()
    src0, par0 = enc.src.clone(), enc.par.clone()
    status = enc.update(cols, rows, delta=delta)
    assert status.tolist() == [0, 0, 0]
    sv, rv = src0.view(3, 20, enc.pitch), rows.view(3, 2, enc.pitch)
    new = src0.clone()
    nv = new.view(3, 20, enc.pitch)
    for b, i, j in ((0, 0, 2), (0, 1, 19), (2, 0, 0)):
        nv[b, j, :4096] = (rv[b, i, :4096] ^ sv[b, j, :4096]) if delta else rv[b, i, :4096]
    if delta:
        # the sources stay; the parity is the one of the rows XORed in
        assert torch.equal(enc.src, src0)
        enc.src.copy_(new)
    assert torch.equal(enc.src, new)
    assert not torch.equal(enc.par, par0)
    assert (enc.scrub()["status"] == sm.CLEAN).all()
    assert enc.update(np.array([[3, 3], [N, N], [N, N]], np.uint8), rows).tolist() == [-2, 0, 0]
    with pytest.raises(ValueError):
        enc.update(cols[:2], rows)


def test_damaged_block_keeps_its_scrub_report(ctx):
    """Block 1 is damaged in row 7 (three columns); an update of other rows,
    and one of the damaged row itself as a delta that the caller also applies
    to the source rows, leave every report as it was."""
    k, e, u, B = 16, 4, 2, 3
    st = Stripe(ctx, k, e, 4160, B, u)
    for col, x in ((0, 0x01), (2049, 0x80), (4159, 0xC3)):
        st.view(st.src, k)[1, 7, col] ^= x
    before = st.scrub()
    assert [(int(r["bad_columns"]), int(r["status"]), int(r["row"])) for r in before] == [
        (0, sm.CLEAN, -1), (3, sm.ONE_ROW, 7), (0, sm.CLEAN, -1)]
    st.cols = np.array([[0, 15], [3, 9], [N, N]], np.uint8)
    st.check()
    assert (st.scrub() == before).all()
    st.cols = np.array([[7, N], [7, 8], [1, 2]], np.uint8)
    st.check(delta=True)
    for b, i, j in ((0, 0, 7), (1, 0, 7), (1, 1, 8), (2, 0, 1), (2, 1, 2)):
        st.view(st.src, k)[b, j, : st.L] ^= st.view(st.upd, u)[b, i, : st.L]
    assert (st.scrub() == before).all()


def test_more_blocks_than_a_grid_holds(ctx):
    """65537 blocks of (2, 1), 16 bytes, one row each: two slices.  The parity
    row of gf_gen_rs_matrix(3, 2) is all ones, so the expected parity is
    par ^ upd ^ old, computed here with torch for the whole batch."""
    k, e, L, B = 2, 1, 16, 65537
    assert (sm.rs_matrix(k, e) == 1).all()
    st = Stripe(ctx, k, e, L, B, 1, pitch=16, parity="random")
    rng = np.random.default_rng(3)
    st.cols = rng.integers(0, 2, (B, 1)).astype(np.uint8)
    st.cols[5, 0] = N
    st.cols[65535, 0] = 1
    st.cols[65536, 0] = 2  # malformed, in the second slice
    src, par, upd = st.snapshot()
    sv, pv, uv = src.view(B, 2, 16), par.view(B, 1, 16), upd.view(B, 1, 16)
    cols = torch.from_numpy(st.cols[:, 0].astype(np.int64)).to(st.dev)
    live = cols < 2
    idx = torch.nonzero(live).flatten()
    old = sv[idx, cols[idx]]
    pv[idx, 0] ^= uv[idx, 0] ^ old
    sv[idx, cols[idx]] = uv[idx, 0]
    got = np.array(st.update())
    want = np.zeros(B, np.int64)
    want[65536] = -2
    assert (got == want).all()
    assert torch.equal(st.src_all, src) and torch.equal(st.par_all, par) and torch.equal(st.upd_all, upd)
    # the last block of the first slice took its row
    assert torch.equal(st.view(st.src, k)[65534, int(st.cols[65534, 0])], st.view(st.upd, 1)[65534, 0])


def test_another_matrix_replaces_the_devices(ctx):
    """The context keeps the last matrix on the device: the same geometry with
    gf_gen_rs_matrix, a Cauchy matrix and gf_gen_rs_matrix again."""
    for kind in ("rs", "cauchy", "rs"):
        st = Stripe(ctx, 24, 12, 1024, 3, 2, kind, parity="random")
        st.cols = mixed_lists(24, 2, 3)
        assert st.check()[0] == [0] * 3


def test_argument_errors_enqueue_nothing(ctx):
    k, e, u, B = 16, 4, 2, 3
    st = Stripe(ctx, k, e, 2048, B, u)
    st.cols = mixed_lists(k, u, B)
    st.status.fill_(STATUS_POISON)
    before = st.snapshot()
    d_cols = torch.from_numpy(st.cols).to(st.dev)
    h, L = ctx._h, rsgpu.lib()
    c, up, s, p, t = d_cols.data_ptr(), st.upd.data_ptr(), st.src.data_ptr(), st.par.data_ptr(), st.status.data_ptr()

    def call(u=u, cols=c, upd=up, src=s, par=p, flags=0, status=t, pitch=st.pitch):
        return L.rsgpu_update_blocks(h, k, e, 2048, pitch, B, u, cols, upd, src, par, None, flags, status)

    assert call(u=0) == -1 and call(u=k + 1) == -1
    assert call(flags=2) == -1 and call(flags=3) == -1
    assert call(cols=None) == -1 and call(status=None) == -1 and call(upd=None) == -1
    assert call(src=None) == -1 and call(par=None) == -1
    assert call(pitch=2047) == -1
    # the update rows inside the sources, and inside the parity
    assert call(upd=s + st.pitch) == -1 and call(upd=p) == -1 and call(upd=p + st.pitch, flags=1) == -1
    torch.cuda.synchronize()
    assert st.status.cpu().numpy().tolist() == [STATUS_POISON] * B
    snap = st.snapshot()
    assert all(torch.equal(x, y) for x, y in zip(snap, before))
    assert call(upd=s + st.pitch, flags=1) == 0  # DELTA: the sources are not part of the call
    torch.cuda.synchronize()
    assert st.status.cpu().numpy().tolist() == [0] * B
    st.status.fill_(STATUS_POISON)
    snap = st.snapshot()
    assert torch.equal(snap[0], before[0]) and not torch.equal(snap[1], before[1])
    assert call(src=None, flags=1) == 0  # and may be NULL
    torch.cuda.synchronize()
    assert st.status.cpu().numpy().tolist() == [0] * B
    with pytest.raises(rsgpu.RsGpuError, match="RSGPU_ERR_ARG"):
        ctx.update_blocks(k, e, 2048, st.pitch, B, u, d_cols, st.upd, None, st.par, st.status)
