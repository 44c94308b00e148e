"""rsgpu_ec_encode_data_batch on the device (include/rsgpu.h): one call of 14
blocks, each with its own scattered rows and its own length
(tests/ec_batch_cases.py: the geometries, one per layout of the generated
program, the matrices, the lengths and the placement), bit-exact with the
project's oracle under every path -- the program plus the byte kernel, the byte
kernel alone (`threaded`), the program alone (`aligned32`) -- with the statuses
the header states and the write footprint observed over the whole arena
(tests/footprint.py): after a call the arena differs from what it was exactly
in [0, len_b) of the output rows of the blocks of status 0 and in the status
ints; the three tables, the sources, the guards, the bytes behind a row's
length and the rows of a rejected block are as before.  Then the launch
sequence by its timing records, more blocks than a grid takes, the program
cache under alternating matrices, and the wrapper's row_tables.

Every test restores the arena from the host copy first, so the expected bytes
of a case are computed once and shared."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ec_batch_cases as bc  # noqa: E402
import gpu_family as gf  # noqa: E402
import rsgpu  # noqa: E402
from oracle_lib import Oracle  # noqa: E402

CLASSIFY, FAST, BYTES = "classify(ec_batch)", "k_rs_jit(ec_batch)", "k_dot_bytes(ec_batch)"
ALL = list(range(len(bc.LENGTHS)))


@pytest.fixture(scope="module")
def ctx():
    yield from gf.device_context()


@pytest.fixture(scope="module")
def orc():
    return Oracle()


_CACHE = {}


def case(k, rows, kind, orc):
    """(plan with its arena on the device, matrix, tables, host noise, expected
    rows), built once per case and never changed."""
    key = (k, rows, kind)
    if key not in _CACHE:
        p = bc.plan(k, rows)
        if not hasattr(p.lay, "t"):
            p.lay.allocate(torch.device("cuda", 0), seed=1)
        c = bc.matrix(k, rows, kind, orc)
        noise = p.lay.noise(1)
        _CACHE[key] = (p, c, orc.init_tables(k, rows, c), noise, p.expected(c, noise, orc))
    return _CACHE[key]


def run(ctx, p, g, noise, blocks, max_len, lens=None, status=True, aligned32=False):
    """One call on the blocks `blocks` of the plan, their tables at the head of
    the arena's table regions.  Returns the arena before and after (host)."""
    lay = p.lay
    d, c, n = p.tables(lay.t.data_ptr(), blocks, lens)
    before = noise.copy()
    for name, a in (("data_tab", d), ("coding_tab", c), ("len_tab", n)):
        raw = a.reshape(-1).view(np.uint8)
        before[lay[name].start: lay[name].start + raw.size] = raw
    lay.t.copy_(torch.from_numpy(before))
    torch.cuda.synchronize()
    ctx.ec_encode_data_batch(p.k, p.rows, g, len(blocks), lay.ptr("data_tab"), lay.ptr("coding_tab"),
                             lay.ptr("len_tab"), max_len, lay.ptr("status") if status else None, aligned32)
    torch.cuda.synchronize()
    return before, lay.snapshot()


def check(p, want, before, after, blocks, statuses, lens=None, status=True):
    """The footprint over the whole arena, the statuses, the bytes."""
    lay = p.lay
    ok = [i for i, s in enumerate(statuses) if s == 0]
    allowed = p.written([blocks[i] for i in ok], None if lens is None else [lens[i] for i in ok])
    if status:
        allowed += lay["status"].head(4 * len(blocks))
    lay.check(before, after, allowed)
    if status:
        got = after[lay["status"].start: lay["status"].start + 4 * len(blocks)].view(np.int32)
        assert got.tolist() == list(statuses)
    for i in ok:
        b = blocks[i]
        n = p.lens[b] if lens is None else lens[i]
        for r, name in enumerate(p.out[b]):
            if n:
                got = after[lay[name].start: lay[name].start + n]
                bad = np.nonzero(got != want[(b, r)][:n])[0]
                assert bad.size == 0, (b, r, n, int(bad[0]), int(bad.size))


@pytest.mark.parametrize("max_len", bc.MAX_LENS)
@pytest.mark.parametrize("k,rows,kind", bc.CASES, ids=str)
def test_exact_with_its_footprint(ctx, orc, k, rows, kind, max_len):
    p, c, g, noise, want = case(k, rows, kind, orc)
    ctx.set_encode_kernel("auto")
    before, after = run(ctx, p, g, noise, ALL, max_len)
    check(p, want, before, after, ALL, [0] * len(ALL))


@pytest.mark.parametrize("k,rows,kind", bc.CASES, ids=str)
def test_exact_through_the_byte_kernel_alone(ctx, orc, k, rows, kind):
    p, c, g, noise, want = case(k, rows, kind, orc)
    ctx.set_encode_kernel("threaded")
    try:
        before, after = run(ctx, p, g, noise, ALL, bc.MAX_LENS[0])
    finally:
        ctx.set_encode_kernel("auto")
    check(p, want, before, after, ALL, [0] * len(ALL))


@pytest.mark.parametrize("threaded", (False, True), ids=("auto", "threaded"))
@pytest.mark.parametrize("k,rows,kind", bc.CASES, ids=str)
def test_aligned32(ctx, orc, k, rows, kind, threaded):
    """The blocks that keep the promise, then one that breaks it by its length
    and one by a pointer: those two get -2 and are not touched."""
    p, c, g, noise, want = case(k, rows, kind, orc)
    blocks = list(bc.ALIGNED32_KEEP + bc.ALIGNED32_BREAK)
    statuses = [0] * len(bc.ALIGNED32_KEEP) + [-2, -2]
    ctx.set_encode_kernel("threaded" if threaded else "auto")
    try:
        before, after = run(ctx, p, g, noise, blocks, bc.MAX_LENS[0], aligned32=True)
    finally:
        ctx.set_encode_kernel("auto")
    check(p, want, before, after, blocks, statuses)


@pytest.mark.parametrize("status", (True, False), ids=("status", "no status"))
@pytest.mark.parametrize("k,rows,kind", [(4, 2, "rs"), (9, 22, "rs"), (5, 64, "rs"), (3, 70, "cauchy")], ids=str)
def test_rejected_lengths(ctx, orc, k, rows, kind, status):
    """A length above max_len and a negative one: -2, the block's rows byte for
    byte as before; the other blocks as ever.  Without d_status the same."""
    p, c, g, noise, want = case(k, rows, kind, orc)
    max_len = bc.MAX_LENS[0]
    lens = list(p.lens)
    lens[7], lens[10] = max_len + 1, -1
    statuses = [-2 if b in (7, 10) else 0 for b in ALL]
    before, after = run(ctx, p, g, noise, ALL, max_len, lens=lens, status=status)
    check(p, want, before, after, ALL, statuses, lens=lens, status=status)


@pytest.mark.parametrize("k,rows", bc.GEOMS, ids=str)
def test_launch_sequence(ctx, orc, k, rows):
    kind = next(kd for kk, rr, kd in bc.CASES if (kk, rr) == (k, rows))
    p, c, g, noise, want = case(k, rows, kind, orc)
    call = lambda **kw: gf.recorded(ctx, lambda: run(ctx, p, g, noise, kw.pop("blocks", ALL), bc.MAX_LENS[0], **kw))  # noqa: E731
    fast = [FAST] * bc.passes_of(rows)
    assert len(fast) == (2 if rows == 70 else 1)
    assert call() == [CLASSIFY] + fast + [BYTES]
    assert call(aligned32=True, blocks=list(bc.ALIGNED32_KEEP)) == [CLASSIFY] + fast
    ctx.set_encode_kernel("threaded")
    try:
        assert call() == [CLASSIFY, BYTES]
        assert call(aligned32=True, blocks=list(bc.ALIGNED32_KEEP)) == [CLASSIFY, BYTES]
    finally:
        ctx.set_encode_kernel("auto")


def test_nothing_to_do_enqueues_at_most_the_status_fill(ctx, orc):
    p, c, g, noise, want = case(4, 2, "rs", orc)
    lay = p.lay
    for rows, blocks, max_len, names in ((2, 0, 64, []), (0, 14, 64, [CLASSIFY]), (2, 14, 0, [CLASSIFY])):
        def call():
            ctx.ec_encode_data_batch(4, rows, g, blocks, lay.ptr("data_tab"), lay.ptr("coding_tab"),
                                     lay.ptr("len_tab"), max_len, lay.ptr("status"))
            torch.cuda.synchronize()
        run(ctx, p, g, noise, ALL, bc.MAX_LENS[0])  # tables in place
        before = lay.snapshot()
        assert gf.recorded(ctx, call) == names
        after = lay.snapshot()
        lay.check(before, after, lay["status"].head(4 * blocks))
        if blocks:
            got = after[lay["status"].start: lay["status"].start + 4 * blocks].view(np.int32).tolist()
            assert got == [0 if n <= max_len else -2 for n in bc.LENGTHS]


def test_more_blocks_than_a_grid_takes(ctx, orc):
    """65536 + 3 blocks of (2, 1), lengths cycling 32, 33, 64, 0: a second
    slice of three blocks.  Every block exact, the status written for all of
    them and no int beyond, no byte behind a row's length."""
    B, P = 65536 + 3, 64
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    c = np.array([[0x53, 0xCA]], np.uint8)
    g = orc.init_tables(2, 1, c)
    lens = np.tile(np.array([32, 33, 64, 0], np.int32), B // 4 + 1)[:B]
    h_src = rng.integers(0, 256, (B, 2, P), dtype=np.uint8)
    h_out = rng.integers(0, 256, (B, P), dtype=np.uint8)
    src, out = torch.from_numpy(h_src).to(dev), torch.from_numpy(h_out).to(dev)
    status = torch.full((B + 16,), 77, dtype=torch.int32, device=dev)
    d = src.data_ptr() + (np.arange(B * 2, dtype=np.int64) * P).reshape(B, 2)
    o = out.data_ptr() + (np.arange(B, dtype=np.int64) * P).reshape(B, 1)
    d_data, d_coding = torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev)
    d_len = torch.from_numpy(lens).to(dev)
    names = gf.recorded(ctx, lambda: ctx.ec_encode_data_batch(2, 1, g, B, d_data, d_coding, d_len, 64, status), True)
    torch.cuda.synchronize()
    assert names == [(CLASSIFY, 65535), (FAST, 65535), (BYTES, 65535), (CLASSIFY, 4), (FAST, 4), (BYTES, 4)]
    st = status.cpu().numpy()
    assert not st[:B].any() and (st[B:] == 77).all()
    # the oracle once, over the blocks' rows end to end (one matrix for all)
    full = [np.zeros(B * P, np.uint8)]
    orc.encode_data(B * P, 2, 1, g, [np.ascontiguousarray(h_src[:, j]).reshape(-1) for j in range(2)], full)
    inside = np.arange(P)[None, :] < lens[:, None]
    want = np.where(inside, full[0].reshape(B, P), h_out)
    got = out.cpu().numpy()
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (int(bad[0]), int(bad.size))
    assert (src.cpu().numpy() == h_src).all()
    assert (d_data.cpu().numpy() == d).all() and (d_coding.cpu().numpy() == o).all()
    assert (d_len.cpu().numpy() == lens).all()


def test_two_matrices_alternate(ctx, orc):
    """The program cache: six calls, two matrices by turns, on the same rows."""
    a, b = case(13, 16, "cauchy", orc), case(13, 16, "random", orc)
    assert a[0] is b[0] and (a[1] != b[1]).any()
    for i in range(6):
        p, c, g, noise, want = (a, b)[i % 2]
        before, after = run(ctx, p, g, noise, ALL, bc.MAX_LENS[0])
        check(p, want, before, after, ALL, [0] * len(ALL))


def test_row_tables_of_tensor_views(ctx, orc):
    """rsgpu.row_tables on views of one buffer: tables the call accepts."""
    k, rows, dev = 4, 2, torch.device("cuda", 0)
    c = bc.matrix(k, rows, "rs", orc)
    g = orc.init_tables(k, rows, c)
    lens = [4096, 100, 0, 2080]
    rng = np.random.default_rng(2)
    h = rng.integers(0, 256, 64 * 4352, dtype=np.uint8)
    buf = torch.from_numpy(h).to(dev)
    slot = iter(range(64))
    view = lambda n, off=0: buf[next(slot) * 4352 + off:][:n]  # noqa: E731
    data = [[view(n, 1 if b == 1 and j == 2 else 0) for j in range(k)] for b, n in enumerate(lens)]
    coding = [[view(n) for _ in range(rows)] for n in lens]
    d_data, d_coding, d_len, max_len = rsgpu.row_tables(data, coding, dev)
    assert max_len == 4096 and d_data.shape == (4, k) and d_coding.shape == (4, rows)
    assert d_len.dtype == torch.int32 and d_data.dtype == torch.int64 and d_len.tolist() == lens
    status = torch.full((4,), 9, dtype=torch.int32, device=dev)
    h_data = [[t.cpu().numpy() for t in blk] for blk in data]
    ctx.ec_encode_data_batch(k, rows, g, 4, d_data, d_coding, d_len, max_len, status)
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, 0, 0]
    for b, n in enumerate(lens):
        want = [np.zeros(n, np.uint8) for _ in range(rows)]
        if n:
            orc.encode_data(n, k, rows, g, [np.ascontiguousarray(x) for x in h_data[b]], want)
        for r in range(rows):
            assert (coding[b][r].cpu().numpy() == want[r]).all(), (b, r)
    with pytest.raises(ValueError):
        rsgpu.row_tables([[buf[:4], buf[8:13]]], [[buf[16:20]]], dev)
