"""Rebuild in place of lists of 9 to 32 rows on the GPU (include/rsgpu.h
rsgpu_rebuild_blocks, rsgpu_set_rebuild_kernel), on the stripes of the rebuild
suite (tests/test_gpu_rebuild.py Stripe): every case runs under the kernel
choices auto, lanes and threaded from the same state, the lost rows filled
with noise, and what each leaves behind is compared as WHOLE allocations with
what the numpy model of the contract (tests/rebuild_model.py) rebuilds.

The threaded kernel jumps to addresses the wide prepare writes, so the FIRST
test runs the prepare alone and compares every address, row pointer and count
with the model's before any other test launches that kernel.

Row lengths: 4207 = two 2 KB tiles, a partial tile of three 32-byte lanes and
a 15-byte tail for the byte passes; 4208 the same with a 16-byte tail and a
pitch that is a multiple of 16 as it is; 32 one lane; 31 none (LANES)."""
import ctypes as C

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
from test_gpu_rebuild import Stripe, same  # noqa: E402
from test_rebuild_wide import (BLIND, BLIND_AND_PARITY, BLIND_SHORT, DEFICIENT, DEFICIENT_FULL, U_RULE,  # noqa: E402
                               custom_matrix, u_accepted)

N = dm.NONE
DT = rsgpu.SCRUB_REPORT_DTYPE
POISON = gf.POISON
KERNELS = ("auto", "lanes", "threaded")


def hooks():
    H = rsgpu.testhooks()
    H.rsgpu_internal_set_rebuild_prepare_only.argtypes = [C.c_void_p, C.c_int]
    H.rsgpu_internal_set_rebuild_group.argtypes = [C.c_void_p, C.c_longlong]
    H.rsgpu_internal_rebuild_wide_layout.argtypes = [C.c_void_p, C.c_void_p]
    H.rsgpu_internal_rebuild_wide_read.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    H.rsgpu_internal_tc_table.argtypes = [C.c_void_p, C.c_void_p]
    return H


@pytest.fixture(scope="module")
def ctx():
    for c in gf.device_context():
        yield c
        H = hooks()
        H.rsgpu_internal_set_rebuild_prepare_only(c.handle, 0)
        H.rsgpu_internal_set_rebuild_group(c.handle, 0)
        c.set_rebuild_kernel("auto")


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def code_matrix(k, e, kind):
    return custom_matrix(k, e) if kind == "custom" else None


def stripe(ctx, k, e, kind, L, B, u, mode):
    c = code_matrix(k, e, kind)
    return Stripe(ctx, k, e, L, B, u, "cauchy" if kind == "custom" else kind, mode, c=c)


def lists_of(k, e, u, kind, seed=7):
    """8 lists of one call: n = 0, n = 1, n = u as a mix, data rows only,
    parity rows only, n == e (or a second mix where u < e), and two malformed
    ones, not ascending and a row past the block.  The custom matrix gets its
    blind-row and rank-deficient lists instead."""
    rng = np.random.default_rng(seed + 1000 * k + u)
    pick = lambda pool, n: sorted(int(r) for r in rng.choice(pool, n, replace=False))  # noqa: E731
    if kind == "custom":
        rows = [[], BLIND, BLIND_AND_PARITY, DEFICIENT, DEFICIENT_FULL, BLIND_SHORT, [3], list(range(20, 32))]
        lost = np.stack([dm.pad(r, u) for r in rows])
    else:
        rows = [[], pick(k + e, 1), pick(k + e, u), pick(k, min(u, k)), [k + p for p in pick(e, u)],
                pick(k + e, e if u == e else u - 1)]
        bad1 = pick(k + e, u)
        bad1[3], bad1[4] = bad1[4], bad1[3]  # not ascending
        bad2 = pick(k + e, u - 1) + [k + e]  # a row past the block
        lost = np.stack([dm.pad(r, u) for r in rows + [bad1, bad2]])
    return lost.astype(np.uint8)


def run(st, kernel, pre, seed):
    """One unchecked call under `kernel` from the state `pre` with fresh noise
    in the lost rows: (reports, record names)."""
    st.src_all.copy_(pre[0])
    st.par_all.copy_(pre[1])
    st.noise(seed)
    st.ctx.set_rebuild_kernel(kernel)
    got = []
    try:
        names = gf.recorded(st.ctx, lambda: got.append(st.rebuild(check=False)))
    finally:
        st.ctx.set_rebuild_kernel("auto")
    return got[0], names


def wide_names(st, kernel):
    """The records of one call with u > 8 (one group of blocks)."""
    vec = st.pitch % 16 == 0 and st.offset == 0
    most = min(st.u, st.e)
    passes = (most + 7) // 8
    if kernel != "lanes" and vec and st.L >= 32:
        return ["k_rebuild_wide_prepare", "k_rs_tc(rebuild)"] + ["k_rebuild_blocks(pass)"] * (passes if st.L % 32 else 0)
    per_pass = 2 if vec and st.L >= 16 and st.L % 16 else 1
    return ["k_rebuild_wide_prepare"] + ["k_rebuild_blocks(pass)"] * (passes * per_pass)


def factors(c, k, lost):
    """The model's k source rows and M[s][o], the factor of source s in the
    o-th row of `lost`: from the definition, the pivots of the model and the
    solution of c[Q][D] X = I."""
    e = c.shape[0]
    d = [r for r in lost if r < k]
    q = rm.greedy_q(c, lost)
    srcl = [r for r in range(k) if r not in d] + [k + p for p in q]
    nd = len(d)
    inv = rm.solve(c[np.ix_(q, d)], np.eye(nd, dtype=np.uint8)) if nd else np.zeros((0, 0), np.uint8)
    m = np.zeros((k, len(lost)), np.uint8)
    for s, r in enumerate(srcl):
        for i in range(nd):
            if r < k:
                x = 0
                for j in range(nd):
                    x ^= int(sm.gf_mul(int(inv[i, j]), int(c[q[j], r])))
            else:
                x = int(inv[i, s - (k - nd)])
            m[s, i] = x
        for o in range(nd, len(lost)):
            p = lost[o] - k
            x = int(c[p, r]) if r < k else 0
            for i in range(nd):
                x ^= int(sm.gf_mul(int(c[p, d[i]]), int(m[s, i])))
            m[s, o] = x
    return srcl, m


TABLE_CASES = [(20, 12, "cauchy", 4207, 12, "tail"), (20, 12, "custom", 4207, 12, "tail"),
               (5, 12, "cauchy", 4208, 9, "plus48"), (64, 32, "rs", 32, 32, "eq"), (20, 12, "rs", 64, 9, "eq"),
               # k > 64: the sources the prepare's lanes write on their second and later trips
               (65, 17, "rs", 4207, 17, "tail"), (129, 12, "cauchy", 4208, 12, "plus48"),
               (218, 32, "rs", 4207, 32, "tail"), (218, 32, "rs", 64, 24, "eq")]


@pytest.mark.parametrize("k,e,kind,L,u,mode", TABLE_CASES, ids=str)
def test_tables_before_the_first_jump(ctx, k, e, kind, L, u, mode):
    """The wide prepare alone (a test hook stops the call after it): every
    handler address is h_tc_table[(slot & 7) * 256 + M[s][o]] with the model's
    M and handler 0 in the padding, every source and destination pointer is
    the address of its row, the counts are n or 0; nothing of a row is
    written."""
    H = hooks()
    st = stripe(ctx, k, e, kind, L, 8, u, mode)
    st.lost = lists_of(k, e, u, kind)
    st.noise(1)
    pre = st.snapshot()
    ctx.set_rebuild_kernel("threaded")
    assert H.rsgpu_internal_set_rebuild_prepare_only(ctx.handle, 1) == 0
    try:
        got = st.rebuild(check=False)
    finally:
        H.rsgpu_internal_set_rebuild_prepare_only(ctx.handle, 0)
        ctx.set_rebuild_kernel("auto")
    st.same_bytes(*pre)
    lay = np.zeros(10, np.int64)
    assert H.rsgpu_internal_rebuild_wide_layout(ctx.handle, lay.ctypes.data) == 0
    blocks, lk, passes, slots, _, _, o_addr, o_srcs, o_dsts, o_count = (int(v) for v in lay)
    most = min(u, e)
    assert (blocks, lk, slots) == (st.B, k, (most + 7) // 8 * 8)
    assert passes == ((most + 7) // 8 if L % 32 else 0)

    def read(off, n, dtype):
        out = np.zeros(n, dtype)
        assert H.rsgpu_internal_rebuild_wide_read(ctx.handle, off, out.ctypes.data, out.nbytes) == 0
        return out

    tc = np.zeros(2048, np.uint64)
    assert H.rsgpu_internal_tc_table(ctx.handle, tc.ctypes.data) == 0
    # 256 handlers per copy, and slots that share a copy share its addresses
    assert tc.min() > 0 and all(len(set(tc[s * 256:(s + 1) * 256].tolist())) == 256 for s in range(8))
    addr = read(o_addr, st.B * k * slots, np.uint64).reshape(st.B, k, slots)
    srcs = read(o_srcs, st.B * k, np.uint64).reshape(st.B, k)
    dsts = read(o_dsts, st.B * slots, np.uint64).reshape(st.B, slots)
    count = read(o_count, st.B, np.int32)

    def row_ptr(b, r):
        if r < k:
            return st.src.data_ptr() + (b * k + r) * st.pitch
        return st.par.data_ptr() + (b * e + r - k) * st.pitch

    ran = 0
    for b in range(st.B):
        lost = dm.list_rows(st.lost[b], k, e)
        ok = bool(lost) and rm.greedy_q(st.c, lost) is not None
        want = (0, dm.BAD_LIST if lost is None else dm.CLEAN if ok or not lost else dm.BAD_MATRIX, -1)
        assert tuple(int(got[b][f]) for f in gf.SCRUB_FIELDS) == want, b
        assert count[b] == (len(lost) if ok else 0), b
        if not ok:
            continue
        ran += 1
        srcl, m = factors(st.c, k, lost)
        n = len(lost)
        assert [int(p) for p in srcs[b]] == [row_ptr(b, r) for r in srcl], b
        assert [int(p) for p in dsts[b, :n]] == [row_ptr(b, r) for r in lost], b
        assert not dsts[b, n:].any(), b
        slot = np.arange(slots)
        coef = np.zeros((k, slots), np.int64)
        coef[:, :n] = m
        assert (addr[b] == tc[(slot[None, :] & 7) * 256 + coef]).all(), b
    assert ran >= 3


# (k, e, kind, len, pitch mode, u)
CASES = [
    (20, 12, "cauchy", 4207, "tail", 12),
    (20, 12, "rs", 4208, "eq", 9),
    (20, 12, "rs", 4207, "mis1", 12),
    (20, 12, "custom", 4207, "tail", 12),
    (5, 12, "cauchy", 4208, "plus48", 9),
    (5, 12, "cauchy", 32, "eq", 12),
    (64, 32, "rs", 4207, "tail", 32),
    (64, 32, "rs", 32, "eq", 17),
    (64, 32, "cauchy", 4208, "plus48", 24),
    (64, 32, "rs", 31, "eq", 16),
    # k > 64
    (65, 17, "rs", 4207, "tail", 17),
    (129, 12, "cauchy", 4208, "plus48", 12),
    (218, 32, "rs", 4207, "tail", 32),
    (218, 32, "rs", 64, "eq", 24),
]


@pytest.mark.parametrize("k,e,kind,L,mode,u", CASES, ids=str)
def test_against_the_model_under_every_kernel(ctx, k, e, kind, L, mode, u):
    """Reports and whole allocations are the model's under auto, lanes and
    threaded; malformed lists, undetermined ones and n = 0 leave their blocks
    as they were (noise included); the records are the chosen kernel's."""
    st = stripe(ctx, k, e, kind, L, 8, u, mode)
    st.lost = lists_of(k, e, u, kind)
    st.noise(1)
    pre, host = st.snapshot(), st.hosts()
    want, es, ep = st.expect(pre, host, check=False)
    statuses = [w[1] for w in want]
    assert statuses.count(dm.BAD_LIST) >= (0 if kind == "custom" else 2) and statuses.count(dm.CLEAN) >= 4
    if kind == "custom":
        assert statuses[3:6] == [dm.BAD_MATRIX] * 3 and statuses[1:3] == [dm.CLEAN] * 2
    first = None
    for kernel in KERNELS:
        got, names = run(st, kernel, pre, seed=1)
        same(got, want)
        st.same_bytes(es, ep)
        assert names == wide_names(st, kernel), kernel
        first = first if first is not None else got.tobytes()
        assert got.tobytes() == first
    # other noise in the lost rows: the rebuilt rows and the reports do not
    # depend on it (a block that is not written keeps whatever it held)
    got, _ = run(st, "auto", pre, seed=2)
    same(got, want)
    vs, vp = st.view(es[st.offset:], k), st.view(ep[st.offset:], e)
    for b, w in enumerate(want):
        if w[1] == dm.BAD_MATRIX:
            for r in dm.list_rows(st.lost[b], k, e):
                (vs[b, r] if r < k else vp[b, r - k])[:L] = st.row(b, r)
    st.same_bytes(es, ep)


def test_two_damaged_survivors(ctx):
    """Inconsistent survivors at (20, 12) Cauchy: the result is the one the
    greedy pivots define, byte for byte, in the threaded body and in the byte
    tail, the same under every kernel."""
    k, e, L, u = 20, 12, 4207, 12
    st = stripe(ctx, k, e, "cauchy", L, 8, u, "tail")
    st.lost = lists_of(k, e, u, "cauchy")
    rng = np.random.default_rng(6)
    for b in range(st.B):
        surv = [r for r in range(k + e) if r not in (dm.list_rows(st.lost[b], k, e) or [])]
        for r, col in zip(rng.choice(surv, 2, replace=False), (int(rng.integers(0, L - 15)), L - 1 - b % 15)):
            st.xor(b, int(r), col, int(rng.integers(1, 256)))
    st.noise(3)
    pre, host = st.snapshot(), st.hosts()
    want, es, ep = st.expect(pre, host, check=False)
    for kernel in KERNELS:
        got, _ = run(st, kernel, pre, seed=3)
        same(got, want)
        st.same_bytes(es, ep)
    assert not torch.equal(st.src_all, st.orig[0])  # the damage went into rebuilt rows


def test_auto_keeps_todays_kernels_up_to_eight(ctx):
    """u <= 8 under AUTO: the records of the narrow path, unchanged; THREADED
    takes the same lists when asked and writes the same bytes."""
    k, e, u = 20, 12, 8
    for L, mode, names in ((4208, "eq", ["k_rebuild_prepare", "k_rebuild_blocks"]),
                           (4207, "tail", ["k_rebuild_prepare", "k_rebuild_blocks", "k_rebuild_blocks(tail)"]),
                           (4207, "mis1", ["k_rebuild_prepare", "k_rebuild_blocks(bytes)"])):
        st = stripe(ctx, k, e, "rs", L, 8, u, mode)
        st.lost = gf.mixed_lists(k, e, u, st.B)
        st.noise(1)
        pre = st.snapshot()
        for kernel in ("auto", "lanes"):
            got, got_names = run(st, kernel, pre, seed=1)
            assert got_names == names, (L, mode, kernel)
            assert (got["status"] == dm.CLEAN).all()
            st.same_bytes(*st.orig)
        got, got_names = run(st, "threaded", pre, seed=2)
        assert (got_names[:2] == ["k_rebuild_wide_prepare", "k_rs_tc(rebuild)"]) == (mode != "mis1")
        assert (got["status"] == dm.CLEAN).all()
        st.same_bytes(*st.orig)


def test_threaded_with_the_check(ctx, orc):
    """u = 7 at (20, 12), one damaged survivor per block, in the threaded body
    or in the byte tail: ONE_ROW, the located row joins the 7 listed ones (8
    outputs) and the block comes back as the original encode, under LANES and
    under THREADED alike."""
    k, e, L, u, B = 20, 12, 4207, 7, 6
    st = stripe(ctx, k, e, "rs", L, B, u, "tail")
    rng = np.random.default_rng(12)
    hit = []
    for b in range(B):
        rows = sorted(int(r) for r in rng.choice(k + e, u if b else 0, replace=False))
        st.lost[b] = dm.pad(rows, u)
        r = int(rng.choice([r for r in range(k + e) if r not in rows]))
        st.xor(b, r, (100 + 37 * b, L - 1 - b)[b % 2], 0x40 + b)
        hit.append(r)
    st.noise(4)
    pre, host = st.snapshot(), st.hosts()
    reports = st.model(orc)
    assert [tuple(r) for r in reports] == [(1, dm.ONE_ROW, r) for r in hit]
    want, es, ep = st.expect(pre, host, check=True, reports=reports)
    for kernel in ("lanes", "threaded"):
        st.src_all.copy_(pre[0])
        st.par_all.copy_(pre[1])
        ctx.set_rebuild_kernel(kernel)
        got = []
        try:
            names = gf.recorded(ctx, lambda: got.append(st.rebuild(check=True)))
        finally:
            ctx.set_rebuild_kernel("auto")
        got = got[0]
        same(got, want)
        st.same_bytes(es, ep)
        st.same_bytes(*st.orig)
        assert ("k_rs_tc(rebuild)" in names) == (kernel == "threaded")
        if kernel == "threaded":
            assert names[-3:] == ["k_rebuild_wide_prepare", "k_rs_tc(rebuild)", "k_rebuild_blocks(pass)"]
        else:
            assert names[-3:] == ["k_rebuild_prepare", "k_rebuild_blocks", "k_rebuild_blocks(tail)"]


@pytest.mark.parametrize("k,e", [(20, 12), (5, 4)], ids=str)
def test_return_codes(ctx, k, e):
    """The rule for u (tests/test_rebuild_wide.py U_RULE) at both codes, every
    u from 0 to 33 besides: accepted calls return 0, refused ones
    RSGPU_ERR_ARG with the report left as it was."""
    st = Stripe(ctx, k, e, 64, 3, 2, "rs", "eq")
    rep = torch.empty(3 * DT.itemsize, dtype=torch.uint8, device=st.dev)
    lost = torch.full((3 * 40,), N, dtype=torch.uint8, device=st.dev)
    L = rsgpu.lib()
    cases = [(u, check) for ee, u, check, _ in U_RULE if ee == e]
    cases += [(u, check) for u in range(0, 34) for check in (False, True)]
    assert (9, False) in cases
    for u, check in cases:
        rep.fill_(POISON)
        rc = L.rsgpu_rebuild_blocks(ctx.handle, k, e, 64, 64, 3, rsgpu._ptr(st.src), rsgpu._ptr(st.par), None, u,
                                    rsgpu._ptr(lost), 1 if check else 0, rsgpu._ptr(rep))
        torch.cuda.synchronize()
        if u_accepted(e, u, check):
            assert rc == 0, (u, check)
            assert (rep.cpu().numpy().view(DT)["status"] == dm.CLEAN).all(), (u, check)
        else:
            assert rc == -1, (u, check)
            assert (rep.cpu().numpy() == POISON).all(), (u, check)
    for ee, u, check, ok in U_RULE:
        assert u_accepted(ee, u, check) == ok
    st.same_bytes(*st.orig)


def test_encoder_rebuild_with_twelve_lost_rows(ctx):
    """GpuEncoder.rebuild(lost, check=False) with a (blocks, 12) array at
    (20, 12): parity rows and a few data rows per block, and an empty list."""
    k, e, B = 20, 12, 3
    enc = rsgpu.GpuEncoder(k, 4096, e, blocks=B, seed=2, ctx=ctx)
    enc.encode_all()
    torch.cuda.synchronize()
    good = enc.src.clone(), enc.par.clone()
    rows = [[], [0, 7, 19] + list(range(k + 3, k + 12)), list(range(k, k + 12))]
    c = sm.rs_matrix(k, e)
    assert all(rm.greedy_q(c, r) is not None for r in rows)
    lost = np.stack([dm.pad(r, 12) for r in rows]).astype(np.uint8)
    for b, rs_ in enumerate(rows):
        for r in rs_:
            (enc.src.view(B, k, enc.pitch)[b, r] if r < k else enc.par.view(B, e, enc.pitch)[b, r - k]).fill_(0xE7)
    assert not torch.equal(enc.src, good[0]) and not torch.equal(enc.par, good[1])
    rep = enc.rebuild(lost, check=False)
    same(rep, [(0, dm.CLEAN, -1)] * 3)
    assert torch.equal(enc.src, good[0]) and torch.equal(enc.par, good[1])
    with pytest.raises(rsgpu.RsGpuError):
        enc.rebuild(lost, check=True)  # with the check u <= 7


def test_more_blocks_than_a_grid_holds(ctx):
    """65535 + 3 blocks of Cauchy (5, 12) at len 32, nine lost rows each (a
    data row and eight parity rows, rotating): two groups, the second of three
    blocks; every block comes back as the original encode."""
    k, e, L, u = 5, 12, 32, 9
    B = 65535 + 3
    st = stripe(ctx, k, e, "cauchy", L, B, u, "eq")
    b = np.arange(B)
    par = np.sort(k + (b[:, None] // k + np.arange(8)[None, :]) % e, axis=1)
    st.lost = np.concatenate([(b % k)[:, None], par], axis=1).astype(np.uint8)
    assert (np.diff(st.lost.astype(int), axis=1) > 0).all()
    view_s, view_p = st.view(st.src, k), st.view(st.par, e)
    for r in range(k + e):  # noise into the lost rows, a row index at a time
        blocks = torch.from_numpy(np.flatnonzero((st.lost == r).any(axis=1))).to(st.dev)
        if r < k:
            view_s[blocks, r, :L] = 0x3D
        else:
            view_p[blocks, r - k, :L] = 0x3D
    torch.cuda.synchronize()
    assert not torch.equal(st.src_all, st.orig[0]) and not torch.equal(st.par_all, st.orig[1])
    got = []
    names = gf.recorded(ctx, lambda: got.append(st.rebuild(check=False)))
    got = got[0]
    assert names == ["k_rebuild_wide_prepare", "k_rs_tc(rebuild)"] * 2
    assert (got["status"] == dm.CLEAN).all() and (got["bad_columns"] == 0).all() and (got["row"] == -1).all()
    st.same_bytes(*st.orig)


@pytest.mark.parametrize("kernel", ["lanes", "threaded"])
def test_groups_of_blocks(ctx, kernel):
    """A test hook caps a group at 3 blocks: 8 blocks of 80 bytes at (20, 12)
    run as three groups, each with its own prepare, and come back whole."""
    k, e, L, u = 20, 12, 80, 12
    H = hooks()
    st = stripe(ctx, k, e, "cauchy", L, 8, u, "eq")
    st.lost = lists_of(k, e, u, "cauchy")
    st.noise(5)
    pre, host = st.snapshot(), st.hosts()
    want, es, ep = st.expect(pre, host, check=False)
    assert H.rsgpu_internal_set_rebuild_group(ctx.handle, 3) == 0
    try:
        got, names = run(st, kernel, pre, seed=5)
    finally:
        H.rsgpu_internal_set_rebuild_group(ctx.handle, 0)
    same(got, want)
    st.same_bytes(es, ep)
    assert names.count("k_rebuild_wide_prepare") == 3
    assert names.count("k_rs_tc(rebuild)") == (3 if kernel == "threaded" else 0)
    assert names == wide_names(st, kernel) * 3


@pytest.mark.parametrize("kernel", ["lanes", "threaded"])
def test_groups_of_blocks_above_64_sources(ctx, kernel):
    """The same cap at (218, 32) with 32 lost rows and a byte tail: every
    group's prepare writes the tables of sources 64..217 at its own offset."""
    k, e, L, u = 218, 32, 4207, 32
    H = hooks()
    st = stripe(ctx, k, e, "rs", L, 8, u, "tail")
    st.lost = lists_of(k, e, u, "rs")
    st.noise(5)
    pre, host = st.snapshot(), st.hosts()
    want, es, ep = st.expect(pre, host, check=False)
    assert [w[1] for w in want].count(dm.CLEAN) >= 4
    assert H.rsgpu_internal_set_rebuild_group(ctx.handle, 3) == 0
    try:
        got, names = run(st, kernel, pre, seed=5)
    finally:
        H.rsgpu_internal_set_rebuild_group(ctx.handle, 0)
    same(got, want)
    st.same_bytes(es, ep)
    assert names == wide_names(st, kernel) * 3
