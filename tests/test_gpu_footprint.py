"""The write footprint of the hot path (include/rsgpu.h rsgpu_encode_blocks,
rsgpu_decode_blocks, rsgpu_decode_prepare / rsgpu_decode_apply,
rsgpu_decode_general, the ISA-L pointer calls, rsgpu_encode_blocks_host /
rsgpu_decode_blocks_host): every buffer of a call lies in one arena of seeded
noise with guard bands (tests/footprint.py), the whole arena is compared
before and after the call, and only these bytes may differ:
    encode   [0, len) of each parity row
    decode   [0, len) of each of the blocks x e output rows, the first
             *_workspace_bytes() bytes of the workspace, `blocks` ints of the
             status (prepare alone: workspace and status; apply alone: outputs)
Padding in [len, pitch), the guards, the sources, the parity of a decode and
the erasure lists stay as they were.  Every case also asserts what the older
suites assert: the bytes in [0, len) against the oracle (encode) or against
the rows saved before they were overwritten with 0xA5 (decode), and the
record names of the timing log, pinned, so that a case is known to run the
kernel it is named for.

Shapes, the smallest at which a lane mask, a tail or a layout can be wrong.
Aligned (len % 32 == 0): one 32-byte lane, a 2 KB tile less a lane, one tile, a
tile plus a lane, two tiles plus a lane (an odd third tile for the layouts with
two tiles per workgroup), three tiles plus a lane; pitch == len, len + 16, len
+ 48 by turns, so that every kernel meets every len and every pitch mode.
Unaligned (v_perm body + byte tail, or all bytes): len in {1, 7, 8, 15, 16, 17,
33, 4099}, pitch == len, pitch rounded up to 16, buffers one byte past their
alignment.  3 blocks, one case per kernel with 1 block, and one with a
malformed list in block 1 (status -2, its own [0, len) unspecified, everything
else exact)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import footprint as fp  # noqa: E402
import gpu_family as gf  # noqa: E402
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402
from oracle_lib import Oracle  # noqa: E402

B = 3
POISON = 0xA5
ALIGNED_LENS = (32, 2016, 2048, 2080, 4128, 6176)
ALIGNED_MODES = ("eq", "p16", "p48")
UNALIGNED_LENS = (1, 7, 8, 15, 16, 17, 33, 4099)
UNALIGNED_MODES = ("eq", "r16", "mis1")
DECODE_KERNELS = ("auto", "generated", "one_matrix", "general")
ENCODE_KERNELS = ("auto", "compiled", "generated", "threaded", "karatsuba")


def pitch_of(L, mode):
    """(pitch, byte offset of the row buffers past their alignment)."""
    return {"eq": (L, 0), "p16": (L + 16, 0), "p48": (L + 48, 0), "r16": ((L + 15) // 16 * 16, 0),
            "mis1": (L, 1)}[mode]


def vector_rows(L, mode):
    """Rows the kernels may address as 16-byte vectors."""
    pitch, offset = pitch_of(L, mode)
    return pitch % 16 == 0 and offset == 0


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU test needs a HIP device"
    c = rsgpu.Context(0)
    c.set_torch_stream()
    yield c
    torch.cuda.synchronize()
    c.set_decode_kernel("auto")
    c.set_encode_kernel("auto")
    c.close()


@pytest.fixture(scope="module")
def orc():
    return Oracle()


_LAST = {}


def shared(key, make):
    """The case data of `key`, built once and shared by the consecutive cases
    that need it (the kernel choices of one shape); never changed after."""
    if _LAST.get("key") != key:
        _LAST.clear()
        _LAST.update(key=key, val=make())
    return _LAST["val"]


def host_rows(a, r):
    """[blocks, per, len] view of row buffer r in a host copy of the arena."""
    return np.lib.stride_tricks.as_strided(a[r.start:], (r.blocks, r.per, r.length), (r.per * r.pitch, r.pitch, 1))


def hook(name, ctx, n):
    f = getattr(rsgpu.testhooks(), name)
    f.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert f(ctx._h, n) == 0


# ---- decode -----------------------------------------------------------------

SYN, PREP = "k_decode_prepare_syn", "k_decode_prepare"
TC, DOT = "k_rs_tc(decode)", "k_dot_generic(decode)"
# the codes and what each records under `generated`: waves of 8 rows; two waves
# of 10, 12, 16 rows; four waves of 10, 12, 16 rows; passes of <= 64 rows
GENERATED = {
    (5, 4): ["k_jit_emit", "k_rs_jit(decode)"],
    (6, 3): ["k_jit_emit", "k_rs_jit(decode)"],
    (24, 20): ["k_jit10_emit", "k_rs_jit10(decode)"],
    (24, 22): ["k_jit12_emit", "k_rs_jit12(decode)"],
    (30, 28): ["k_jit16_emit", "k_rs_jit16(decode)"],
    (40, 34): ["k_jit10_emit", "k_rs_jit10x4(decode)"],
    (46, 44): ["k_jit12_emit", "k_rs_jit12x4(decode)"],
    (60, 56): ["k_jit16_emit", "k_rs_jit16x4(decode)"],
    (70, 66): ["k_jit10_emit", "k_rs_jitw_passes(decode)", "k_rs_jitw_passes(decode)"],
}
CODES = tuple(GENERATED)
PREPARES = (SYN, PREP, "k_jit_emit", "k_jit10_emit", "k_jit12_emit", "k_jit16_emit")


def decode_names(k, e, kernel, single_launch=True):
    """What a decode of aligned rows records (rsgpu_decode.cpp decode_plan at
    fewer than 16 column tiles per block): generated code; the k x k
    inversion and k_rs_tc in passes of 32 rows under `general` and for e > 32;
    else the closed-form rows and k_rs_tc, which rsgpu_decode_blocks runs as
    one launch for e <= 8 (k_rs_syn_split for the compiled (5, 4) under auto,
    k_rs_tc_fused otherwise)."""
    if kernel == "generated":
        return [SYN] + GENERATED[k, e]
    if kernel == "general" or e > 32:
        return [PREP] + [TC] * ((e + 31) // 32)
    if single_launch and e <= 8:
        return ["k_rs_syn_split(decode)" if kernel == "auto" and (k, e) == (5, 4) else "k_rs_tc_fused(decode)"]
    return [SYN, TC]


class DecodeArena:
    """`blocks` encoded blocks of a k + p row code in one arena, n rows of each
    erased (err: [blocks][n] ascending rows in [0, k + p); drawn among the
    sources when None) and overwritten with 0xA5, the rows as they were in
    `want`.  bad: a block whose list is made malformed (its first entry
    repeated).  pristine: the arena before any decode."""

    def __init__(self, ctx, k, p, L, mode, blocks=B, err=None, coef=None, bad=None, general=False):
        self.k, self.p, self.L, self.blocks, self.bad = k, p, L, blocks, bad
        self.pitch, offset = pitch_of(L, mode)
        if err is None:
            err = rsgpu.erasure_patterns(23, 0, blocks, k, p)
        self.err = np.ascontiguousarray(err, np.uint8).reshape(blocks, -1)
        self.n = n = self.err.shape[1]
        self.ws_bytes = (rsgpu.decode_general_workspace_bytes(k, k + p, n, blocks) if general
                         else rsgpu.decode_workspace_bytes(k, p, blocks))
        ar = self.ar = fp.Arena()
        ar.rows("src", blocks, k, self.pitch, L, offset)
        ar.rows("par", blocks, p, self.pitch, L, offset)
        ar.rows("out", blocks, n, self.pitch, L, offset)
        ar.flat("err", blocks * n)
        ar.flat("workspace", self.ws_bytes)
        ar.flat("status", 4 * blocks)
        ar.allocate(torch.device("cuda", 0), seed=k * 1000 + L)
        ctx.set_encode_kernel("auto")
        ctx.fill_synthetic(ar.ptr("src"), blocks * k, L, self.pitch, 29, 0)
        ctx.encode_blocks(k, p, L, self.pitch, blocks, ar.ptr("src"), ar.ptr("par"), coef=coef)
        rows = torch.cat([ar.view("src"), ar.view("par")], dim=1)
        pick = (torch.arange(blocks, device=rows.device)[:, None],
                torch.from_numpy(self.err.astype(np.int64)).to(rows.device))
        self.want = rows[pick].cpu().numpy()
        rows[pick] = POISON
        ar.view("src")[:] = rows[:, :k]
        ar.view("par")[:] = rows[:, k:]
        lists = self.err.copy()
        if bad is not None:
            lists[bad, 1] = lists[bad, 0]
        ar.buf("err").copy_(torch.from_numpy(lists.reshape(-1)))
        ar.ints("status").fill_(7)
        torch.cuda.synchronize()
        self.pristine = ar.t.clone()
        self.before = ar.snapshot()

    def args(self, nb):
        a = self.ar
        return self.k, self.p, self.L, self.pitch, nb, a.ptr("src"), a.ptr("par")

    def decode(self, ctx, nb):
        a = self.ar
        ctx.decode_blocks(*self.args(nb), a.ptr("err"), a.ptr("out"), a.ptr("workspace"), a.ptr("status"))

    def prepare(self, ctx, nb):
        a = self.ar
        ctx.decode_prepare(*self.args(nb), a.ptr("err"), a.ptr("out"), a.ptr("workspace"), a.ptr("status"))

    def apply(self, ctx, nb):
        a = self.ar
        ctx.decode_apply(*self.args(nb), a.ptr("out"), a.ptr("workspace"), a.ptr("status"))

    def general(self, matrix):
        def call(ctx, nb):
            a = self.ar
            k, p, L, pitch, nb, src, par = self.args(nb)
            ctx.decode_general(k, k + p, L, pitch, nb, matrix, src, par, a.ptr("err"), self.n, a.ptr("out"),
                               a.ptr("workspace"), a.ptr("status"))
        return call

    def run(self, ctx, call, kernel="auto", out=True, prepare=True, restore=True, nb=None):
        """call(ctx, blocks) under decode kernel choice `kernel`, from the
        pristine arena (restore) or from what the call before left; the
        footprint, the statuses and the decoded rows checked.  Returns the
        (name, blocks) records of the timing log."""
        nb = self.blocks if nb is None else nb
        ar = self.ar
        if restore:
            ar.t.copy_(self.pristine)
            torch.cuda.synchronize()
        before = self.before if restore else ar.snapshot()
        ctx.set_decode_kernel(kernel)
        try:
            recs = gf.recorded(ctx, lambda: call(ctx, nb), blocks=True)
        finally:
            ctx.set_decode_kernel("auto")
        torch.cuda.synchronize()
        after = ar.snapshot()
        ar.check(before, after, fp.decode_allowed(ar, self.ws_bytes, nb, out=out, prepare=prepare))
        rows = np.concatenate([host_rows(after, ar["src"]), host_rows(after, ar["par"])], axis=1)
        erased = rows[np.arange(self.blocks)[:, None], self.err.astype(np.int64)]
        assert (erased == POISON).all(), "an erased row no longer holds 0xA5"
        good = [b for b in range(nb) if b != self.bad]
        status = after[ar["status"].start: ar["status"].end].view(np.int32)
        if prepare:
            assert status[:nb].tolist() == [-2 if b == self.bad else 0 for b in range(nb)], status
        if out:
            got = host_rows(after, ar["out"])
            for b in good:
                assert np.array_equal(got[b], self.want[b]), f"decoded rows of block {b} differ"
        return recs


def names(recs):
    return [n for n, _ in recs]


def rotation(kernels, codes, lens, modes):
    """(code, len, mode, kernel): every kernel choice at every code and len,
    the pitch mode rotating so that every (code, kernel) also meets every
    mode; the kernel choices of one (code, len) in a row, on one arena."""
    return [(c, L, modes[(ci + li) % len(modes)], kn) for ci, c in enumerate(codes) for li, L in enumerate(lens)
            for kn in kernels]


def case_id(v):
    return "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


DECODE_ALIGNED = rotation(DECODE_KERNELS, CODES, ALIGNED_LENS, ALIGNED_MODES)


def covers_every_pair(cases, codes, kernels):
    """Every (code, kernel choice) -- so every kernel -- occurs with every len
    and with every pitch mode."""
    seen_len = {(c, kn, L) for c, L, _, kn in cases}
    seen_mode = {(c, kn, m) for c, _, m, kn in cases}
    return all((c, kn, L) in seen_len for c in codes for kn in kernels for L in ALIGNED_LENS) and \
        all((c, kn, m) in seen_mode for c in codes for kn in kernels for m in ALIGNED_MODES)


def test_the_rotation_covers_every_pair():
    assert covers_every_pair(DECODE_ALIGNED, CODES, DECODE_KERNELS)
    assert covers_every_pair(ENCODE_ALIGNED, ENCODE_CODES, ENCODE_KERNELS)
    assert not covers_every_pair(DECODE_ALIGNED[1:], CODES, DECODE_KERNELS)


@pytest.mark.parametrize("code,L,mode,kernel", DECODE_ALIGNED, ids=case_id)
def test_decode_blocks_aligned(ctx, code, L, mode, kernel):
    k, e = code
    d = shared(("dec", code, L, mode), lambda: DecodeArena(ctx, k, e, L, mode))
    assert names(d.run(ctx, d.decode, kernel)) == decode_names(k, e, kernel)


@pytest.mark.parametrize("kernel", DECODE_KERNELS)
@pytest.mark.parametrize("code", CODES, ids=case_id)
def test_decode_blocks_one_block(ctx, code, kernel):
    k, e = code
    d = shared(("dec1", code), lambda: DecodeArena(ctx, k, e, 2080, "p48", blocks=1))
    assert names(d.run(ctx, d.decode, kernel)) == decode_names(k, e, kernel)


@pytest.mark.parametrize("kernel", DECODE_KERNELS)
@pytest.mark.parametrize("code", CODES, ids=case_id)
def test_decode_blocks_malformed_list(ctx, code, kernel):
    """Block 1 has a malformed list: status -2, its own output rows may hold
    anything in [0, len); its padding and every other block are exact."""
    k, e = code
    d = shared(("decbad", code), lambda: DecodeArena(ctx, k, e, 4128, "p16", bad=1))
    assert names(d.run(ctx, d.decode, kernel)) == decode_names(k, e, kernel)


UNALIGNED_CODES = ((5, 4), (6, 3), (24, 20), (70, 66))
DECODE_UNALIGNED = [(c, L, m, DECODE_KERNELS[(ci + li + mi) % 4]) for ci, c in enumerate(UNALIGNED_CODES)
                    for li, L in enumerate(UNALIGNED_LENS) for mi, m in enumerate(UNALIGNED_MODES)]


@pytest.mark.parametrize("code,L,mode,kernel", DECODE_UNALIGNED, ids=case_id)
def test_decode_blocks_unaligned(ctx, code, L, mode, kernel):
    """Every kernel choice runs the v_perm kernel on these shapes: 8-byte
    words and a byte tail (k_dot_generic, k_dot_bytes), or bytes throughout
    where the rows are no 16-byte vectors."""
    k, e = code
    d = DecodeArena(ctx, k, e, L, mode, bad=1 if L == 33 else None)
    assert names(d.run(ctx, d.decode, kernel)) == [PREP, DOT]


@pytest.mark.parametrize("kernel", DECODE_KERNELS)
@pytest.mark.parametrize("code", CODES, ids=case_id)
def test_decode_prepare_then_apply(ctx, code, kernel):
    """The prepare alone may write only the workspace and the status, the
    apply only the outputs."""
    k, e = code
    d = shared(("prep", code), lambda: DecodeArena(ctx, k, e, 2080, "p48", bad=1))
    whole = decode_names(k, e, kernel, single_launch=False)
    prep = names(d.run(ctx, d.prepare, kernel, out=False))
    app = names(d.run(ctx, d.apply, kernel, prepare=False, restore=False))
    assert prep == [n for n in whole if n in PREPARES] and app == [n for n in whole if n not in PREPARES]


def test_decode_fewer_blocks_than_the_buffers_hold(ctx):
    """2 of 3 blocks: the rows, the list and the status of the third stay."""
    d = DecodeArena(ctx, 24, 20, 2080, "p16")
    for kernel in DECODE_KERNELS:
        assert names(d.run(ctx, d.decode, kernel, nb=2)) == decode_names(24, 20, kernel)


GENERAL_JIT = [PREP, "k_jit_emit", "k_rs_jit(decode)"]
# (k, m, [blocks][n] erased rows among data and parity)
GENERAL_CODES = [(6, 9, [[1, 7], [0, 4], [2, 8]]), (10, 16, [[0, 3, 9, 10, 12, 15], [1, 2, 4, 5, 6, 7],
                                                             [10, 11, 12, 13, 14, 15]])]


# the threaded shape, the unaligned shapes (8-byte words and a tail; bytes),
# and the generated general decode from 48 column tiles, at one code
GENERAL_SHAPES = [("threaded", 2080, "p48", [PREP, TC]), ("unaligned", 4099, "r16", [PREP, DOT]),
                  ("bytes", 33, "mis1", [PREP, DOT]), ("generated", 98304, "p48", GENERAL_JIT)]
GENERAL_CASES = [pytest.param(k, m, err, L, mode, want, id=f"{k}-{m}-{name}")
                 for k, m, err in GENERAL_CODES for name, L, mode, want in GENERAL_SHAPES
                 if name != "generated" or k == 6]


@pytest.mark.parametrize("with_matrix", [False, True], ids=["rs", "cauchy"])
@pytest.mark.parametrize("k,m,err,L,mode,want", GENERAL_CASES)
def test_decode_general(ctx, orc, k, m, err, L, mode, want, with_matrix):
    """rsgpu_decode_general with its own workspace size, gf_gen_rs_matrix or a
    caller's Cauchy matrix, erasures among data and parity rows; the parity
    the erased rows are compared with is the oracle's."""
    matrix = rsgpu.gf_gen_cauchy1_matrix(m, k) if with_matrix else None
    coef = None if matrix is None else matrix[k:]
    d = DecodeArena(ctx, k, m - k, L, mode, err=err, coef=coef, general=True)
    a = orc.gen_rs_matrix(m, k)[k:] if matrix is None else coef
    src, par = host_rows(d.before, d.ar["src"]), host_rows(d.before, d.ar["par"])
    g = orc.init_tables(k, m - k, a)
    for b in range(B):
        data = [np.ascontiguousarray(s) if j not in err[b] else np.ascontiguousarray(d.want[b][err[b].index(j)])
                for j, s in enumerate(src[b])]
        ref = [np.zeros(L, np.uint8) for _ in range(m - k)]
        orc.encode_data(L, k, m - k, g, data, ref)
        for i in range(m - k):
            have = d.want[b][err[b].index(k + i)] if k + i in err[b] else par[b, i]
            assert np.array_equal(have, ref[i]), "the arena's parity is not the oracle's"
    assert names(d.run(ctx, d.general(matrix))) == want


@pytest.mark.parametrize("tiles", [2, 3])
@pytest.mark.parametrize("L", [4128, 6176])
def test_decode_tiles_per_workgroup(ctx, L, tiles):
    """The two-wave layouts with 2 and 3 column tiles per workgroup
    (rsgpu_internal_set_jitw_tiles) on 3 and 4 tiles, the last of one lane."""
    d = shared(("dec", (24, 20), L, "p48"), lambda: DecodeArena(ctx, 24, 20, L, "p48"))
    hook("rsgpu_internal_set_jitw_tiles", ctx, tiles)
    try:
        assert names(d.run(ctx, d.decode, "generated")) == decode_names(24, 20, "generated")
    finally:
        hook("rsgpu_internal_set_jitw_tiles", ctx, 0)


@pytest.mark.parametrize("code", [(24, 20), (40, 34), (70, 66)], ids=case_id)
def test_decode_code_prefetch(ctx, code):
    """k_rs_jitw's code prefetch forced on (rsgpu_internal_set_jitw_prefetch)."""
    k, e = code
    d = DecodeArena(ctx, k, e, 2080, "p16")
    hook("rsgpu_internal_set_jitw_prefetch", ctx, 1)
    try:
        assert names(d.run(ctx, d.decode, "generated")) == decode_names(k, e, "generated")
    finally:
        hook("rsgpu_internal_set_jitw_prefetch", ctx, -1)


@pytest.mark.parametrize("parts", [2, 3])
def test_decode_pipelined(ctx, parts):
    """5 blocks in slices of 4 and 1 (rsgpu_internal_set_decode_pipeline):
    prepare and emission on a second stream, each slice through its own part
    of the workspace and the status; block 3 has a malformed list."""
    d = shared(("pipe",), lambda: DecodeArena(ctx, 24, 20, 2080, "p48", blocks=5, bad=3))
    hook("rsgpu_internal_set_decode_pipeline", ctx, parts)
    try:
        recs = d.run(ctx, d.decode, "generated")
    finally:
        hook("rsgpu_internal_set_decode_pipeline", ctx, -1)
    assert recs == [(n, nb) for nb in (4, 1) for n in decode_names(24, 20, "generated")]


# ---- encode -----------------------------------------------------------------

BUILT_IN = ((5, 4), (16, 4), (64, 32))
CAUCHY = ((6, 3), (24, 20), (9, 40), (70, 66))
ENCODE_CODES = tuple((k, e, "rs") for k, e in BUILT_IN) + tuple((k, e, "cauchy") for k, e in CAUCHY)


def encode_names(kernel, k, e, kind, L, vectors):
    """What an encode of 3 blocks records (rsgpu_capi.cpp encode_slice): the
    Karatsuba program; the compiled kernels of a built-in code (the split form
    of a single-chunk code in a small call; the nibble-table kernel for len %
    4 == 0); the shared generated program in passes of <= 64 rows (e > 16) or
    <= 32; threaded code in passes of 32 rows; the v_perm kernel."""
    a32 = vectors and L % 32 == 0
    compiled = kernel in ("auto", "compiled", "karatsuba") and kind == "rs"
    if kernel == "karatsuba" and compiled and (k, e) == (64, 32) and a32:
        return ["k_rs_jit(encode)"]
    if compiled and a32:
        return ["k_rs_bs(encode)" if (k, e) == (64, 32) else "k_rs_bs_split(encode)"]
    if compiled and vectors and L % 4 == 0:
        return ["k_rs_encode_lh"]
    if a32 and kernel != "threaded":
        return ["k_rs_jit(encode)"] * ((e + 63) // 64 if e > 16 else (e + 31) // 32)
    if a32:
        return ["k_rs_tc(encode)"] * ((e + 31) // 32)
    return ["k_dot_generic"]


class EncodeArena:
    """B synthetic blocks and room for their parity in one arena; want: the
    oracle's parity of the sources."""

    def __init__(self, ctx, orc, k, e, kind, L, mode, blocks=B):
        self.k, self.e, self.L, self.blocks = k, e, L, blocks
        self.pitch, offset = pitch_of(L, mode)
        self.coef = None if kind == "rs" else sm.cauchy_matrix(k, e)
        ar = self.ar = fp.Arena()
        ar.rows("src", blocks, k, self.pitch, L, offset)
        ar.rows("par", blocks, e, self.pitch, L, offset)
        ar.allocate(torch.device("cuda", 0), seed=e * 1000 + L)
        ctx.fill_synthetic(ar.ptr("src"), blocks * k, L, self.pitch, 5, 0)
        torch.cuda.synchronize()
        self.pristine = ar.t.clone()
        self.before = ar.snapshot()
        a = orc.gen_rs_matrix(k + e, k)[k:] if self.coef is None else self.coef
        g = orc.init_tables(k, e, a)
        src = host_rows(self.before, ar["src"])
        self.want = np.zeros((blocks, e, L), np.uint8)
        for b in range(blocks):
            ref = [np.zeros(L, np.uint8) for _ in range(e)]
            orc.encode_data(L, k, e, g, [np.ascontiguousarray(s) for s in src[b]], ref)
            self.want[b] = np.stack(ref)

    def run(self, ctx, kernel):
        ar = self.ar
        ar.t.copy_(self.pristine)
        torch.cuda.synchronize()
        ctx.set_encode_kernel(kernel)
        try:
            recs = gf.recorded(ctx, lambda: ctx.encode_blocks(self.k, self.e, self.L, self.pitch, self.blocks,
                                                              ar.ptr("src"), ar.ptr("par"), coef=self.coef))
        finally:
            ctx.set_encode_kernel("auto")
        torch.cuda.synchronize()
        after = ar.snapshot()
        ar.check(self.before, after, fp.encode_allowed(ar))
        assert np.array_equal(host_rows(after, ar["par"]), self.want), "parity differs from the oracle's"
        return recs


ENCODE_ALIGNED = rotation(ENCODE_KERNELS, ENCODE_CODES, ALIGNED_LENS, ALIGNED_MODES)
# the kernel choice by turns; besides, the nibble-table kernel of the built-in
# codes wherever it applies (len % 4 == 0 on 16-byte vector rows)
ENCODE_UNALIGNED = [(c, L, m, ENCODE_KERNELS[(ci + li + mi) % 5]) for ci, c in enumerate(ENCODE_CODES)
                    for li, L in enumerate(UNALIGNED_LENS) for mi, m in enumerate(UNALIGNED_MODES)]
ENCODE_UNALIGNED += [(c, L, m, "compiled") for c in ENCODE_CODES[:3] for L, m in ((8, "r16"), (16, "eq"))
                     if (c, L, m, "compiled") not in ENCODE_UNALIGNED]


@pytest.mark.parametrize("code,L,mode,kernel", ENCODE_ALIGNED, ids=case_id)
def test_encode_blocks_aligned(ctx, orc, code, L, mode, kernel):
    k, e, kind = code
    d = shared(("enc", code, L, mode), lambda: EncodeArena(ctx, orc, k, e, kind, L, mode))
    assert d.run(ctx, kernel) == encode_names(kernel, k, e, kind, L, True)


@pytest.mark.parametrize("code,L,mode,kernel", ENCODE_UNALIGNED, ids=case_id)
def test_encode_blocks_unaligned(ctx, orc, code, L, mode, kernel):
    k, e, kind = code
    d = EncodeArena(ctx, orc, k, e, kind, L, mode)
    assert d.run(ctx, kernel) == encode_names(kernel, k, e, kind, L, vector_rows(L, mode))


@pytest.mark.parametrize("kernel", ENCODE_KERNELS)
@pytest.mark.parametrize("code", ENCODE_CODES, ids=case_id)
def test_encode_blocks_one_block(ctx, orc, code, kernel):
    k, e, kind = code
    d = shared(("enc1", code), lambda: EncodeArena(ctx, orc, k, e, kind, 2080, "p48", blocks=1))
    assert d.run(ctx, kernel) == encode_names(kernel, k, e, kind, 2080, True)


# ---- the ISA-L pointer calls --------------------------------------------------

PK, PROWS = 5, 3
POINTER_LENS = UNALIGNED_LENS + (32, 2080)
# byte offsets of the rows past their alignment: all at 0, 1, 15; by turns
POINTER_OFFSETS = {"0": (0,), "1": (1,), "15": (15,), "mixed": (0, 1, 15)}


class PointerArena:
    """Every row of a pointer call a buffer of its own in one arena, the guard
    bands the gaps between the rows: data0.., coding0.., upd (the update's
    source), dest (the single-output calls' row)."""

    def __init__(self, L, offsets):
        ar = self.ar = fp.Arena()
        self.names = [f"data{j}" for j in range(PK)] + [f"coding{r}" for r in range(PROWS)] + ["upd", "dest"]
        for i, n in enumerate(self.names):
            ar.rows(n, 1, 1, L, L, offsets[i % len(offsets)])
        ar.allocate(torch.device("cuda", 0), seed=L)
        self.L = L
        self.vectors = all(ar.ptr(n) % 16 == 0 for n in self.names)

    def host(self, a, name):
        r = self.ar[name]
        return np.ascontiguousarray(a[r.start: r.end])

    def call(self, ctx, f, written):
        """f() with the whole arena compared around it: only the rows
        `written` may change.  Returns (record names, arena after)."""
        before = self.ar.snapshot()
        recs = gf.recorded(ctx, f)
        torch.cuda.synchronize()
        after = self.ar.snapshot()
        self.ar.check(before, after, [rg for n in written for rg in self.ar[n].row_ranges()])
        return recs, after


@pytest.mark.parametrize("offsets", list(POINTER_OFFSETS))
@pytest.mark.parametrize("L", POINTER_LENS)
def test_pointer_calls(ctx, orc, L, offsets):
    """ec_encode_data, ec_encode_data_update, gf_vect_dot_prod, gf_vect_mad and
    gf_vect_mul on rows at byte offsets 0, 1 and 15: the gaps, the guards and
    the source rows stay, the outputs equal the oracle's."""
    p = PointerArena(L, POINTER_OFFSETS[offsets])
    ar = p.ar
    rng = np.random.default_rng(L)
    coef = rng.integers(1, 256, (PROWS, PK), dtype=np.uint8)
    g = orc.init_tables(PK, PROWS, coef)
    first = ar.snapshot()
    data = [p.host(first, f"data{j}") for j in range(PK)]
    d_data = [ar.ptr(f"data{j}") for j in range(PK)]
    coding = [f"coding{r}" for r in range(PROWS)]
    d_coding = [ar.ptr(n) for n in coding]
    fast = p.vectors and L % 32 == 0
    dot = ["k_rs_jit(ec_encode_data)"] if fast else ["k_dot_generic"]

    recs, after = p.call(ctx, lambda: ctx.ec_encode_data(L, PK, PROWS, g, d_data, d_coding), coding)
    ref = [np.zeros(L, np.uint8) for _ in range(PROWS)]
    orc.encode_data(L, PK, PROWS, g, data, ref)
    assert recs == dot and all(np.array_equal(p.host(after, coding[r]), ref[r]) for r in range(PROWS))
    if fast:  # the same call through threaded code, the rows it just wrote gone
        for n in coding:
            ar.view(n).fill_(0x3C)
        ctx.set_encode_kernel("threaded")
        try:
            recs, after = p.call(ctx, lambda: ctx.ec_encode_data(L, PK, PROWS, g, d_data, d_coding), coding)
        finally:
            ctx.set_encode_kernel("auto")
        assert recs == ["k_rs_tc(ec_encode_data)"]
        assert all(np.array_equal(p.host(after, coding[r]), ref[r]) for r in range(PROWS))

    upd = p.host(first, "upd")
    recs, after = p.call(ctx, lambda: ctx.ec_encode_data_update(L, PK, PROWS, 2, g, ar.ptr("upd"), d_coding), coding)
    orc.encode_data_update(L, PK, PROWS, 2, g, upd, ref)
    assert recs == [] and all(np.array_equal(p.host(after, coding[r]), ref[r]) for r in range(PROWS))

    g1 = np.ascontiguousarray(g[: 32 * PK])
    recs, after = p.call(ctx, lambda: ctx.gf_vect_dot_prod(L, PK, g1, d_data, ar.ptr("dest")), ["dest"])
    one = [np.zeros(L, np.uint8)]
    orc.encode_data(L, PK, 1, g1, data, one)
    assert recs == dot and np.array_equal(p.host(after, "dest"), one[0])

    recs, after = p.call(ctx, lambda: ctx.gf_vect_mad(L, PK, 3, g1, ar.ptr("upd"), ar.ptr("dest")), ["dest"])
    orc.encode_data_update(L, PK, 1, 3, g1, upd, one)
    assert recs == [] and np.array_equal(p.host(after, "dest"), one[0])

    tbl = orc.vect_mul_init(0x53)
    rc = []
    recs, after = p.call(ctx, lambda: rc.append(ctx.gf_vect_mul(L, tbl, ar.ptr("upd"), ar.ptr("dest"))),
                         ["dest"] if L % 32 == 0 else [])
    if L % 32:  # as ISA-L's: an error, and nothing written
        assert rc[0] != 0 and recs == []
    else:
        mul = np.zeros(L, np.uint8)
        orc.vect_mul(L, tbl, upd, mul)
        assert rc[0] == 0 and recs == dot and np.array_equal(p.host(after, "dest"), mul)


# ---- the host-resident calls ---------------------------------------------------

# (len, host pitch): (1000, 1024) and (66000, 66048) have the host pitch of
# the device staging (len rounded up to 256); 66000 is above the 64 KiB from
# which the decode ships the survivors as runs of rows
HOST_SHAPES = ((1000, 1000), (1000, 1024), (1000, 1001), (4096, 4144), (66000, 66048))
HOST_ENCODE = {(10, 4): "k_rs_jit(encode)", (20, 7): "k_rs_bs_split(encode)"}  # on 4096-byte rows
HOST_DECODE = {(10, 4): "k_rs_tc_fused(decode)", (20, 7): "k_rs_syn_split(decode)"}


@pytest.mark.parametrize("L,pitch", HOST_SHAPES, ids=case_id)
@pytest.mark.parametrize("k,e", [(10, 4), (20, 7)])
def test_host_resident_calls(ctx, orc, k, e, L, pitch):
    """rsgpu_encode_blocks_host writes [0, len) of the parity rows only;
    rsgpu_decode_blocks_host writes [0, len) of the h_out rows and `blocks`
    ints of h_status only; h_src, h_parity and h_err stay.  All five buffers
    lie in one pinned arena."""
    ar = fp.Arena()
    ar.rows("src", B, k, pitch, L)
    ar.rows("par", B, e, pitch, L)
    ar.rows("out", B, e, pitch, L)
    ar.flat("err", B * e)
    ar.flat("status", 4 * B)
    ar.allocate(None, seed=L + pitch)
    dev = torch.zeros(B * k * pitch, dtype=torch.uint8, device="cuda")
    ctx.fill_synthetic(dev, B * k, L, pitch, 31, 0)
    torch.cuda.synchronize()
    ar.view("src").copy_(dev.view(B, k, pitch)[:, :, :L])

    before = ar.snapshot()
    enc = gf.recorded(ctx, lambda: ctx.encode_blocks_host(k, e, L, pitch, B, ar.ptr("src"), ar.ptr("par")))
    after = ar.snapshot()
    ar.check(before, after, fp.encode_allowed(ar))
    g = orc.init_tables(k, e, orc.gen_rs_matrix(k + e, k)[k:])
    src = host_rows(before, ar["src"])
    for b in range(B):
        ref = [np.zeros(L, np.uint8) for _ in range(e)]
        orc.encode_data(L, k, e, g, [np.ascontiguousarray(s) for s in src[b]], ref)
        assert np.array_equal(host_rows(after, ar["par"])[b], np.stack(ref)), "parity differs from the oracle's"
    assert enc == ([HOST_ENCODE[k, e]] if L % 32 == 0 else ["k_dot_generic"])

    err = rsgpu.erasure_patterns(7, 0, B, k, e)
    pick = (torch.arange(B)[:, None], torch.from_numpy(err.astype(np.int64)))
    want = ar.view("src")[pick].numpy().copy()
    ar.view("src")[pick] = POISON
    ar.buf("err").copy_(torch.from_numpy(err.reshape(-1).copy()))
    ar.ints("status").fill_(7)
    before = ar.snapshot()
    dec = gf.recorded(ctx, lambda: ctx.decode_blocks_host(k, e, L, pitch, B, ar.ptr("src"), ar.ptr("par"),
                                                          ar.ptr("err"), ar.ptr("out"), ar.ptr("status")))
    after = ar.snapshot()
    ar.check(before, after, fp.decode_allowed(ar, 0))
    assert (host_rows(after, ar["src"])[np.arange(B)[:, None], err.astype(np.int64)] == POISON).all()
    assert after[ar["status"].start: ar["status"].end].view(np.int32).tolist() == [0] * B
    assert np.array_equal(host_rows(after, ar["out"]), want), "decoded rows differ"
    assert dec == ([HOST_DECODE[k, e]] if L % 32 == 0 else [PREP, DOT])
