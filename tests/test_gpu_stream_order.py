"""Stream order of every device entry point, observed behind a gated stream
(tests/stream_gate.py has the method): include/rsgpu.h's "work is enqueued on
the context's HIP stream; nothing synchronises unless the function says so",
and rsgpu_set_stream's "work on the old stream is ordered before anything
enqueued afterwards".

Every row of CASES runs warm (the call has run before: the result is the
ordinary run's AND the call returns while the gate is closed) and cold (a
matrix, lists and data the context has not seen, after a warm-up of the same
sizes: the result is right; whether the gate was still closed at the return is
recorded).  The ordinary run every gated one is compared with is itself
checked against the numpy models of the family suites (scrub_model.py and the
others), and its timing records are pinned in NAMES, so that each case is
known to run the kernel it is named for.  Then the sequences: rsgpu_set_stream
under load, two calls back to back behind one gate, eviction from the cache of
64 programs behind the gate, two contexts.  The premise checks come first and
fail loudly: a side stream's gate does not hold the null stream back, and a
context deliberately left on the null stream does compute a different result
(the negative controls; they read decoys only).

Shapes: 3 blocks, len 2080 (one 2 KB tile plus a lane) at pitch len + 48; the
generated decode at len 32768 (16 tiles), the generated general decode at
98304.  GpuEncoder.heal itself ends with a read-back of its reports, so its
row runs the two device calls it makes, locate_blocks then rebuild_blocks on
the located lists, with no host decision between them.

A cold case's gated call comes before its ordinary run (the expectation made
first would be the first use), and every cold case has a matrix of its own.

Measured on an MI355X, one run of this module (the tests print the figures):
the gate is 118e6 cycles of torch.cuda._sleep (2.36e6 cycles per ms) and
lasted 49.5 ms; the longest host time of a warm call was 0.05 ms; every warm
call returned with the gate closed.  Cold calls that were seen to return with
the gate OPEN, by entry point:
    rsgpu_ec_encode_data_batch  fast + byte kernels (ec_encode_data_batch-mixed)
    rsgpu_scrub_blocks          generated
    rsgpu_locate_blocks         fused + generated
    rsgpu_repair_blocks         generated, one_row and columns
    rsgpu_correct_blocks        fused + generated
each after 49.2 ms, the rest of the gate.  All of them are first uses of a
matrix that stage two uploads in one call through the context's one pinned
buffer (the program's code, then the locator, the matrix or the byte kernel's
tables): the second waits on the host until the first has left the buffer,
which is behind the gate.  The cold generated encode, ec_encode_data and the
batch under ALIGNED32 stage once and returned with the gate closed, the (24,
20) encode's program built in 4.2 - 4.5 ms, the others in at most 0.3 ms.  In
the sequences the same wait shows when a call that stages follows one whose
upload is still behind the gate: the second call of the generated-scrub and of
the batch sequence returned with the gate open, the others with it closed; the
66 calls of the eviction took 64 ms on the host: an eviction drains the
stream before it frees a program (rsgpu_capi.cpp).  The sequences assert
results only.  In a process that has opened many streams (the whole suite) the
two side streams were seen to share a hardware queue; test_two_contexts probes
for that before it asserts that context B did not wait for A's gate."""
import ctypes
import contextlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import correct_model as cm  # noqa: E402
import degraded_model as dm  # noqa: E402
import gpu_family as gf  # noqa: E402
import locate_model as lm  # noqa: E402
import rebuild_model as rbm  # noqa: E402
import repair_model as rpm  # noqa: E402
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402
import stream_gate as sg  # noqa: E402
import update_model as um  # noqa: E402
from golden import synth  # noqa: E402

B, L0, PAD = 3, 2080, 48
POISON = 0xA5
CORRECT_FIELDS = ("bad_columns", "corrected_columns", "two_row_columns", "status", "row")


def dev():
    return torch.device("cuda", 0)


def coef_of(k, e, kind, v):
    """(coef, c) of variant v: None and the gf_gen_rs_matrix rows for `rs`; for
    `cauchy` rows v .. v + e - 1 of the Cauchy parity rows of a (k, e + v)
    code, another Cauchy (so MDS and locatable) matrix of the same size for
    every v."""
    if kind == "rs":
        return None, sm.rs_matrix(k, e)
    assert k + e + v <= 255
    c = np.ascontiguousarray(sm.cauchy_matrix(k, e + v)[v:])
    return c, c


def hook(name, ctx, n):
    f = getattr(rsgpu.testhooks(), name)
    f.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert f(ctx._h, n) == 0


@contextlib.contextmanager
def choices(ctx, kern):
    """The kernel choices (and test hooks) of a case, restored after."""
    kern = dict(kern)
    pipeline = kern.pop("pipeline", None)
    try:
        for what, choice in kern.items():
            getattr(ctx, f"set_{what}_kernel")(choice)
        if pipeline is not None:
            hook("rsgpu_internal_set_decode_pipeline", ctx, pipeline)
        yield
    finally:
        if pipeline is not None:
            hook("rsgpu_internal_set_decode_pipeline", ctx, -1)
        for what in kern:
            getattr(ctx, f"set_{what}_kernel")("auto")


# ---- cases -------------------------------------------------------------------

class Blocks(sg.Case):
    """B blocks of a (k, e) code in one arena: src, par and what more() adds.
    state(v) builds variant v of the inputs with the builder context (which
    stays on the null stream and is not the context under test, so that a cold
    matrix is cold); writes names the regions the call may change."""

    writes = ()

    def __init__(self, bctx, k, e, kind, v=0, L=L0, blocks=B):
        self.bctx, self.k, self.e, self.kind, self.v, self.L, self.B = bctx, k, e, kind, v, L, blocks
        self.pitch = L + PAD
        self.ar = sg.arena(self.layout, dev())
        self.keep = {}
        self.decoy = self.state(1)
        self.true = self.state(v)
        self.coef, self.c = coef_of(k, e, kind, v)
        self.host = {}
        if self.coef is not None:
            self.host["coef"] = sg.HostArg(self.coef, coef_of(k, e, kind, 1 if v != 1 else 0)[0])
            self.coef = self.host["coef"].live

    def layout(self, ar):
        ar.rows("src", self.B, self.k, self.pitch, self.L)
        ar.rows("par", self.B, self.e, self.pitch, self.L)
        self.more(ar)

    def more(self, ar):
        pass

    def fill(self, v):
        self.encode(v)

    def state(self, v):
        ar = self.ar
        ar.t.copy_(sg.noise_state(ar, 100 + v))
        self.bctx.fill_synthetic(ar.ptr("src"), self.B * self.k, self.L, self.pitch, 40 + v, 0)
        self.fill(v)
        torch.cuda.synchronize()
        return ar.t.clone()

    def encode(self, v):
        self.bctx.encode_blocks(self.k, self.e, self.L, self.pitch, self.B, self.ar.ptr("src"), self.ar.ptr("par"),
                                coef=coef_of(self.k, self.e, self.kind, v)[0])

    def put(self, name, a):
        """Host bytes into a flat region."""
        raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        assert raw.size <= self.ar[name].size
        self.ar.buf(name)[: raw.size].copy_(torch.from_numpy(raw.copy()))

    def damage(self, v):
        """Block (v) mod B stays clean; the next has one byte of one row
        XORed; the third two rows in one column and the first of them in
        another as well.  Rows, columns and values depend on v."""
        rng = np.random.default_rng(70 + v)
        n = self.k + self.e
        one, two = (v + 1) % self.B, (v + 2) % self.B
        self.xor(one, int(rng.integers(0, n)), int(rng.integers(0, self.L)), int(rng.integers(1, 256)))
        r1, r2 = (int(r) for r in rng.choice(n, 2, replace=False))
        col = int(rng.integers(0, self.L - 1))
        self.xor(two, r1, col, int(rng.integers(1, 256)))
        self.xor(two, r2, col, int(rng.integers(1, 256)))
        self.xor(two, r1, col + 1, int(rng.integers(1, 256)))

    def xor(self, b, row, col, x):
        name, r = ("src", row) if row < self.k else ("par", row - self.k)
        self.ar.view(name)[b, r, col] ^= x

    def lists(self, v, u, top, counts=(1, 2, 0)):
        """(B, u) lists of rows in [0, top): block b has counts[(b + v) mod 3]
        of them, ascending, then 255."""
        rng = np.random.default_rng(80 + v)
        out = np.full((self.B, u), 255, np.uint8)
        for b in range(self.B):
            n = counts[(b + v) % len(counts)]
            out[b, :n] = np.sort(rng.choice(top, n, replace=False))
        return out

    def rows(self, a, name):
        return sg.host_rows(a, self.ar[name])

    def flat(self, a, name, dtype=np.uint8):
        r = self.ar[name]
        return a[r.start: r.end].view(dtype)

    def untouched(self, before, after):
        m = self.mask()
        for name in self.writes:
            r = self.ar[name]
            m[r.start: r.end] = False
        bad = (before != after) & m
        assert not bad.any(), f"{self.ar.describe(int(np.argmax(bad)))} written"

    def verify(self, before, after):
        self.untouched(before, after)
        self.model(before, after)

    def geometry(self):
        return self.k, self.e, self.L, self.pitch, self.B

    def blocks_args(self):
        return self.geometry() + (self.ar.ptr("src"), self.ar.ptr("par"))


class Encode(Blocks):
    writes = ("par",)

    def fill(self, v):
        pass  # the parity rows hold noise

    def call(self, ctx):
        ctx.encode_blocks(*self.blocks_args(), coef=self.coef)

    def model(self, before, after):
        src, par = self.rows(before, "src"), self.rows(after, "par")
        for b in range(self.B):
            assert np.array_equal(par[b], rbm.encode(self.c, src[b])), f"parity of block {b}"


class Pointer(Blocks):
    """The ISA-L pointer calls at (5, 3): data rows, coding rows, the update's
    source `upd` and the single output `dest`, every row at the pitch."""
    writes = ("par", "dest")

    def __init__(self, bctx, which, v=0):
        self.which = which
        super().__init__(bctx, 5, 3, "cauchy", v, blocks=1)
        g = lambda w: rsgpu.ec_init_tables(5, 3, coef_of(5, 3, "cauchy", w)[0])  # noqa: E731
        self.host = {"gftbls": sg.HostArg(g(v), g(1 if v != 1 else 0))}
        self.g = self.host["gftbls"].live
        self.g1 = self.g[: 32 * 5]
        tbl = lambda w: rsgpu.gf_vect_mul_init(0x53 + w)  # noqa: E731
        self.host["gftbl"] = sg.HostArg(tbl(v), tbl(1 if v != 1 else 0))

    def more(self, ar):
        ar.rows("upd", 1, 1, self.pitch, self.L)
        ar.rows("dest", 1, 1, self.pitch, self.L)

    def fill(self, v):
        ar = self.ar
        self.bctx.fill_synthetic(ar.ptr("par"), 3, self.L, self.pitch, 50 + v, 0)
        self.bctx.fill_synthetic(ar.ptr("upd"), 1, self.L, self.pitch, 60 + v, 0)
        self.bctx.fill_synthetic(ar.ptr("dest"), 1, self.L, self.pitch, 65 + v, 0)

    def ptrs(self, name, n):
        return [self.ar.ptr(name) + i * self.pitch for i in range(n)]

    def call(self, ctx):
        ar, L = self.ar, self.L
        if self.which == "ec_encode_data":
            ctx.ec_encode_data(L, 5, 3, self.g, self.ptrs("src", 5), self.ptrs("par", 3))
        elif self.which == "ec_encode_data_update":
            ctx.ec_encode_data_update(L, 5, 3, 2, self.g, ar.ptr("upd"), self.ptrs("par", 3))
        elif self.which == "gf_vect_dot_prod":
            ctx.gf_vect_dot_prod(L, 5, self.g1, self.ptrs("src", 5), ar.ptr("dest"))
        elif self.which == "gf_vect_mad":
            ctx.gf_vect_mad(L, 5, 3, self.g1, ar.ptr("upd"), ar.ptr("dest"))
        else:
            assert ctx.gf_vect_mul(L, self.host["gftbl"].live, ar.ptr("upd"), ar.ptr("dest")) == 0

    def model(self, before, after):
        c = self.c
        src, upd = self.rows(before, "src")[0], self.rows(before, "upd")[0]
        par0, dest0 = self.rows(before, "par")[0], self.rows(before, "dest")[0]
        par, dest = self.rows(after, "par")[0], self.rows(after, "dest")[0]
        want_par, want_dest = par0, dest0
        if self.which == "ec_encode_data":
            want_par = rbm.encode(c, src)
        elif self.which == "ec_encode_data_update":
            want_par = par0 ^ sm.gf_mul(c[:, 2][:, None], upd)
        elif self.which == "gf_vect_dot_prod":
            want_dest = rbm.encode(c[:1], src)
        elif self.which == "gf_vect_mad":
            want_dest = dest0 ^ sm.gf_mul(c[0, 3], upd)
        else:
            want_dest = sm.gf_mul(0x53 + self.v, upd)
        assert np.array_equal(par, want_par) and np.array_equal(dest, want_dest)


class Batch(Blocks):
    """rsgpu_ec_encode_data_batch at (5, 3): the rows of a block anywhere in
    the arena, a length per block.  The true tables name rows of the working
    arena; the decoy tables name the same rows of `shadow`, a second arena
    that holds the decoy state."""
    writes = ("par", "status")
    LENS = {False: ((2080, 2077, 64), (1056, 2080, 33), (2048, 31, 2080)),
            True: ((2080, 2048, 64), (1056, 2080, 32), (2048, 96, 2080))}

    def __init__(self, bctx, aligned32, v=0):
        self.aligned32 = aligned32
        self.lens = self.LENS[aligned32][min(v, 2)]
        self.shadow = None
        super().__init__(bctx, 5, 3, "cauchy", v)
        self.shadow.copy_(self.decoy)
        g = lambda w: rsgpu.ec_init_tables(5, 3, coef_of(5, 3, "cauchy", w)[0])  # noqa: E731
        self.host = {"gftbls": sg.HostArg(g(v), g(1 if v != 1 else 0))}
        self.g = self.host["gftbls"].live

    def more(self, ar):
        ar.flat("data_tab", 8 * self.B * 5)
        ar.flat("coding_tab", 8 * self.B * 3)
        ar.flat("len_tab", 4 * self.B)
        ar.flat("status", 4 * self.B)

    def fill(self, v):
        ar = self.ar
        if self.shadow is None:
            self.shadow = torch.empty_like(ar.t)
        base = self.shadow.data_ptr() if v == 1 else ar.t.data_ptr()
        tab = lambda name, per: np.array(  # noqa: E731
            [[base + ar[name].row_start(b, i) for i in range(per)] for b in range(self.B)], np.uint64)
        self.put("data_tab", tab("src", 5))
        self.put("coding_tab", tab("par", 3))
        self.put("len_tab", np.array(self.LENS[self.aligned32][min(v, 2)], np.int32))

    def call(self, ctx):
        ar = self.ar
        ctx.ec_encode_data_batch(5, 3, self.g, self.B, ar.ptr("data_tab"), ar.ptr("coding_tab"), ar.ptr("len_tab"),
                                 2080, ar.ptr("status"), self.aligned32)

    def model(self, before, after):
        src, par0, par = self.rows(before, "src"), self.rows(before, "par"), self.rows(after, "par")
        assert self.flat(after, "status", np.int32).tolist() == [0] * self.B
        for b, n in enumerate(self.lens):
            assert np.array_equal(par[b][:, :n], rbm.encode(self.c, src[b][:, :n])), f"block {b}"
            assert np.array_equal(par[b][:, n:], par0[b][:, n:]), f"block {b} written behind its length"


class Decode(Blocks):
    """rsgpu_decode_blocks and its halves: e erased originals per block, their
    rows overwritten with 0xA5, `want` what they held."""
    writes = ("out", "status")

    def __init__(self, bctx, k, e, v=0, L=L0, blocks=B, halves=False):
        self.halves = halves
        super().__init__(bctx, k, e, "rs", v, L, blocks)

    def more(self, ar):
        ar.rows("out", self.B, self.e, self.pitch, self.L)
        ar.flat("err", self.B * self.e)
        ar.flat("workspace", rsgpu.decode_workspace_bytes(self.k, self.e, self.B))
        ar.flat("status", 4 * self.B)

    def fill(self, v):
        self.encode(v)
        err = rsgpu.erasure_patterns(23 + v, 0, self.B, self.k, self.e)
        self.erase(v, err, self.ar.view("src"))

    def erase(self, v, err, rows):
        pick = (torch.arange(self.B, device=rows.device)[:, None],
                torch.from_numpy(err.astype(np.int64)).to(rows.device))
        self.keep[v] = rows[pick].cpu().numpy()
        rows[pick] = POISON
        self.put("err", err)
        return rows

    def args(self):
        a = self.ar
        return self.blocks_args() + (a.ptr("err"), a.ptr("out"), a.ptr("workspace"), a.ptr("status"))

    def call(self, ctx):
        if self.halves:
            a = self.ar
            ctx.decode_prepare(*self.args())
            ctx.decode_apply(*self.blocks_args(), a.ptr("out"), a.ptr("workspace"), a.ptr("status"))
        else:
            ctx.decode_blocks(*self.args())

    def model(self, before, after):
        assert self.flat(after, "status", np.int32).tolist() == [0] * self.B
        assert np.array_equal(self.rows(after, "out"), self.keep[self.v]), "decoded rows differ from the erased ones"


class General(Decode):
    """rsgpu_decode_general at (6, 9) with a caller's matrix, two erasures per
    block among data and parity rows."""
    ERR = ([[1, 7], [0, 4], [2, 8]], [[0, 5], [6, 7], [3, 4]], [[2, 6], [1, 3], [5, 8]])

    def __init__(self, bctx, v=0, L=L0):
        Blocks.__init__(self, bctx, 6, 3, "cauchy", v, L)
        m = lambda w: np.concatenate([np.eye(6, dtype=np.uint8), coef_of(6, 3, "cauchy", w)[0]])  # noqa: E731
        self.host = {"encode_matrix": sg.HostArg(m(v), m(1 if v != 1 else 0))}

    def more(self, ar):
        ar.rows("out", self.B, 2, self.pitch, self.L)
        ar.flat("err", self.B * 2)
        ar.flat("workspace", rsgpu.decode_general_workspace_bytes(6, 9, 2, self.B))
        ar.flat("status", 4 * self.B)

    def fill(self, v):
        self.encode(v)
        ar = self.ar
        rows = torch.cat([ar.view("src"), ar.view("par")], dim=1)
        rows = self.erase(v, np.array(self.ERR[min(v, 2)], np.uint8), rows)
        ar.view("src")[:] = rows[:, :6]
        ar.view("par")[:] = rows[:, 6:]

    def call(self, ctx):
        a = self.ar
        ctx.decode_general(6, 9, self.L, self.pitch, self.B, self.host["encode_matrix"].live, a.ptr("src"),
                           a.ptr("par"), a.ptr("err"), 2, a.ptr("out"), a.ptr("workspace"), a.ptr("status"))


class Verify(Blocks):
    """rsgpu_verify_blocks: out holds the erased rows but for some bytes; the
    counts are ADDED to d_mismatch, whose start is part of the inputs."""
    writes = ("mism",)

    def more(self, ar):
        ar.rows("out", self.B, self.e, self.pitch, self.L)
        ar.flat("err", self.B * self.e)
        ar.flat("mism", 8 * self.B)

    def fill(self, v):
        ar = self.ar
        err = rsgpu.erasure_patterns(31 + v, 0, self.B, self.k, self.e)
        pick = (torch.arange(self.B, device=ar.t.device)[:, None],
                torch.from_numpy(err.astype(np.int64)).to(ar.t.device))
        ar.view("out")[:] = ar.view("src")[pick]
        for b in range(self.B):
            for i in range((b + v) % 3 + 1):
                ar.view("out")[b, i % self.e, 17 * (i + v) + b] ^= 0x40 + i
        self.put("err", err)
        self.put("mism", np.arange(5 + v, 5 + v + self.B, dtype=np.uint64))

    def call(self, ctx):
        a = self.ar
        ctx.verify_blocks(*self.geometry(), a.ptr("src"), a.ptr("out"), a.ptr("err"), a.ptr("mism"))

    def model(self, before, after):
        src, out, err = self.rows(before, "src"), self.rows(before, "out"), self.flat(before, "err")
        err = err.reshape(self.B, self.e).astype(np.int64)
        want = [int(self.flat(before, "mism", np.uint64)[b]) + int((out[b] != src[b][err[b]]).sum()) for b in range(self.B)]
        assert self.flat(after, "mism", np.uint64).tolist() == want


class Fill(Blocks):
    """rsgpu_fill_synthetic: no input but its arguments."""
    writes = ("src",)

    def state(self, v):
        return sg.noise_state(self.ar, 100 + v)

    def call(self, ctx):
        ctx.fill_synthetic(self.ar.ptr("src"), self.B * self.k, self.L, self.pitch, 90 + self.v, 3)

    def model(self, before, after):
        got = self.rows(after, "src").reshape(self.B * self.k, self.L)
        for r in range(self.B * self.k):
            assert np.array_equal(got[r], synth.synth_row(90 + self.v, 3 + r, self.L)), f"row {r}"


class Scrub(Blocks):
    writes = ("report",)

    def more(self, ar):
        ar.flat("report", 16 * self.B)

    def fill(self, v):
        self.encode(v)
        self.damage(v)

    def call(self, ctx):
        ctx.scrub_blocks(*self.blocks_args(), self.ar.ptr("report"), coef=self.coef)

    def model(self, before, after):
        src, par = self.rows(before, "src"), self.rows(before, "par")
        gf.same(self.flat(after, "report", gf.SCRUB_DT), [sm.scrub(self.c, src[b], par[b]) for b in range(self.B)])


class Degraded(Scrub):
    U = 4

    def more(self, ar):
        super().more(ar)
        ar.flat("lost", self.B * self.U)

    def fill(self, v):
        super().fill(v)
        self.put("lost", self.lists(v, self.U, self.k + self.e))

    def call(self, ctx):
        a = self.ar
        ctx.scrub_degraded_blocks(*self.blocks_args(), self.U, a.ptr("lost"), a.ptr("report"), coef=self.coef)

    def model(self, before, after):
        src, par = self.rows(before, "src"), self.rows(before, "par")
        lost = self.flat(before, "lost").reshape(self.B, self.U)
        gf.same(self.flat(after, "report", gf.SCRUB_DT),
                [dm.report(self.c, src[b], par[b], lost[b]) for b in range(self.B)])


class Locate(Scrub):
    U = 4
    writes = ("report", "rows")

    def more(self, ar):
        super().more(ar)
        ar.flat("rows", self.B * self.U)

    def call(self, ctx):
        a = self.ar
        ctx.locate_blocks(*self.blocks_args(), self.U, a.ptr("rows"), a.ptr("report"), coef=self.coef)

    def located(self, before):
        src, par = self.rows(before, "src"), self.rows(before, "par")
        return [lm.report(self.c, src[b], par[b], self.U) for b in range(self.B)]

    def model(self, before, after):
        want = self.located(before)
        gf.same(self.flat(after, "report", gf.SCRUB_DT), [w[0] for w in want])
        assert np.array_equal(self.flat(after, "rows").reshape(self.B, self.U), np.stack([w[1] for w in want]))


class Heal(Locate):
    """What GpuEncoder.heal enqueues: locate_blocks, then rebuild_blocks
    without the check on the located lists, which stay on the device."""
    writes = ("report", "rows", "report2", "src", "par")

    def more(self, ar):
        super().more(ar)
        ar.flat("report2", 16 * self.B)

    def call(self, ctx):
        a = self.ar
        super().call(ctx)
        ctx.rebuild_blocks(*self.blocks_args(), self.U, a.ptr("rows"), a.ptr("report2"), coef=self.coef, check=False)

    def model(self, before, after):
        super().model(before, after)
        src, par = self.rows(before, "src"), self.rows(before, "par")
        want = [rbm.call(self.c, src[b], par[b], w[1], False) for b, w in enumerate(self.located(before))]
        gf.same(self.flat(after, "report2", gf.SCRUB_DT), [w[0] for w in want])
        for b, w in enumerate(want):
            assert np.array_equal(self.rows(after, "src")[b], w[1]) and np.array_equal(self.rows(after, "par")[b], w[2])


class Repair(Scrub):
    writes = ("report", "src", "par")

    def __init__(self, bctx, k, e, kind, mode, v=0):
        self.mode = mode
        super().__init__(bctx, k, e, kind, v)

    def more(self, ar):
        ar.flat("report", 24 * self.B)

    def call(self, ctx):
        ctx.repair_blocks(*self.blocks_args(), self.ar.ptr("report"), coef=self.coef, mode=self.mode)

    def fixed(self, b, src, par):
        return rpm.repair(self.c, src, par, self.mode)

    fields, dtype = gf.REPAIR_FIELDS, rsgpu.REPAIR_REPORT_DTYPE

    def model(self, before, after):
        src, par = self.rows(before, "src"), self.rows(before, "par")
        want = [self.fixed(b, src[b], par[b]) for b in range(self.B)]
        gf.same(self.flat(after, "report", self.dtype), [w[2] for w in want], self.fields)
        for b, w in enumerate(want):
            assert np.array_equal(self.rows(after, "src")[b], w[0]) and np.array_equal(self.rows(after, "par")[b], w[1])


class Correct(Repair):
    fields, dtype = CORRECT_FIELDS, rsgpu.CORRECT_REPORT_DTYPE

    def __init__(self, bctx, k, e, kind, v=0):
        super().__init__(bctx, k, e, kind, None, v)

    def more(self, ar):
        ar.flat("report", 32 * self.B)

    def call(self, ctx):
        ctx.correct_blocks(*self.blocks_args(), self.ar.ptr("report"), coef=self.coef, t=2)

    def fixed(self, b, src, par):
        return cm.correct(self.c, src, par, 2)


class Rebuild(Degraded):
    """The listed rows hold 0xA5 when the call comes; with the check a
    damaged survivor decides per block."""
    writes = ("report", "src", "par")

    def __init__(self, bctx, k, e, kind, check, v=0):
        self.check = check
        super().__init__(bctx, k, e, kind, v)

    def fill(self, v):
        self.encode(v)
        if self.check:
            self.damage(v)
        lost = self.lists(v, self.U, self.k + self.e)
        for b in range(self.B):
            for r in dm.list_rows(lost[b], self.k, self.e):
                name, i = ("src", r) if r < self.k else ("par", r - self.k)
                self.ar.view(name)[b, i] = POISON
        self.put("lost", lost)

    def call(self, ctx):
        a = self.ar
        ctx.rebuild_blocks(*self.blocks_args(), self.U, a.ptr("lost"), a.ptr("report"), coef=self.coef,
                           check=self.check)

    def model(self, before, after):
        src, par = self.rows(before, "src"), self.rows(before, "par")
        lost = self.flat(before, "lost").reshape(self.B, self.U)
        want = [rbm.call(self.c, src[b], par[b], lost[b], self.check) for b in range(self.B)]
        gf.same(self.flat(after, "report", gf.SCRUB_DT), [w[0] for w in want])
        for b, w in enumerate(want):
            assert np.array_equal(self.rows(after, "src")[b], w[1]) and np.array_equal(self.rows(after, "par")[b], w[2])


class Update(Blocks):
    U = 2
    writes = ("src", "par", "status")

    def __init__(self, bctx, k, e, kind, delta, v=0):
        self.delta = delta
        super().__init__(bctx, k, e, kind, v)

    def more(self, ar):
        ar.rows("upd", self.B, self.U, self.pitch, self.L)
        ar.flat("cols", self.B * self.U)
        ar.flat("status", 4 * self.B)

    def fill(self, v):
        self.encode(v)
        self.bctx.fill_synthetic(self.ar.ptr("upd"), self.B * self.U, self.L, self.pitch, 55 + v, 0)
        self.put("cols", self.lists(v, self.U, self.k))

    def call(self, ctx):
        a = self.ar
        ctx.update_blocks(*self.geometry(), self.U, a.ptr("cols"), a.ptr("upd"), None if self.delta else a.ptr("src"),
                          a.ptr("par"), a.ptr("status"), coef=self.coef, delta=self.delta)

    def model(self, before, after):
        src, par, upd = self.rows(before, "src"), self.rows(before, "par"), self.rows(before, "upd")
        cols = self.flat(before, "cols").reshape(self.B, self.U)
        assert self.flat(after, "status", np.int32).tolist() == [0] * self.B
        for b in range(self.B):
            s, p, _ = um.update(self.c, src[b], par[b], cols[b], upd[b], self.delta)
            if not self.delta:
                assert np.array_equal(self.rows(after, "src")[b], s), f"sources of block {b}"
            assert np.array_equal(self.rows(after, "par")[b], p), f"parity of block {b}"


# ---- the case table ------------------------------------------------------------
# id: (entry points, kernel choices and hooks, factory(builder context, variant))

CASES = {}


def add(ident, entries, kern, make):
    assert ident not in CASES
    CASES[ident] = (tuple(entries), kern, make)


for _k, _e, _kind in ((64, 32, "rs"), (5, 4, "rs"), (24, 20, "cauchy")):
    for _kn in ("auto", "compiled", "generated", "threaded", "karatsuba"):
        add(f"encode_blocks-{_k}-{_e}-{_kind}-{_kn}", ["rsgpu_encode_blocks"], {"encode": _kn},
            lambda b, v, k=_k, e=_e, kind=_kind: Encode(b, k, e, kind, v))
for _w in ("ec_encode_data", "ec_encode_data_update", "gf_vect_dot_prod", "gf_vect_mad", "gf_vect_mul"):
    add(_w, ["rsgpu_" + _w], {}, lambda b, v, w=_w: Pointer(b, w, v))
add("ec_encode_data-threaded", ["rsgpu_ec_encode_data"], {"encode": "threaded"},
    lambda b, v: Pointer(b, "ec_encode_data", v))
add("ec_encode_data_batch-mixed", ["rsgpu_ec_encode_data_batch"], {}, lambda b, v: Batch(b, False, v))
add("ec_encode_data_batch-aligned32", ["rsgpu_ec_encode_data_batch"], {}, lambda b, v: Batch(b, True, v))
add("ec_encode_data_batch-threaded", ["rsgpu_ec_encode_data_batch"], {"encode": "threaded"},
    lambda b, v: Batch(b, False, v))
for _k, _e in ((5, 4), (24, 20), (70, 66)):
    for _kn in ("auto", "generated", "one_matrix", "general"):
        add(f"decode_blocks-{_k}-{_e}-{_kn}", ["rsgpu_decode_blocks"], {"decode": _kn},
            lambda b, v, k=_k, e=_e, L=32768 if _kn == "generated" else L0: Decode(b, k, e, v, L))
add("decode_prepare-apply", ["rsgpu_decode_prepare", "rsgpu_decode_apply"], {},
    lambda b, v: Decode(b, 24, 20, v, halves=True))
add("decode_prepare-apply-generated", ["rsgpu_decode_prepare", "rsgpu_decode_apply"], {"decode": "generated"},
    lambda b, v: Decode(b, 24, 20, v, 32768, halves=True))
add("decode_general-threaded", ["rsgpu_decode_general"], {}, lambda b, v: General(b, v))
add("decode_general-generated", ["rsgpu_decode_general"], {}, lambda b, v: General(b, v, 98304))
add("decode_blocks-pipelined", ["rsgpu_decode_blocks"], {"decode": "generated", "pipeline": 2},
    lambda b, v: Decode(b, 24, 20, v, blocks=5))
add("scrub_blocks-two_pass", ["rsgpu_scrub_blocks"], {"scrub": "two_pass"}, lambda b, v: Scrub(b, 16, 4, "rs", v))
add("scrub_blocks-fused", ["rsgpu_scrub_blocks"], {"scrub": "fused"}, lambda b, v: Scrub(b, 16, 4, "rs", v))
add("scrub_blocks-generated", ["rsgpu_scrub_blocks"], {"scrub": "generated"},
    lambda b, v: Scrub(b, 10, 4, "cauchy", v))
add("scrub_degraded_blocks-lanes", ["rsgpu_scrub_degraded_blocks"], {"degraded": "two_pass"},
    lambda b, v: Degraded(b, 16, 4, "rs", v))
add("scrub_degraded_blocks-fused", ["rsgpu_scrub_degraded_blocks"], {"degraded": "fused"},
    lambda b, v: Degraded(b, 16, 4, "rs", v))
add("locate_blocks-two_pass", ["rsgpu_locate_blocks"], {"locate": "two_pass"}, lambda b, v: Locate(b, 16, 4, "rs", v))
add("locate_blocks-fused", ["rsgpu_locate_blocks"], {"locate": "fused"}, lambda b, v: Locate(b, 16, 4, "rs", v))
add("locate_blocks-fused-generated", ["rsgpu_locate_blocks"], {"locate": "fused", "scrub": "generated"},
    lambda b, v: Locate(b, 10, 4, "cauchy", v))
for _mode in ("one_row", "columns"):
    add(f"repair_blocks-{_mode}-two_pass", ["rsgpu_repair_blocks"], {"scrub": "two_pass"},
        lambda b, v, m=_mode: Repair(b, 16, 4, "rs", m, v))
    add(f"repair_blocks-{_mode}-fused", ["rsgpu_repair_blocks"], {"scrub": "fused"},
        lambda b, v, m=_mode: Repair(b, 16, 4, "rs", m, v))
    add(f"repair_blocks-{_mode}-generated", ["rsgpu_repair_blocks"], {"repair": "generated"},
        lambda b, v, m=_mode: Repair(b, 10, 4, "cauchy", m, v))
add("correct_blocks-two_pass", ["rsgpu_correct_blocks"], {"correct": "two_pass"},
    lambda b, v: Correct(b, 16, 8, "rs", v))
add("correct_blocks-fused", ["rsgpu_correct_blocks"], {"correct": "fused"}, lambda b, v: Correct(b, 16, 8, "rs", v))
add("correct_blocks-fused-generated", ["rsgpu_correct_blocks"], {"correct": "fused", "scrub": "generated"},
    lambda b, v: Correct(b, 10, 6, "cauchy", v))
for _kn in ("lanes", "threaded"):
    for _check in (True, False):
        add(f"rebuild_blocks-{_kn}-{'checked' if _check else 'unchecked'}", ["rsgpu_rebuild_blocks"],
            {"rebuild": _kn}, lambda b, v, c=_check: Rebuild(b, 16, 4, "rs", c, v))
add("update_blocks-plain", ["rsgpu_update_blocks"], {}, lambda b, v: Update(b, 16, 4, "rs", False, v))
add("update_blocks-delta", ["rsgpu_update_blocks"], {}, lambda b, v: Update(b, 10, 4, "cauchy", True, v))
add("heal", ["rsgpu_locate_blocks", "rsgpu_rebuild_blocks"], {}, lambda b, v: Heal(b, 16, 4, "rs", v))
add("verify_blocks", ["rsgpu_verify_blocks"], {}, lambda b, v: Verify(b, 16, 4, "rs", v))
add("fill_synthetic", ["rsgpu_fill_synthetic"], {}, lambda b, v: Fill(b, 16, 4, "rs", v))


def covered(cases):
    """The entry points the rows of a case table name."""
    return {e for entries, _, _ in cases.values() for e in entries}


# The timing records of each case's ordinary run, warm and cold alike.
ENC = "k_rs_bs_split(encode)"  # the compiled (16, 4) / (16, 8) / (5, 4) encode of a small call
JIT, TC = "k_rs_jit(encode)", "k_rs_tc(encode)"
SYN, PREP, DTC = "k_decode_prepare_syn", "k_decode_prepare", "k_rs_tc(decode)"
DEGRADED = ["k_degraded_prepare", ENC, "k_degraded_compare", "k_degraded_finalise"]
JIT10 = [SYN, "k_jit10_emit", "k_rs_jit10(decode)"]
NAMES = {
    "encode_blocks-64-32-rs-auto": ["k_rs_bs(encode)"],
    "encode_blocks-64-32-rs-compiled": ["k_rs_bs(encode)"],
    "encode_blocks-64-32-rs-generated": [JIT],
    "encode_blocks-64-32-rs-threaded": [TC],
    "encode_blocks-64-32-rs-karatsuba": [JIT],
    "encode_blocks-5-4-rs-auto": [ENC],
    "encode_blocks-5-4-rs-compiled": [ENC],
    "encode_blocks-5-4-rs-generated": [JIT],
    "encode_blocks-5-4-rs-threaded": [TC],
    "encode_blocks-5-4-rs-karatsuba": [ENC],
    "encode_blocks-24-20-cauchy-auto": [JIT],
    "encode_blocks-24-20-cauchy-compiled": [JIT],
    "encode_blocks-24-20-cauchy-generated": [JIT],
    "encode_blocks-24-20-cauchy-threaded": [TC],
    "encode_blocks-24-20-cauchy-karatsuba": [JIT],
    "ec_encode_data": ["k_rs_jit(ec_encode_data)"],
    "ec_encode_data_update": [],
    "gf_vect_dot_prod": ["k_rs_jit(ec_encode_data)"],
    "gf_vect_mad": [],
    "gf_vect_mul": ["k_rs_jit(ec_encode_data)"],
    "ec_encode_data-threaded": ["k_rs_tc(ec_encode_data)"],
    "ec_encode_data_batch-mixed": ["classify(ec_batch)", "k_rs_jit(ec_batch)", "k_dot_bytes(ec_batch)"],
    "ec_encode_data_batch-aligned32": ["classify(ec_batch)", "k_rs_jit(ec_batch)"],
    "ec_encode_data_batch-threaded": ["classify(ec_batch)", "k_dot_bytes(ec_batch)"],
    "decode_blocks-5-4-auto": ["k_rs_syn_split(decode)"],
    "decode_blocks-5-4-generated": [SYN, "k_jit_emit", "k_rs_jit(decode)"],
    "decode_blocks-5-4-one_matrix": ["k_rs_tc_fused(decode)"],
    "decode_blocks-5-4-general": [PREP, DTC],
    "decode_blocks-24-20-auto": [SYN, DTC],
    "decode_blocks-24-20-generated": JIT10,
    "decode_blocks-24-20-one_matrix": [SYN, DTC],
    "decode_blocks-24-20-general": [PREP, DTC],
    "decode_blocks-70-66-auto": [PREP, DTC, DTC, DTC],
    "decode_blocks-70-66-generated": [SYN, "k_jit10_emit", "k_rs_jitw_passes(decode)", "k_rs_jitw_passes(decode)"],
    "decode_blocks-70-66-one_matrix": [PREP, DTC, DTC, DTC],
    "decode_blocks-70-66-general": [PREP, DTC, DTC, DTC],
    "decode_prepare-apply": [SYN, DTC],
    "decode_prepare-apply-generated": JIT10,
    "decode_general-threaded": [PREP, DTC],
    "decode_general-generated": [PREP, "k_jit_emit", "k_rs_jit(decode)"],
    "decode_blocks-pipelined": JIT10 + JIT10,  # slices of 4 and 1 blocks
    "scrub_blocks-two_pass": [ENC, "k_scrub_compare", "k_scrub_finalise"],
    "scrub_blocks-fused": ["k_rs_bs_scrub", "k_scrub_finalise"],
    "scrub_blocks-generated": ["k_rs_jit_scrub", "k_scrub_finalise"],
    "scrub_degraded_blocks-lanes": DEGRADED,
    "scrub_degraded_blocks-fused": ["k_degraded_prepare", "k_rs_bs_degraded", "k_degraded_finalise"],
    "locate_blocks-two_pass": [ENC, "k_locate_span", "k_locate_finish"],
    "locate_blocks-fused": ["k_rs_bs_locate", "k_locate_finish"],
    "locate_blocks-fused-generated": ["k_rs_jit_locate", "k_locate_finish"],
    "repair_blocks-one_row-two_pass": [ENC, "k_repair_compare", "k_repair_finalise", "k_repair_compare_gated"],
    "repair_blocks-one_row-fused": ["k_rs_bs_repair", "k_repair_finalise", "k_rs_bs_repair_gated"],
    "repair_blocks-one_row-generated": ["k_rs_jit_repair", "k_repair_finalise", "k_rs_jit_repair_gated"],
    "repair_blocks-columns-two_pass": [ENC, "k_repair_compare", "k_repair_finalise"],
    "repair_blocks-columns-fused": ["k_rs_bs_repair", "k_repair_finalise"],
    "repair_blocks-columns-generated": ["k_rs_jit_repair", "k_repair_finalise"],
    "correct_blocks-two_pass": [ENC, "k_correct_compare", "k_correct_finalise"],
    "correct_blocks-fused": ["k_rs_bs_correct", "k_correct_finalise"],
    "correct_blocks-fused-generated": ["k_rs_jit_correct", "k_correct_finalise"],
    "rebuild_blocks-lanes-checked": DEGRADED + ["k_rebuild_prepare", "k_rebuild_blocks"],
    "rebuild_blocks-lanes-unchecked": ["k_rebuild_prepare", "k_rebuild_blocks"],
    "rebuild_blocks-threaded-checked": DEGRADED + ["k_rebuild_wide_prepare", "k_rs_tc(rebuild)"],
    "rebuild_blocks-threaded-unchecked": ["k_rebuild_wide_prepare", "k_rs_tc(rebuild)"],
    "update_blocks-plain": ["k_update_blocks"],
    "update_blocks-delta": ["k_update_blocks"],
    "heal": [ENC, "k_locate_span", "k_locate_finish", "k_rebuild_prepare", "k_rebuild_blocks"],
    "verify_blocks": [],  # these two and the two update calls of the pointer ABI are not timed
    "fill_synthetic": [],
}


# ---- fixtures -------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    yield from gf.device_context()


@pytest.fixture(scope="module")
def bctx():
    """The builder context: makes the states, stays on the null stream."""
    yield from gf.device_context()


@pytest.fixture(scope="module")
def streams():
    """The two side streams of the module."""
    assert torch.cuda.is_available(), "GPU test needs a HIP device"
    return torch.cuda.Stream(), torch.cuda.Stream()


@pytest.fixture(scope="module")
def gate():
    assert torch.cuda.is_available(), "GPU test needs a HIP device"
    return sg.Gate()


# ---- premise checks --------------------------------------------------------------

def test_premise_the_gate_does_not_hold_the_null_stream(gate, streams):
    """A fill enqueued on the null stream completes while the event behind
    the gate is pending, and the gate lasts what it was calibrated to."""
    s = streams[0]
    ms = gate.measure(s)
    print(f"GATE cycles_per_ms {gate.cycles_per_ms:.0f} probe_ms {gate.probe_ms:.3f} gate_ms {ms:.2f}")
    assert 0.5 * sg.GATE_MS <= ms <= sg.GATE_CAP_MS, ms
    t = torch.zeros(1 << 20, dtype=torch.uint8, device=dev())
    torch.cuda.synchronize()
    g = gate.close(s)
    done = torch.cuda.Event()
    t.fill_(7)
    done.record()
    done.synchronize()
    pending = not g.query()
    s.synchronize()
    assert pending, "the null stream waited for the gate: nothing here could detect work on the wrong stream"
    assert int(t.sum().item()) == 7 << 20


CONTROLS = ("encode_blocks-24-20-cauchy-generated", "scrub_blocks-two_pass", "repair_blocks-columns-two_pass")


@pytest.mark.parametrize("ident", CONTROLS)
def test_premise_negative_control(ctx, bctx, gate, streams, ident):
    """The context deliberately left on the null stream while the true inputs
    arrive behind the gate: the call meets decoys, and what is found behind
    the gate must DIFFER from the expectation."""
    _, kern, make = CASES[ident]
    case = make(bctx, 0)
    with choices(ctx, kern):
        want, _ = sg.ordinary(ctx, case)
        assert ctx.get_stream() == 0
        r = sg.gated(ctx, gate, case, streams[0], move=False)
    n, where = case.differs(r.result, want)
    print(f"CONTROL {ident}: {n} bytes differ, the first in {where}")
    assert r.entry and r.closed and n > 0, "a call on the wrong stream went unnoticed"


# ---- every entry point, warm and cold -----------------------------------------------

@pytest.mark.parametrize("ident", list(CASES))
def test_warm(ctx, bctx, gate, streams, ident):
    _, kern, make = CASES[ident]
    case = make(bctx, 0)
    with choices(ctx, kern):
        r, _ = sg.warm(ctx, gate, case, streams[0], NAMES[ident])
    print(f"WARM {ident}: host_ms {r.ms:.3f}")


def cold_variant(ident):
    """A variant of its own per case, so that no cold matrix has been seen by
    the context in another case (variants 0 and 1 are the warm state and the
    decoy)."""
    return 2 + list(CASES).index(ident)


@pytest.mark.parametrize("ident", list(CASES))
def test_cold(ctx, bctx, gate, streams, ident):
    _, kern, make = CASES[ident]
    first, case = make(bctx, 0), make(bctx, cold_variant(ident))
    with choices(ctx, kern):
        r, names = sg.cold(ctx, gate, first, case, streams[0], ident, NAMES[ident])
    print(f"COLD {ident}: closed {r.closed} host_ms {r.ms:.2f}")


# ---- sequences ---------------------------------------------------------------------

def run_sequence(ctx, gate, kern, cases, streams_of, first_use=()):
    """The cases' ordinary runs (each checked by its model; they also warm the
    context), then the same calls behind one gate on the streams given; every
    call's result must be its ordinary run's.  The cases in first_use have a
    matrix the context has not seen (and the sizes of a case that has run):
    their ordinary runs come after the sequence, so that the gated call is the
    one that builds the program."""
    with choices(ctx, kern):
        wants = {i: sg.ordinary(ctx, c)[0] for i, c in enumerate(cases) if i not in first_use}
        steps = [(ctx, c, st) for c, st in zip(cases, streams_of)]
        results, closed = sg.sequence(gate, steps, streams_of[0])
        print(f"SEQUENCE gate closed at each return: {closed}")
        wants.update({i: sg.ordinary(ctx, cases[i])[0] for i in first_use})
    for i, (c, got) in enumerate(zip(cases, results)):
        c.same(got, wants[i], f"call {i + 1} of the sequence")


UNDER_LOAD = {
    # call 2 re-encodes into the parity scratch call 1's compare still reads
    "two_pass-scrub": ({"scrub": "two_pass"}, lambda b, v: Scrub(b, 16, 4, "rs", v)),
    # call 2 re-emits into the executable buffer call 1's decode still runs
    "generated-decode": ({"decode": "generated"}, lambda b, v: Decode(b, 24, 20, v, 32768)),
    # call 2 builds a second program through the code stage
    "generated-scrub": ({"scrub": "generated"}, lambda b, v: Scrub(b, 10, 4, "cauchy", v)),
    "ec_encode_data_batch": ({}, lambda b, v: Batch(b, False, v)),
}


@pytest.mark.parametrize("ident", list(UNDER_LOAD))
def test_set_stream_under_load(ctx, bctx, gate, streams, ident):
    """Call 1 gated on s1, rsgpu_set_stream(s2), at once call 2 on other
    buffers with another matrix or other lists."""
    kern, make = UNDER_LOAD[ident]
    second = 80 + list(UNDER_LOAD).index(ident)  # a matrix of this test alone
    run_sequence(ctx, gate, kern, [make(bctx, 0), make(bctx, second)], [streams[0], streams[1]], first_use=(1,))


def test_two_pipelined_decodes_back_to_back(ctx, bctx, gate, streams):
    """Two decodes through the second stream with different lists, on one
    gated stream."""
    cases = [Decode(bctx, 24, 20, 0, blocks=5), Decode(bctx, 24, 20, 2, blocks=5)]
    run_sequence(ctx, gate, {"decode": "generated", "pipeline": 2}, cases, [streams[0], streams[0]])


class CorrectThenRepair(Correct):
    """rsgpu_correct_blocks, then rsgpu_repair_blocks (columns) on the same
    blocks, the second report in `report2`."""

    def more(self, ar):
        super().more(ar)
        ar.flat("report2", 24 * self.B)

    writes = ("report", "report2", "src", "par")

    def call(self, ctx):
        super().call(ctx)
        ctx.repair_blocks(*self.blocks_args(), self.ar.ptr("report2"), coef=self.coef, mode="columns")

    def model(self, before, after):
        src, par = self.rows(before, "src"), self.rows(before, "par")
        first = [cm.correct(self.c, src[b], par[b], 2) for b in range(self.B)]
        want = [rpm.repair(self.c, w[0], w[1], "columns") for w in first]
        gf.same(self.flat(after, "report", rsgpu.CORRECT_REPORT_DTYPE), [w[2] for w in first], CORRECT_FIELDS)
        gf.same(self.flat(after, "report2", rsgpu.REPAIR_REPORT_DTYPE), [w[2] for w in want], gf.REPAIR_FIELDS)
        for b, w in enumerate(want):
            assert np.array_equal(self.rows(after, "src")[b], w[0]) and np.array_equal(self.rows(after, "par")[b], w[1])


def test_correct_then_repair_back_to_back(ctx, bctx, gate, streams):
    case = CorrectThenRepair(bctx, 16, 8, "rs", 0)
    want, _ = sg.ordinary(ctx, case)
    r = sg.gated(ctx, gate, case, streams[0])
    assert r.entry
    case.same(r.result, want, "behind the gate")


class Eviction(sg.Case):
    """66 (5, 3) matrices through rsgpu_ec_encode_data at len 32 on one data
    block: the context's cache holds 64 programs, so the last two calls evict
    the programs of the first two while their kernels wait behind the gate."""
    N, LEN = 66, 32

    def __init__(self):
        rng = np.random.default_rng(66)
        self.mats = rng.integers(1, 256, (self.N, 3, 5), dtype=np.uint8)
        self.tables = [rsgpu.ec_init_tables(5, 3, m) for m in self.mats]
        self.ar = sg.arena(self.layout, dev())
        self.decoy, self.true = sg.noise_state(self.ar, 1), sg.noise_state(self.ar, 2)

    def layout(self, ar):
        ar.rows("src", 1, 5, self.LEN + PAD, self.LEN)
        ar.rows("out", self.N, 3, self.LEN + PAD, self.LEN)

    def call(self, ctx):
        ar, pitch = self.ar, self.LEN + PAD
        data = [ar.ptr("src") + j * pitch for j in range(5)]
        for i, g in enumerate(self.tables):
            ctx.ec_encode_data(self.LEN, 5, 3, g, data, [ar.ptr("out") + (3 * i + r) * pitch for r in range(3)])

    def verify(self, before, after):
        src, out = sg.host_rows(before, self.ar["src"])[0], sg.host_rows(after, self.ar["out"])
        for i in reversed(range(self.N)):  # the first matrix's outputs last
            assert np.array_equal(out[i], rbm.encode(self.mats[i], src)), f"matrix {i}"


def test_eviction_behind_the_gate(bctx, gate, streams):
    """A context of its own, so that its cache starts empty."""
    case = Eviction()
    c = rsgpu.Context(0)
    c.set_torch_stream()
    try:
        r = sg.gated(c, gate, case, streams[0])
        assert r.entry
        print(f"EVICTION 66 calls took {r.ms:.1f} ms on the host, gate closed at the return: {r.closed}")
        want = case.true.cpu().numpy()
        case.verify(want, r.result)
        src = case.ar["src"]
        assert np.array_equal(r.result[src.start: src.end], want[src.start: src.end])
    finally:
        torch.cuda.synchronize()
        c.close()


def test_two_contexts(ctx, bctx, gate, streams):
    """Context A gated on sA with one matrix; context B on sB with another
    runs to completion meanwhile, and both are right ("distinct contexts are
    independent").  That B does not wait for A's gate is asserted where the
    two streams are seen not to share a hardware queue (a probe with plain
    fills, first): in a process that has opened many streams they may."""
    kern = {"encode": "generated"}
    a, b = Encode(bctx, 24, 20, "cauchy", 0), Encode(bctx, 24, 20, "cauchy", 2)
    sa, sb = streams[0], streams[1]
    apart = sg.independent(gate, sa, sb)
    prev = bctx.get_stream()
    with choices(ctx, kern), choices(bctx, kern):
        want_a, _ = sg.ordinary(ctx, a)
        want_b, _ = sg.ordinary(bctx, b)
        b.ar.t.copy_(b.true)
        torch.cuda.synchronize()
        done = {}

        def meanwhile():
            try:
                bctx.set_stream(sb.cuda_stream)
                b.call(bctx)
                sb.synchronize()
                done["b"] = b.ar.snapshot()
            finally:
                bctx.set_stream(prev)

        r = sg.gated(ctx, gate, a, sa, before_clobber=meanwhile)
    print(f"TWO CONTEXTS streams apart: {apart}; B complete with A's gate closed: {r.clobbered}")
    assert r.entry and r.closed
    b.same(done["b"], want_b, "context B")
    a.same(r.result, want_a, "context A")
    assert r.clobbered or not apart, "context B waited for the gate of context A's stream"


def test_zz_summary(gate):
    print(f"SUMMARY longest_warm_host_ms {gate.longest_warm_ms:.2f} cold_opened {sorted(gate.opened_cold)!r}")
