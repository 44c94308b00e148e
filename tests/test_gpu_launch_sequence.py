"""The launch sequences of the scrub family (include/rsgpu.h rsgpu_scrub_blocks,
rsgpu_repair_blocks, rsgpu_scrub_degraded_blocks, rsgpu_locate_blocks,
rsgpu_correct_blocks, rsgpu_rebuild_blocks), pinned through the timing log: the exact ordered list of record names each entry point produces, for a
compiled code, (5, 4), and for one that is not, (3, 3) with a caller's Cauchy
matrix, on 2 blocks.  ENC stands for whatever a plain encode_blocks call with
the same arguments records; it is captured here, not spelled out.  The
update's names are pinned in tests/test_gpu_update.py.

The decode section below pins rsgpu_decode_blocks, rsgpu_decode_prepare +
rsgpu_decode_apply and rsgpu_decode_general in the same way, under every
decode kernel choice, at the smallest shapes that still take each branch of
the host path; every case also compares the decoded rows with the rows it
erased (overwritten with 0xA5 while the decode runs)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import gpu_family as gf  # noqa: E402
import rsgpu  # noqa: E402
import scrub_model as sm  # noqa: E402

B = 2
COMPILED = (5, 4, None)
CAUCHY = (3, 3, sm.cauchy_matrix(3, 3))
CODES = pytest.mark.parametrize("code", [COMPILED, CAUCHY], ids=["5-4-rs", "3-3-cauchy"])


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU test needs a HIP device"
    c = rsgpu.Context(0)
    c.set_torch_stream()
    yield c
    torch.cuda.synchronize()
    c.set_scrub_kernel("auto")
    c.set_decode_kernel("auto")
    c.set_locate_kernel("auto")
    c.set_degraded_kernel("auto")
    c.set_repair_kernel("auto")
    c.set_rebuild_kernel("auto")
    c.close()


class Rows:
    """B consistent blocks at (len, pitch), 16-byte aligned allocations; row 1
    of block 1 damaged in one column, so that both repair modes have a block
    to write."""

    def __init__(self, ctx, code, L, pitch):
        self.ctx, (self.k, self.e, self.coef), self.L, self.pitch = ctx, code, L, pitch
        dev = torch.device("cuda", 0)
        k, e = self.k, self.e
        self.src = torch.zeros(max(16, B * k * pitch), dtype=torch.uint8, device=dev)
        self.par = torch.zeros(max(16, B * e * pitch), dtype=torch.uint8, device=dev)
        self.calc = torch.zeros_like(self.par)
        self.rep = torch.zeros(B * rsgpu.REPAIR_REPORT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        assert self.src.data_ptr() % 16 == 0 and self.par.data_ptr() % 16 == 0
        ctx.fill_synthetic(self.src, B * k, L, pitch, 11, 0)
        ctx.encode_blocks(k, e, L, pitch, B, self.src, self.par, coef=self.coef)
        if L:
            self.src[(k + 1) * pitch + L // 2] ^= 0x5A
        torch.cuda.synchronize()

    def names(self, call, kernel="auto", locate="auto", degraded="auto"):
        """The record names of one call, under scrub kernel choice `kernel`,
        locate kernel choice `locate` and degraded kernel choice `degraded`."""
        self.ctx.set_scrub_kernel(kernel)
        self.ctx.set_locate_kernel(locate)
        self.ctx.set_degraded_kernel(degraded)
        try:
            return gf.recorded(self.ctx, call)
        finally:
            self.ctx.set_scrub_kernel("auto")
            self.ctx.set_locate_kernel("auto")
            self.ctx.set_degraded_kernel("auto")

    def enc(self):
        """ENC: a plain encode of the same rows, into a buffer of its own."""
        names = self.names(lambda: self.ctx.encode_blocks(self.k, self.e, self.L, self.pitch, B, self.src,
                                                          self.calc, coef=self.coef))
        assert names, "the encode records nothing"
        return names

    def scrub(self, kernel="auto"):
        return self.names(lambda: self.ctx.scrub_blocks(self.k, self.e, self.L, self.pitch, B, self.src, self.par,
                                                        self.rep, coef=self.coef, locate=True), kernel)

    def repair(self, mode, kernel="auto"):
        return self.names(lambda: self.ctx.repair_blocks(self.k, self.e, self.L, self.pitch, B, self.src, self.par,
                                                         self.rep, coef=self.coef, mode=mode), kernel)

    def degraded(self, kernel="auto"):
        lost = torch.tensor([[1, 255], [255, 255]], dtype=torch.uint8, device=self.src.device)
        return self.names(lambda: self.ctx.scrub_degraded_blocks(self.k, self.e, self.L, self.pitch, B, self.src,
                                                                 self.par, 2, lost, self.rep, coef=self.coef),
                          degraded=kernel)

    def locate(self, locate="auto", kernel="auto"):
        rows = torch.zeros(B * 2, dtype=torch.uint8, device=self.src.device)
        return self.names(lambda: self.ctx.locate_blocks(self.k, self.e, self.L, self.pitch, B, self.src, self.par,
                                                         2, rows, self.rep, coef=self.coef), kernel, locate=locate)

    def correct(self):
        rep = torch.zeros(B * rsgpu.CORRECT_REPORT_DTYPE.itemsize, dtype=torch.uint8, device=self.src.device)
        return self.names(lambda: self.ctx.correct_blocks(self.k, self.e, self.L, self.pitch, B, self.src, self.par,
                                                          rep, coef=self.coef, t=1))

    def rebuild(self, check):
        lost = torch.tensor([[1, 255], [255, 255]], dtype=torch.uint8, device=self.src.device)
        return self.names(lambda: self.ctx.rebuild_blocks(self.k, self.e, self.L, self.pitch, B, self.src, self.par,
                                                          2, lost, self.rep, coef=self.coef, check=check))


def test_the_codes_are_what_the_cases_assume():
    assert rsgpu.scrub_locatable(5, 4) and rsgpu.scrub_locatable(3, 3, CAUCHY[2])
    assert np.array_equal(CAUCHY[2], rsgpu.gf_gen_cauchy1_matrix(6, 3)[3:])


def test_scrub_fused(ctx):
    r = Rows(ctx, COMPILED, 64, 64)
    assert r.scrub() == ["k_rs_bs_scrub", "k_scrub_finalise"]
    assert r.scrub("fused") == ["k_rs_bs_scrub", "k_scrub_finalise"]


def test_scrub_two_pass(ctx):
    r = Rows(ctx, COMPILED, 64, 64)
    assert r.scrub("two_pass") == r.enc() + ["k_scrub_compare", "k_scrub_finalise"]
    r = Rows(ctx, CAUCHY, 64, 64)
    for kernel in ("auto", "fused", "two_pass"):  # a caller's matrix never runs fused
        assert r.scrub(kernel) == r.enc() + ["k_scrub_compare", "k_scrub_finalise"]


@CODES
def test_scrub_of_empty_rows(ctx, code):
    assert Rows(ctx, code, 0, 64).scrub() == ["k_scrub_finalise"]


def test_repair_fused(ctx):
    r = Rows(ctx, COMPILED, 64, 64)
    assert r.repair("columns") == ["k_rs_bs_repair", "k_repair_finalise"]
    assert r.repair("one_row") == ["k_rs_bs_repair", "k_repair_finalise", "k_rs_bs_repair_gated"]


@CODES
def test_repair_two_pass(ctx, code):
    r = Rows(ctx, code, 64, 64)
    enc = r.enc()
    assert r.repair("columns", "two_pass") == enc + ["k_repair_compare", "k_repair_finalise"]
    assert r.repair("one_row", "two_pass") == enc + ["k_repair_compare", "k_repair_finalise",
                                                     "k_repair_compare_gated"]


@CODES
def test_repair_of_empty_rows(ctx, code):
    r = Rows(ctx, code, 0, 64)
    assert r.repair("one_row") == ["k_repair_finalise"] and r.repair("columns") == ["k_repair_finalise"]


@CODES
def test_degraded(ctx, code):
    r = Rows(ctx, code, 48, 48)
    assert r.degraded() == ["k_degraded_prepare"] + r.enc() + ["k_degraded_compare", "k_degraded_finalise"]
    r = Rows(ctx, code, 50, 64)
    assert r.degraded() == (["k_degraded_prepare"] + r.enc() +
                            ["k_degraded_compare", "k_degraded_compare(tail)", "k_degraded_finalise"])
    r = Rows(ctx, code, 50, 63)
    assert r.degraded() == ["k_degraded_prepare"] + r.enc() + ["k_degraded_compare(bytes)", "k_degraded_finalise"]
    assert Rows(ctx, code, 0, 64).degraded() == ["k_degraded_prepare"]


@CODES
def test_locate_two_pass(ctx, code):
    r = Rows(ctx, code, 64, 64)
    assert r.locate() == r.enc() + ["k_locate_span", "k_locate_finish"]
    r = Rows(ctx, code, 64, 65)
    assert r.locate() == r.enc() + ["k_locate_span(bytes)", "k_locate_finish"]
    assert Rows(ctx, code, 0, 64).locate() == ["k_locate_finish"]


def test_locate_two_pass_with_a_byte_tail(ctx):
    r = Rows(ctx, CAUCHY, 72, 80)
    assert r.locate() == r.enc() + ["k_locate_span", "k_locate_span(tail)", "k_locate_finish"]


def test_locate_fused(ctx):
    r = Rows(ctx, COMPILED, 64, 64)
    assert r.locate("fused") == ["k_rs_bs_locate", "k_locate_finish"]


def test_locate_generated(ctx):
    r = Rows(ctx, CAUCHY, 64, 64)
    assert r.locate("fused", "generated") == ["k_rs_jit_locate", "k_locate_finish"]


@CODES
def test_correct(ctx, code):
    r = Rows(ctx, code, 64, 64)
    assert r.correct() == r.enc() + ["k_correct_compare", "k_correct_finalise"]
    assert Rows(ctx, code, 0, 64).correct() == ["k_correct_finalise"]


def test_degraded_fused(ctx):
    r = Rows(ctx, COMPILED, 64, 64)
    assert r.degraded("fused") == ["k_degraded_prepare", "k_rs_bs_degraded", "k_degraded_finalise"]


@CODES
def test_rebuild(ctx, code):
    rebuilt = ["k_rebuild_prepare", "k_rebuild_blocks"]
    r = Rows(ctx, code, 64, 64)
    assert r.rebuild(check=False) == rebuilt
    r = Rows(ctx, code, 64, 64)
    checked = ["k_degraded_prepare"] + r.enc() + ["k_degraded_compare", "k_degraded_finalise"]
    assert r.rebuild(check=True) == checked + rebuilt
    assert Rows(ctx, code, 0, 64).rebuild(check=False) == ["k_rebuild_prepare"]


# ---- decode ------------------------------------------------------------------

KERNELS = ("auto", "generated", "one_matrix", "general")
# (5, 4): compiled split code, the single-launch small decode; (6, 3): no
# compiled split, k_rs_tc_fused and the 8-row generated layout; (24, 20): the
# two-wave layout, k_rs_tc in passes; (40, 34): e > 32, the four-wave names,
# the general plan under one_matrix; (70, 66): e > 64, k_rs_jitw_passes
GEOMS = ((5, 4), (6, 3), (24, 20), (40, 34), (70, 66))
SHAPES = ((4096, 4096), (2048, 2112))  # (len, pitch): pitch == len, pitch != len


class Erased:
    """`blocks` encoded blocks of a k + p row code at (len, pitch), n rows of
    each erased (err: [blocks][n] ascending indices in [0, k + p); drawn among
    the sources when not given).  names() runs a call with the erased rows
    overwritten, then compares what it decoded with the rows saved before."""

    def __init__(self, ctx, k, p, L, pitch, blocks=B, err=None, coef=None):
        self.ctx, self.k, self.p, self.L, self.pitch, self.blocks = ctx, k, p, L, pitch, blocks
        dev = torch.device("cuda", 0)
        if err is None:
            err = rsgpu.erasure_patterns(23, 0, blocks, k, p)
        self.err_host = np.ascontiguousarray(err, np.uint8).reshape(blocks, -1)
        self.n = n = self.err_host.shape[1]
        self.src = torch.zeros(max(16, blocks * k * pitch), dtype=torch.uint8, device=dev)
        self.par = torch.zeros(max(16, blocks * p * pitch), dtype=torch.uint8, device=dev)
        self.out = torch.zeros(max(16, blocks * n * pitch), dtype=torch.uint8, device=dev)
        self.err = torch.from_numpy(np.ascontiguousarray(self.err_host.reshape(-1))).to(dev) if n else self.out
        self.ws = torch.empty(rsgpu.decode_general_workspace_bytes(k, k + p, max(n, 1), blocks), dtype=torch.uint8,
                              device=dev)
        self.status = torch.zeros(blocks, dtype=torch.int32, device=dev)
        self.mism = torch.zeros(blocks, dtype=torch.int64, device=dev)
        assert all(t.data_ptr() % 16 == 0 for t in (self.src, self.par, self.out, self.ws))
        ctx.fill_synthetic(self.src, blocks * k, L, pitch, 29, 0)
        ctx.encode_blocks(k, p, L, pitch, blocks, self.src, self.par, coef=coef)
        # the erased rows saved, then overwritten for good
        rows = torch.cat([self.rows(self.src, k), self.rows(self.par, p)], dim=1)
        self.pick = pick = (torch.arange(blocks, device=dev)[:, None],
                            torch.from_numpy(self.err_host.astype(np.int64)).to(dev))
        self.want = rows[pick][:, :, :L].clone()
        rows[pick] = 0xA5
        self.rows(self.src, k)[:] = rows[:, :k]
        self.rows(self.par, p)[:] = rows[:, k:]
        torch.cuda.synchronize()

    def rows(self, t, r):
        return t[: self.blocks * r * self.pitch].view(self.blocks, r, self.pitch)

    def names(self, call, kernel="auto", blocks=None, check=True):
        """The record names of call(blocks) under decode kernel choice `kernel`;
        check: the first `blocks` blocks are decoded as they were erased."""
        nb = self.blocks if blocks is None else blocks
        self.ctx.set_decode_kernel(kernel)
        try:
            self.recs = gf.recorded(self.ctx, lambda: call(nb), blocks=True)
        finally:
            self.ctx.set_decode_kernel("auto")
        torch.cuda.synchronize()
        if check and self.n:
            assert (self.status[:nb] == 0).all(), self.status[:nb]
            assert torch.equal(self.rows(self.out, self.n)[:nb, :, : self.L], self.want[:nb]), "decoded rows differ"
        return [n for n, _ in self.recs]

    def args(self, nb):
        """What the decode entry points start with; the outputs and statuses of an earlier call gone."""
        self.out.fill_(0x3C)
        self.status.fill_(7)
        return self.k, self.p, self.L, self.pitch, nb, self.src, self.par

    def decode(self, nb):
        self.ctx.decode_blocks(*self.args(nb), self.err, self.out, self.ws, self.status)

    def prepare(self, nb):
        self.ctx.decode_prepare(*self.args(nb), self.err, self.out, self.ws, self.status)

    def apply(self, nb):  # after prepare(nb): its statuses and workspace
        self.ctx.decode_apply(self.k, self.p, self.L, self.pitch, nb, self.src, self.par, self.out, self.ws,
                              self.status)

    def general(self, matrix):
        def call(nb):
            k, _, L, pitch, nb, src, par = self.args(nb)
            self.ctx.decode_general(k, k + self.p, L, pitch, nb, matrix, src, par, self.err, self.n, self.out, self.ws,
                                    self.status)
        return call


def set_pipeline(ctx, n):
    f = rsgpu.testhooks().rsgpu_internal_set_decode_pipeline
    f.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert f(ctx._h, n) == 0


SYN, PREP = "k_decode_prepare_syn", "k_decode_prepare"
TC, DOT = "k_rs_tc(decode)", "k_dot_generic(decode)"
JIT8 = [SYN, "k_jit_emit", "k_rs_jit(decode)"]
GENERAL_JIT = [PREP, "k_jit_emit", "k_rs_jit(decode)"]
# what decode_blocks records per geometry and kernel choice, at both SHAPES
DECODE_BLOCKS = {
    (5, 4): {"auto": ["k_rs_syn_split(decode)"], "generated": JIT8, "one_matrix": ["k_rs_tc_fused(decode)"],
             "general": [PREP, TC]},
    (6, 3): {"auto": ["k_rs_tc_fused(decode)"], "generated": JIT8, "one_matrix": ["k_rs_tc_fused(decode)"],
             "general": [PREP, TC]},
    (24, 20): {"auto": [SYN, TC], "generated": [SYN, "k_jit10_emit", "k_rs_jit10(decode)"], "one_matrix": [SYN, TC],
               "general": [PREP, TC]},
    (40, 34): {"auto": [PREP, TC, TC], "generated": [SYN, "k_jit10_emit", "k_rs_jit10x4(decode)"],
               "one_matrix": [PREP, TC, TC], "general": [PREP, TC, TC]},
    (70, 66): {"auto": [PREP, TC, TC, TC],
               "generated": [SYN, "k_jit10_emit", "k_rs_jitw_passes(decode)", "k_rs_jitw_passes(decode)"],
               "one_matrix": [PREP, TC, TC, TC], "general": [PREP, TC, TC, TC]},
}
# (prepare, apply) as two calls, L = 4096
PREPARE_APPLY = {
    (6, 3): {"auto": ([SYN], [TC]), "generated": ([SYN, "k_jit_emit"], ["k_rs_jit(decode)"]),
             "one_matrix": ([SYN], [TC]), "general": ([PREP], [TC])},
    (24, 20): {"auto": ([SYN], [TC]), "generated": ([SYN, "k_jit10_emit"], ["k_rs_jit10(decode)"]),
               "one_matrix": ([SYN], [TC]), "general": ([PREP], [TC])},
}
SINGLE_LAUNCH = (["k_rs_syn_split(decode)"], ["k_rs_tc_fused(decode)"])


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("L,pitch", SHAPES)
@pytest.mark.parametrize("k,e", GEOMS)
def test_decode_blocks(ctx, k, e, L, pitch, kernel):
    r = Erased(ctx, k, e, L, pitch)
    assert r.names(r.decode, kernel) == DECODE_BLOCKS[k, e][kernel]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k,e", list(PREPARE_APPLY))
def test_decode_prepare_then_apply(ctx, k, e, kernel):
    """Two calls record what decode_blocks records in one, wherever that takes
    neither the single-launch small decode nor the pipelined path (2 blocks:
    never pipelined)."""
    r = Erased(ctx, k, e, 4096, 4096)
    prep = r.names(r.prepare, kernel, check=False)
    app = r.names(r.apply, kernel)
    assert (prep, app) == PREPARE_APPLY[k, e][kernel]
    whole = DECODE_BLOCKS[k, e][kernel]
    assert prep + app == whole or whole in SINGLE_LAUNCH


def test_decode_general_plan_generated(ctx):
    """The general kernel from kGeneralJitMinTiles (48) column tiles."""
    r = Erased(ctx, 6, 3, 98304, 98304)
    assert r.names(r.decode, "general") == GENERAL_JIT


@pytest.mark.parametrize("kernel", ["auto", "general"])
@pytest.mark.parametrize("L,pitch", [(33, 64), (4096, 4097)])
def test_decode_unaligned(ctx, L, pitch, kernel):
    r = Erased(ctx, 6, 3, L, pitch)
    assert r.names(r.decode, kernel) == [PREP, DOT]


@pytest.mark.parametrize("with_matrix", [False, True], ids=["rs", "cauchy"])
@pytest.mark.parametrize("L,pitch,want", [(4096, 4096, [PREP, TC]), (98304, 98304, GENERAL_JIT), (33, 64, [PREP, DOT])],
                         ids=["general_tc", "general_jit", "general_dot"])
def test_decode_general(ctx, L, pitch, want, with_matrix):
    """(6, 3) as m = 9 rows with two of them lost, a source and a parity row in
    block 0: gf_gen_rs_matrix, or a caller's Cauchy matrix."""
    k, m = 6, 9
    matrix = rsgpu.gf_gen_cauchy1_matrix(m, k) if with_matrix else None
    r = Erased(ctx, k, m - k, L, pitch, err=[[1, 7], [0, 4]], coef=None if matrix is None else matrix[k:])
    assert r.names(r.general(matrix)) == want


@pytest.mark.parametrize("parts", [2, 3])
def test_decode_pipelined(ctx, parts):
    """5 blocks in slices of 4 and 1 (at most one slice per two blocks, slices
    of an even number of blocks): prepare, emission and decode once per slice,
    in slice order, with the slice's block count."""
    r = Erased(ctx, 24, 20, 4096, 4096, blocks=5)
    set_pipeline(ctx, parts)
    try:
        r.names(r.decode, "generated")
    finally:
        set_pipeline(ctx, -1)
    assert r.recs == [(n, nb) for nb in (4, 1) for n in (SYN, "k_jit10_emit", "k_rs_jit10(decode)")]


@pytest.mark.parametrize("kernel,prep", [("auto", [SYN]), ("generated", [SYN, "k_jit_emit"]), ("one_matrix", [SYN]),
                                         ("general", [PREP])])
def test_decode_of_nothing(ctx, kernel, prep):
    """e == 0 records nothing; len == 0 prepares and does not apply."""
    r = Erased(ctx, 6, 0, 4096, 4096)
    assert r.names(r.decode, kernel) == []
    r = Erased(ctx, 6, 3, 0, 64)
    assert r.names(r.decode, kernel) == prep


def test_decode_sliced_above_a_grid(ctx):
    """65537 blocks run as 65535 and then 2, each slice planned on its own."""
    r = Erased(ctx, 6, 3, 32, 32, blocks=65537)
    first, rest = r.names(r.decode, "one_matrix", 65535), r.names(r.decode, "one_matrix", 2)
    assert (first, rest) == ([SYN, TC], ["k_rs_tc_fused(decode)"])
    assert r.names(r.decode, "one_matrix") == first + rest


def test_verify_blocks_counts_and_records_nothing(ctx):
    r = Erased(ctx, 6, 3, 4096, 4096)
    r.names(r.decode)
    r.rows(r.src, 6)[r.pick[0], r.pick[1], :4096] = r.want  # the sources as they were encoded

    def verify(nb):
        r.mism.zero_()
        ctx.verify_blocks(6, 3, 4096, 4096, nb, r.src, r.out, r.err, r.mism)

    assert r.names(verify, check=False) == [] and r.mism.tolist() == [0, 0]
    r.rows(r.out, 3)[1, 2, 5] ^= 1
    r.rows(r.out, 3)[1, 0, 4095] ^= 0x80
    assert r.names(verify, check=False) == [] and r.mism.tolist() == [0, 2]
