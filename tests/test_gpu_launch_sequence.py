"""The launch sequences of the scrub family (include/rsgpu.h rsgpu_scrub_blocks,
rsgpu_repair_blocks, rsgpu_scrub_degraded_blocks), pinned through the timing
log: the exact ordered list of record names each entry point produces, for a
compiled code, (5, 4), and for one that is not, (3, 3) with a caller's Cauchy
matrix, on 2 blocks.  ENC stands for whatever a plain encode_blocks call with
the same arguments records; it is captured here, not spelled out.  The
update's names are pinned in tests/test_gpu_update.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

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

    def names(self, call, kernel="auto"):
        """The record names of one call, under scrub kernel choice `kernel`."""
        self.ctx.set_scrub_kernel(kernel)
        self.ctx.timing_enable(True)
        try:
            self.ctx.timing_read()
            call()
            return [n for n, _, _ in self.ctx.timing_read()]
        finally:
            self.ctx.timing_enable(False)
            self.ctx.set_scrub_kernel("auto")

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

    def degraded(self):
        lost = torch.tensor([[1, 255], [255, 255]], dtype=torch.uint8, device=self.src.device)
        return self.names(lambda: self.ctx.scrub_degraded_blocks(self.k, self.e, self.L, self.pitch, B, self.src,
                                                                 self.par, 2, lost, self.rep, coef=self.coef))


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
