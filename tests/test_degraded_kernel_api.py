"""rsgpu_set_degraded_kernel on the CPU (include/rsgpu.h): the choices of the
wrapper and of the header agree, the symbol is exported and bound, a null
context is an argument error; the constant-times-planes multiply of the fused
kernel's reduction (csrc/plane_mul.h, through the test-hooks library) equals
gf_mul byte by byte; and the lists and damage of the GPU cases
(tests/test_gpu_degraded_fused.py) give, on the model alone, blocks of every
status, so that the GPU comparison cannot pass on an all-clean batch."""
import ctypes as C
import os
import re

import numpy as np

import degraded_model as dm
import rsgpu
import scrub_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rsgpu.h")
CODES = [(16, 4), (16, 8), (64, 32), (64, 16), (100, 20), (5, 4), (20, 7)]


def test_the_wrapper_s_choices():
    assert rsgpu.DEGRADED_KERNELS == {"auto": 0, "two_pass": 1, "fused": 2}
    assert "DEGRADED_KERNELS" in rsgpu.__all__
    assert "rsgpu_set_degraded_kernel" in rsgpu.EXPORTED_SYMBOLS
    assert callable(rsgpu.Context.set_degraded_kernel)


def test_the_header_s_constants():
    txt = open(HEADER).read()
    got = dict(re.findall(r"^#define RSGPU_DEGRADED_(AUTO|TWO_PASS|FUSED)\s+(\d+)\s*$", txt, re.M))
    assert {k.lower(): int(v) for k, v in got.items()} == rsgpu.DEGRADED_KERNELS
    assert re.search(r"^int rsgpu_set_degraded_kernel\(rsgpu_ctx \*ctx, int kernel\);", txt, re.M)


def test_the_symbol_is_exported_and_bound():
    fn = rsgpu.lib().rsgpu_set_degraded_kernel
    assert fn.restype is C.c_int and fn.argtypes == [C.c_void_p, C.c_int]


def test_null_context_is_an_argument_error():
    for kernel in (0, 1, 2, 3, -1):
        assert rsgpu.lib().rsgpu_set_degraded_kernel(None, kernel) == -1


def planes_to_bytes(p):
    """p: 8 uint32 planes, plane a holding bit a of 32 bytes -> the 32 bytes."""
    bits = (p[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1  # [plane a][byte j]
    return (bits.astype(np.uint32) << np.arange(8, dtype=np.uint32)[:, None]).sum(0).astype(np.uint8)


def test_the_plane_multiply_is_gf_mul():
    fn = rsgpu.testhooks().rsgpu_internal_plane_mul_acc
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(3)
    assert fn(256, None, None) == -1
    for c in range(256):
        s = rng.integers(0, 1 << 32, 8, dtype=np.uint64).astype(np.uint32)
        t = rng.integers(0, 1 << 32, 8, dtype=np.uint64).astype(np.uint32)
        before = planes_to_bytes(t)
        assert fn(c, s.ctypes.data, t.ctypes.data) == 0
        want = before ^ sm.gf_mul(np.full(32, c, np.uint8), planes_to_bytes(s))
        assert (planes_to_bytes(t) == want).all(), c


def mixed_lists(k, e, u, B, seed=5):
    """tests/gpu_family.py mixed_lists, which imports torch; the same draws."""
    rng = np.random.default_rng(seed)
    nmax = min(u, e)
    lost = np.full((B, u), dm.NONE, np.uint8)
    for b in range(B):
        n = b % (nmax + 1) if B > 1 else min(nmax, max(1, e - 2))
        kind = (b // (nmax + 1)) % 3
        if kind == 0:
            rows = rng.choice(k, min(n, k), replace=False)
        elif kind == 1:
            rows = k + rng.choice(e, n, replace=False)
        else:
            rows = rng.choice(k + e, n, replace=False)
        lost[b] = dm.pad(np.sort(rows), u)
    if B > 2:
        n = min(nmax, max(1, e - 2))
        lost[0] = dm.pad(np.arange(n), u)
        lost[1] = dm.pad(np.arange(k + e - n, k + e), u)
    return lost


def test_the_gpu_cases_meet_every_status_on_the_model():
    """(5, 4), u = 4, 67 blocks of 4160 bytes: mixed_lists and one list out of
    order, consistent blocks damaged as gpu_family.damage's kinds 1 and 3
    damage them; the model alone names every status."""
    k, e, u, B, L = 5, 4, 4, 67, 4160
    c = sm.rs_matrix(k, e)
    lost = mixed_lists(k, e, u, B)
    lost[9] = [3, 1, dm.NONE, dm.NONE]
    rng = np.random.default_rng(1)
    seen = set()
    for b in range(B):
        syn = np.zeros((e, L), np.uint8)  # consistent: the lost rows' bytes cancel
        rows = dm.list_rows(lost[b], k, e)
        surv = [r for r in range(k + e) if r not in (rows or [])]
        kind = (b // 5) % 3
        for r in surv[:kind]:  # 0, 1 or 2 damaged survivors, in different columns
            col = int(rng.integers(0, L))
            syn[:, col] ^= sm.gf_mul(dm.row_column(c, r), np.uint8(rng.integers(1, 256)))
        seen.add(dm.report_syn(c, syn, lost[b], True)[1])
    assert {dm.CLEAN, dm.ONE_ROW, dm.DAMAGED, dm.UNCHECKED, dm.BAD_LIST} <= seen, seen
