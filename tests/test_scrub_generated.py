"""The generated scrub (rsgpu_set_scrub_kernel RSGPU_SCRUB_GENERATED) on the
CPU: the constant in the header and the wrapper, the setter's argument check
without a device, and the kernels' location rule (rs_lane.h scrub_locate_row,
through the test hook library) against the model's brute force over rows.  The
device path is in tests/test_gpu_scrub_generated.py (-m gpu)."""
import ctypes as C
import os
import re

import numpy as np

import rsgpu
import scrub_model as sm

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "rsgpu.h")


def test_header_defines_generated_as_3():
    with open(HEADER) as f:
        text = f.read()
    found = dict(re.findall(r"^#define (RSGPU_SCRUB_(?:AUTO|FUSED|TWO_PASS|GENERATED)) (\d+)$", text, re.M))
    assert found == {"RSGPU_SCRUB_AUTO": "0", "RSGPU_SCRUB_FUSED": "1", "RSGPU_SCRUB_TWO_PASS": "2",
                     "RSGPU_SCRUB_GENERATED": "3"}


def test_wrapper_names_generated():
    assert rsgpu.SCRUB_KERNELS["generated"] == 3
    assert sorted(rsgpu.SCRUB_KERNELS.values()) == [0, 1, 2, 3]


def test_setter_with_a_null_context_is_an_argument_error():
    L = rsgpu.lib()
    assert L.rsgpu_set_scrub_kernel(None, 3) == -1
    assert L.rsgpu_set_scrub_kernel(None, 4) == -1


def rowtab_of(c):
    """ratio c[1][j] / c[0][j] -> j, 255 for none: what the host uploads."""
    tab = np.full(256, 255, np.uint8)
    for j in range(c.shape[1]):
        tab[int(sm.gf_mul(c[1, j], sm.gf_inv(int(c[0, j]))))] = j
    return tab


def locate(hook, c, tab, s):
    e, k = c.shape
    s = np.ascontiguousarray(s, np.uint8)
    return hook(k, e, tab.ctypes.data, c.ctypes.data, s.ctypes.data)


def test_location_rule_agrees_with_the_model():
    """Per locatable matrix: the columns single-row damage makes (every row,
    several x), columns of two damaged rows, and random columns.  The model
    finds at most one explaining row for a locatable matrix; the rule must
    name exactly that row, or none."""
    hook = rsgpu.testhooks().rsgpu_internal_scrub_locate_row
    hook.restype = C.c_int
    hook.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(31)
    seen = {"source": 0, "parity": 0, "none": 0}
    for k, e, kind in [(10, 4, "rs"), (10, 4, "cauchy"), (6, 3, "cauchy"), (5, 2, "rs"), (9, 34, "rs"),
                       (17, 3, "rs")]:
        c = np.ascontiguousarray(sm.rs_matrix(k, e) if kind == "rs" else sm.cauchy_matrix(k, e))
        assert sm.locatable(c)
        tab = rowtab_of(c)
        cols = []
        for row in range(k + e):
            for x in (1, 0x80, int(rng.integers(1, 256))):
                cols.append(sm.damage(c, np.zeros((e, 1), np.uint8), row, [0], [x])[:, 0])
        for _ in range(40):  # two rows in one column
            r1, r2 = rng.choice(k + e, 2, replace=False)
            s = sm.damage(c, np.zeros((e, 1), np.uint8), int(r1), [0], [int(rng.integers(1, 256))])
            cols.append(sm.damage(c, s, int(r2), [0], [int(rng.integers(1, 256))])[:, 0])
        for _ in range(40):  # anything, zeros in s_0 or s_1 included
            s = rng.integers(0, 256, e, dtype=np.uint8)
            s[: int(rng.integers(0, 3))] = 0
            cols.append(s)
        for s in cols:
            if not s.any():
                continue
            rows = sm.explaining_rows(c, s)
            assert len(rows) <= 1
            got = locate(hook, c, tab, s)
            assert got == (rows[0] if rows else -1), (k, e, kind, s, rows, got)
            seen["none" if not rows else "source" if rows[0] < k else "parity"] += 1
    assert all(seen.values()), seen
