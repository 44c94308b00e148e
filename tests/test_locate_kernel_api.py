"""rsgpu_set_locate_kernel on the CPU (include/rsgpu.h): the choices of the
wrapper and of the header agree, and a null context is an argument error.
tests/test_capi.py checks the symbol against the header, the version script
and the binding table; tests/test_gpu_locate_fused.py runs the kernels."""
import os
import re

import rsgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rsgpu.h")


def test_the_wrapper_s_choices():
    assert rsgpu.LOCATE_KERNELS == {"auto": 0, "two_pass": 1, "fused": 2}
    assert "LOCATE_KERNELS" in rsgpu.__all__
    assert "rsgpu_set_locate_kernel" in rsgpu.EXPORTED_SYMBOLS
    assert callable(rsgpu.Context.set_locate_kernel)


def test_the_header_s_constants():
    txt = open(HEADER).read()
    got = dict(re.findall(r"^#define RSGPU_LOCATE_(AUTO|TWO_PASS|FUSED)\s+(\d+)\s*$", txt, re.M))
    assert {k.lower(): int(v) for k, v in got.items()} == rsgpu.LOCATE_KERNELS


def test_null_context_is_an_argument_error():
    assert rsgpu.lib().rsgpu_set_locate_kernel(None, 0) == -1
